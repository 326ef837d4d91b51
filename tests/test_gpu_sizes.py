"""GPU parity at the BASELINE.json sizes: full-model GRADIENTS of DPOT-Tiny / -Small / -Medium / -Large(256^2) against
the CPU oracle, and the configs[4] workload - a 20-step auto-regressive DPOT-Large rollout train step - with and
without activation recomputation.  (The toy-size golden tests live in test_gpu_model.py.)"""
import functools
import os
from collections import OrderedDict

import pytest
import torch

from helpers import RTOL, assert_close, set_tune, tune_value
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu


def build(kw, salt):
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**kw)
    m = DPOTNet(**kw)
    m.load_state_dict(R.recipe_state_dict(cfg, salt=salt))
    return m.cuda(), cfg


def _rel(a, b):
    return abs(a - b) / (abs(b) + 1e-30)


@functools.lru_cache(maxsize=2)
def _recipe_sd(name, salt):
    return R.recipe_state_dict(R.DPOTConfig(**getattr(R, name)), salt=salt)


@functools.lru_cache(maxsize=1)
def _oracle_case(name, B):
    """inputs + the CPU oracle's forward / dx / every parameter gradient for one (config, batch); cached so that the
    fp32 and the bf16-channel-MLP test of the same case share one oracle run (DPOT-L at B=4: ~12 TFLOP on the host)"""
    cfg = R.DPOTConfig(**getattr(R, name))
    S = cfg.img_size
    x = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=71)
    up_y = R.recipe_input((B, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3
    up_c = R.recipe_input((B, cfg.n_cls), salt=73) * 0.3
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in _recipe_sd(name, 4).items())
    xo = x.clone().requires_grad_(True)
    yo, co = R.dpot_forward(sd, xo, cfg)
    ((yo * up_y).sum() + (co * up_c).sum()).backward()
    return dict(cfg=cfg, x=x, up_y=up_y, up_c=up_c, y=yo.detach(), c=co.detach(), dx=xo.grad,
                grads=OrderedDict((k, v.grad) for k, v in sd.items()))


def _hip_case(name, oc):
    from dpot_amd import DPOTNet
    m = DPOTNet(**getattr(R, name))
    m.load_state_dict(_recipe_sd(name, 4))
    m.cuda()
    xg = oc["x"].cuda().requires_grad_(True)
    y, c = m(xg)
    ((y * oc["up_y"].cuda()).sum() + (c * oc["up_c"].cuda()).sum()).backward()
    return m, xg, y, c


# batch 2/1/1: the small-batch kernel selections, and DPOT-Tiny at the headline batch - against the CPU oracle run LIVE on the
# GPU box's host (seconds each).  The batches bench.py times for the larger models (BASELINE configs[2..4]: S / M at 32, L at 16
# and - `--config L20` - at 4; panel heights, split-K factors, paired weight-gradient launches, the one-launch AFNO layer and the
# DPOT-L pair-grid rule all depend on the batch) are compared with committed numbers from the imported REFERENCE model instead
# (REF_GOLDEN_CASES below; round 5 - the live oracle runs of those cases cost ~4 min of the GPU gate)
# (DPOT-L at batch 1 - the small-batch selections at 256^2 - is covered by the 20-step rollout tests against the reference's
# g11 numbers, fp32 and bf16)
SIZE_CASES = [("TINY", 2), ("TINY", 32), ("SMALL", 1), ("MEDIUM", 1)]
REF_GOLDEN_CASES = [("SMALL", 32), ("MEDIUM", 32), ("LARGE", 4), ("LARGE", 16)]


@pytest.mark.parametrize("name,B", SIZE_CASES)
def test_full_model_gradients_vs_oracle(name, B):
    """every parameter gradient + dx of the whole model at the BASELINE sizes AND batches (Tiny: nb=4/bs=128, S/M: nb=8,
    mlp_ratio 4, L: 256^2, nb=16/bs=96 edge tiles, out_layer_dim=128 un-fused tail, 32x32 DFT) vs torch autograd on the
    CPU oracle, fp32 path, rtol 1e-4"""
    oc = _oracle_case(name, B)
    m, xg, y, c = _hip_case(name, oc)
    assert_close(y, oc["y"], f"{name} pred")
    assert_close(c, oc["c"], f"{name} cls")
    assert_close(xg.grad, oc["dx"], f"{name} dx")
    worst = 0.0
    for k, p in m.named_parameters():
        assert p.grad is not None, k
        g_ref = oc["grads"][k]
        worst = max(worst, assert_close(p.grad, g_ref, f"{name} d{k}"))
        n_ref = g_ref.double().norm().item()                 # float64 accumulation: torch's fp32 norm of a 10M-element
        assert _rel(p.grad.double().norm().item(), n_ref) <= RTOL, f"{name} |d{k}|"   # tensor is itself off by ~5e-4
    print(f"[{name} B={B}] worst normalised gradient error {worst:.2e}")


def test_full_model_gradients_with_one_launch_afno_layer(monkeypatch):
    """DPOT-Tiny at batch 2 with the ONE-launch AFNO layer forward forced on (csrc/afno_fused.hip; `auto` selects it from
    205 (sample, block) workgroups on, i.e. for DPOT-S / -M at batch 32 - test_vs_reference_golden[SMALL-32 / MEDIUM-32] run it):
    64 channels per GroupNorm group = two groups per workgroup; every gradient vs the oracle at rtol 1e-4, and the
    no-grad forward (S / pre-activation not written) bit-identical to the training forward"""
    from dpot_amd import ops
    set_tune(monkeypatch, afno_layer=1)
    if not (ops.afno_mlp2_supported(4, 128) and ops.afno_mlp3_supported(4, 128) and ops.afno_fused_supported(16, 16, 512, 4, 16, 9)):
        pytest.skip("one-launch AFNO layer switched off")
    calls = []
    real = ops.afno_fused_fwd
    monkeypatch.setattr(ops, "afno_fused_fwd", lambda *a, **k: (calls.append(k.get("save", True)), real(*a, **k))[1])
    oc = _oracle_case("TINY", 2)
    m, xg, y, c = _hip_case("TINY", oc)
    assert calls == [True] * 4, calls
    assert_close(y, oc["y"], "pred")
    assert_close(xg.grad, oc["dx"], "dx")
    for k, p in m.named_parameters():
        assert_close(p.grad, oc["grads"][k], f"d{k}")
        assert _rel(p.grad.double().norm().item(), oc["grads"][k].double().norm().item()) <= RTOL, f"|d{k}|"
    with torch.no_grad():
        y0, c0 = m(oc["x"].cuda())
    assert calls[4:] == [False] * 4, calls
    assert torch.equal(y0, y.detach()) and torch.equal(c0, c.detach())


# Tolerance of the OPT-IN reduced-precision channel MLP (`set_mlp_precision("bf16")`, BASELINE configs[2] "bf16
# channel-MLP on MFMA" and the DPOT-M/L headline mode).  Both operands of fc1 / fc2 (forward, data gradient, weight
# gradient) are rounded to bf16 (8-bit significand, unit round-off u = 2^-9 = 1.95e-3), as is the saved activation
# derivative; products exact, fp32 accumulation.  A K-term dot product of rounded operands carries a relative error of
# about u*sqrt(2/3) = 1.6e-3 of sqrt(sum of squared terms); each block adds its MLP branch to the residual stream, so the
# error of the latent - and of every gradient, which passes the chain forward AND backward - grows like sqrt(depth)
# (independent roundings).  Measured on MI355X (norm-wise ||hip - oracle|| / ||oracle||, worst parameter gradient):
# Tiny 1.0e-2, Small 1.1e-2, Medium 1.5e-2, Large 2.7e-2 = (4.3 .. 5.6)e-3 * sqrt(depth); dx (3.1 .. 4.0)e-3 * sqrt(depth);
# prediction 5e-3 .. 6.5e-3.  Bounds = those laws with 1.5x headroom; element-wise bounds are meaningless at this
# precision.  Everything outside the channel MLP stays fp32 - the fp32 test above is the parity gate, this bounds the mode.
BF16_OUT_TOL = 2e-2                          # prediction, cls
BF16_DX_PER_SQRT_DEPTH = 6e-3
BF16_GRAD_PER_SQRT_DEPTH = 8e-3


def _nrel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return ((a - b).norm() / (b.norm() + 1e-300)).item()


@pytest.mark.parametrize("img,B,mlp", [(64, 3, None), (256, 2, None), (256, 2, "bf16"), (192, 2, None)])
def test_tiny_at_other_resolutions_vs_oracle(img, B, mlp):
    """the DPOT-Tiny architecture on the other latent grids of utils/griddataset.py:35 (64^2 -> 8x8 tokens, 256^2 -> 32x32; round 5:
    192^2 -> 24x24, a 3 * 2^k grid: radix-3 register FFTs):
    every gradient vs the CPU oracle.  8x8: the register FFTs for 8-point lines, 64 tokens per sample; 32x32 at 64 channels per
    group: chunked statistics-only GroupNorm with norm1 applied on the load of rfft2 / irfft2 - here in the fp32 mode too -
    and (bf16 channel MLP) norm2 inside the pack pass, at a second shape besides DPOT-L"""
    from dpot_amd import DPOTNet, ops
    kw = dict(R.TINY, img_size=img)
    cfg = R.DPOTConfig(**kw)
    sd0 = R.recipe_state_dict(cfg, salt=5)
    x = R.recipe_input((B, img, img, cfg.in_timesteps, cfg.in_channels), salt=81)
    up_y = R.recipe_input((B, img, img, cfg.out_timesteps, cfg.out_channels), salt=82) * 0.3
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in sd0.items())
    xo = x.clone().requires_grad_(True)
    yo, co = R.dpot_forward(sd, xo, cfg)
    (yo * up_y).sum().backward()
    ops.set_mlp_precision(mlp)
    try:
        m = DPOTNet(**kw)
        m.load_state_dict(sd0)
        m.cuda()
        xg = x.cuda().requires_grad_(True)
        y, c = m(xg)
        (y * up_y.cuda()).sum().backward()
    finally:
        ops.set_mlp_precision(None)
    if mlp is None:
        assert_close(y, yo.detach(), f"Tiny@{img} pred")
        assert_close(xg.grad, xo.grad, f"Tiny@{img} dx")
        for k, p in m.named_parameters():
            if k.startswith("cls_head."):
                continue
            assert_close(p.grad, sd[k].grad, f"Tiny@{img} d{k}")
    else:
        depth = cfg.depth
        assert _nrel(y, yo) <= BF16_OUT_TOL
        assert _nrel(xg.grad, xo.grad) <= BF16_DX_PER_SQRT_DEPTH * depth ** 0.5
        for k, p in m.named_parameters():
            if k.startswith("cls_head."):
                continue
            assert _nrel(p.grad, sd[k].grad) <= BF16_GRAD_PER_SQRT_DEPTH * depth ** 0.5, k


def test_mlp_precision_is_a_per_model_attribute():
    """the channel-MLP precision is an attribute of the MODEL (`DPOTNet.mlp_precision`), applied around
    its forward / weight derivation / backward - two models of one process run different modes, interleaved, and the
    process-global default is untouched afterwards"""
    from dpot_amd import DPOTNet, ops
    assert ops.mlp_precision() is None
    cfg = R.DPOTConfig(**R.SMALL)
    S = cfg.img_size
    x = R.recipe_input((2, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
    up = (R.recipe_input((2, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()

    def fresh(prec):
        m = DPOTNet(**R.SMALL)
        m.load_state_dict(_recipe_sd("SMALL", 4))
        m.cuda()
        m.mlp_precision = prec
        return m

    def run(m):
        for p in m.parameters():
            p.grad = None
        y, _ = m(x)
        (y * up).sum().backward()
        return y.detach().clone(), m.blocks[0].mlp[0].weight.grad.clone()

    y32, g32 = run(fresh(None))                                  # reference: a plain fp32 process
    a, b = fresh("bf16"), fresh(None)
    ya, _ = a(x)                                                 # forward A (bf16) ...
    yb, _ = b(x)                                                 # ... forward B (fp32) ...
    (ya * up).sum().backward()                                   # ... backward A after B's forward
    (yb * up).sum().backward()
    assert torch.equal(yb, y32) and torch.equal(b.blocks[0].mlp[0].weight.grad, g32), "fp32 model disturbed by its neighbour"
    yA, gA = run(fresh("bf16"))
    assert torch.equal(ya.detach(), yA) and torch.equal(a.blocks[0].mlp[0].weight.grad, gA), "bf16 model not reproducible"
    e = _nrel(ya, y32)
    assert 1e-6 < e <= BF16_OUT_TOL, e
    assert ops.mlp_precision() is None


def test_gemm_precision_is_a_per_model_attribute():
    """the GEMM precision of everything outside the channel MLP is an attribute of the MODEL too
    (`DPOTNet.gemm_precision`, per-thread scopes in ops - ADVICE r4: no temporary write to a process global any more):
    a bf16x6 model (fp32-accurate operand split on every GEMM) and a native-fp32 model run interleaved in one process, the
    backward of each re-applies the forward's mode; the fp32 model is bit-identical to a plain run, the bf16x6 one agrees with
    it at fp32 level but not bit for bit, the process default is untouched"""
    from dpot_amd import DPOTNet, ops
    assert ops.gemm_precision() == "f32" or ops.gemm_precision() == "auto"
    default = ops.gemm_precision()
    cfg = R.DPOTConfig(**R.TINY)
    S = cfg.img_size
    x = R.recipe_input((4, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
    up = (R.recipe_input((4, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()

    def fresh(prec):
        m = DPOTNet(**R.TINY)
        m.load_state_dict(_recipe_sd("TINY", 4))
        m.cuda()
        m.gemm_precision = prec
        return m

    def run(m):
        y, _ = m(x)
        (y * up).sum().backward()
        return y.detach().clone(), m.blocks[0].mlp[0].weight.grad.clone(), m.out_layer[0].weight.grad.clone()

    y32, g32, h32 = run(fresh("f32"))
    a, b = fresh("bf16x6"), fresh("f32")
    ya, _ = a(x)
    yb, _ = b(x)
    (ya * up).sum().backward()                                   # backward of A after B's forward
    (yb * up).sum().backward()
    assert torch.equal(yb, y32) and torch.equal(b.blocks[0].mlp[0].weight.grad, g32)
    assert torch.equal(b.out_layer[0].weight.grad, h32), "fp32 model disturbed by its neighbour"
    assert not torch.equal(ya, y32), "the bf16x6 model ran the native kernels"
    assert _nrel(ya, y32) <= 1e-5 and _nrel(a.out_layer[0].weight.grad, h32) <= 1e-5
    assert ops.gemm_precision() == default


def test_small_model_at_1024_resolution_vs_oracle():
    """the largest resolution utils/griddataset.py:35 lists (1024^2 -> a 128 x 128 latent grid at patch 8): a small DPOT
    (embed 64, depth 2) end to end against the CPU oracle - forward, dx, every parameter gradient; the mixer's DFTs run on
    the 128-point register-FFT kernels (csrc/dft_fast.h, round 4), GroupNorm on the chunked kernels"""
    from dpot_amd import DPOTNet
    kw = dict(R.MINI, img_size=1024, embed_dim=64, in_timesteps=3)
    cfg = R.DPOTConfig(**kw)
    B, S = 1, cfg.img_size
    sd0 = R.recipe_state_dict(cfg, salt=5)
    x = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81)
    up_y = R.recipe_input((B, S, S, cfg.out_timesteps, cfg.out_channels), salt=82) * 0.3
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in sd0.items())
    xo = x.clone().requires_grad_(True)
    yo, _ = R.dpot_forward(sd, xo, cfg)
    (yo * up_y).sum().backward()
    m = DPOTNet(**kw)
    m.load_state_dict(sd0)
    m.cuda()
    xg = x.cuda().requires_grad_(True)
    y, _ = m(xg)
    (y * up_y.cuda()).sum().backward()
    assert_close(y, yo.detach(), "1024^2 pred")
    assert_close(xg.grad, xo.grad, "1024^2 dx")
    for k, p in m.named_parameters():
        if k.startswith("cls_head."):
            continue
        assert_close(p.grad, sd[k].grad, f"1024^2 d{k}")


def test_block_finalize_launch_is_bit_identical(monkeypatch):
    """round 4: the three reductions that end a block's backward (AFNO / channel-MLP split-K partials, GroupNorm parameter
    gradients) run as ONE launch (csrc/gemm_tn.hip block_finalize_kernel, slices of one grid, same summation orders) - every
    gradient must equal the three-launch form bit for bit (DPOT_TUNE fused_small=0, which also un-merges the layout launches)"""
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**R.TINY)
    S = cfg.img_size
    x = R.recipe_input((4, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
    up = (R.recipe_input((4, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()

    def grads(flag):
        set_tune(monkeypatch, fused_small=flag)
        m = DPOTNet(**R.TINY)
        m.load_state_dict(_recipe_sd("TINY", 4))
        m.cuda()
        xg = x.clone().requires_grad_(True)
        y, _ = m(xg)
        (y * up).sum().backward()
        return [xg.grad] + [p.grad for k, p in m.named_parameters() if not k.startswith("cls_head.")]

    for a, b in zip(grads("1"), grads("0")):
        assert torch.equal(a, b)


def test_block_finalize_colsum_slice_bf16_mode(monkeypatch):
    """in the bf16 channel-MLP mode the finalising launch also reduces the bias column sums (df1b, df2b), in a
    different order than the stand-alone colsum kernel - so fused_small=1 / 0 agree to fp32 rounding there, not bit for
    bit (the fp32 model above is bit-identical): every gradient within 1e-6 norm-wise, the two bias gradients included"""
    from dpot_amd import DPOTNet
    cfg = R.DPOTConfig(**R.SMALL)
    S = cfg.img_size
    x = R.recipe_input((4, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
    up = (R.recipe_input((4, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()

    def grads(flag):
        set_tune(monkeypatch, fused_small=flag)
        m = DPOTNet(**R.SMALL)
        m.load_state_dict(_recipe_sd("SMALL", 4))
        m.cuda()
        m.mlp_precision = "bf16"
        xg = x.clone().requires_grad_(True)
        y, _ = m(xg)
        (y * up).sum().backward()
        return {"dx": xg.grad, **{k: p.grad for k, p in m.named_parameters() if not k.startswith("cls_head.")}}

    a, b = grads("1"), grads("0")
    for k in a:
        assert _nrel(a[k], b[k]) <= 1e-6, k
    assert any(k.endswith("mlp.0.bias") for k in a)


def test_gradient_packs_between_blocks_are_bit_identical(monkeypatch):
    """round 5: in the bf16 channel-MLP mode a Block's backward hands its input gradient to the previous Block ALSO as bf16 packs
    + bias column sums, written by the GroupNorm backward kernel that produces it (functional._GRAD_PACKS side table) instead of
    a separate pack pass: every gradient must equal the separate-pass form (DPOT_TUNE packs=0) - bit for bit except the fc2 bias
    gradients, whose column sums are formed per sample instead of per 64 tokens (fp32 rounding) - and the side table must not
    keep more than two entries"""
    from dpot_amd import DPOTNet, functional
    cfg = R.DPOTConfig(**R.SMALL)
    S = cfg.img_size
    x = R.recipe_input((4, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
    up = (R.recipe_input((4, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()
    taken = []
    real = functional._take_grad_packs
    monkeypatch.setattr(functional, "_take_grad_packs", lambda t: (lambda r: (taken.append(r is not None), r)[1])(real(t)))

    def grads(flag):
        set_tune(monkeypatch, packs=flag)
        taken.clear()
        m = DPOTNet(**R.SMALL)
        m.load_state_dict(_recipe_sd("SMALL", 4))
        m.cuda()
        m.mlp_precision = "bf16"
        xg = x.clone().requires_grad_(True)
        y, _ = m(xg)
        (y * up).sum().backward()
        return {"dx": xg.grad, **{k: p.grad for k, p in m.named_parameters() if not k.startswith("cls_head.")}}, list(taken)

    a, ta = grads("1")
    b, tb = grads("0")
    assert sum(ta) == cfg.depth - 1 and sum(tb) == 0, (ta, tb)      # every Block but the last one found its packs
    assert len(functional._GRAD_PACKS) <= 2
    for k in a:
        if k.endswith("mlp.2.bias"):
            assert _nrel(a[k], b[k]) <= 1e-6, k
        else:
            assert torch.equal(a[k], b[k]), k


def test_layout_jobs_launch_is_bit_identical(monkeypatch):
    """round 4: the small weight-only layout pieces (padded conv weights, pos_embed^T + bias, de-embed bias per pixel, padded
    tail weights) come from ONE launch over a device-resident job table (csrc/misc.hip layout_jobs_kernel) instead of eight
    copy / transpose / bias launches: prediction, cls output and every gradient must not change by a bit
    (DPOT_TUNE fused_small=0), for DPOT-Tiny and for the mini config (3 channels, 16-wide tail, 4 time steps)"""
    from dpot_amd import DPOTNet
    for name, kw in (("TINY", R.TINY), ("MINI", R.MINI)):
        cfg = R.DPOTConfig(**kw)
        S = cfg.img_size
        x = R.recipe_input((2, S, S, cfg.in_timesteps, cfg.in_channels), salt=71).cuda()
        up = (R.recipe_input((2, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()

        def run(flag):
            set_tune(monkeypatch, fused_small=flag)
            m = DPOTNet(**kw)
            m.load_state_dict(R.recipe_state_dict(cfg, salt=4))
            m.cuda()
            xg = x.clone().requires_grad_(True)
            y, c = m(xg)
            ((y * up).sum() + c.sum()).backward()
            names = ["y", "cls", "dx"] + [k for k, _ in m.named_parameters()]
            return dict(zip(names, [y.detach(), c.detach(), xg.grad] + [p.grad for p in m.parameters()]))

        a, b = run("1"), run("0")
        for k in a:
            # (round 6: fused_small=0 also takes the cls head off the few-row Linear kernel - a different summation order for
            # the head's output and for every gradient downstream of it: dx, the embed / block gradients through the token
            # mean.  Those agree to fp32 rounding; the prediction - upstream of the head - stays bit-identical)
            if k == "y":
                assert torch.equal(a[k], b[k]), (name, k)
            else:
                assert_close(a[k], b[k].double(), f"{name} {k}", rtol=2e-5, atol_scale=2e-6)


@pytest.fixture
def bf16_mlp():
    from dpot_amd import ops
    ops.set_mlp_precision("bf16")
    yield
    ops.set_mlp_precision(None)


@pytest.mark.parametrize("name,B", [("SMALL", 1), ("MEDIUM", 1), ("TINY", 32)])
def test_bf16_channel_mlp_mode_vs_oracle(name, B, bf16_mlp):
    """BASELINE configs[2] (DPOT-S, bf16 channel-MLP on MFMA) and the DPOT-M / -L headline mode, at their sizes and
    batches, against the fp32 CPU oracle: forward, dx and EVERY parameter gradient within the norm-wise bf16 bound above;
    also asserts that the packed-operand bf16 kernels (csrc/gemm_bf16p.hip) are what ran"""
    from dpot_amd.functional import mlp_pack_kind
    oc = _oracle_case(name, B)
    cfg = oc["cfg"]
    tok = (cfg.img_size // cfg.patch_size) ** 2
    assert mlp_pack_kind(cfg.embed_dim, cfg.mlp_hidden, B * tok) == "bf16", "bf16 panel kernels not selected"
    m, xg, y, c = _hip_case(name, oc)
    e_y, e_c, e_dx = _nrel(y, oc["y"]), _nrel(c, oc["c"]), _nrel(xg.grad, oc["dx"])
    worst, worst_k = 0.0, ""
    for k, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), k
        e = _nrel(p.grad, oc["grads"][k])
        if e > worst:
            worst, worst_k = e, k
    print(f"[{name} B={B} bf16-MLP] norm-wise error: pred {e_y:.2e} cls {e_c:.2e} dx {e_dx:.2e}; worst parameter "
          f"gradient {worst:.2e} ({worst_k})")
    sd = cfg.depth ** 0.5
    assert e_y <= BF16_OUT_TOL and e_c <= BF16_OUT_TOL and e_dx <= BF16_DX_PER_SQRT_DEPTH * sd
    assert worst <= BF16_GRAD_PER_SQRT_DEPTH * sd, worst_k
    # and it IS a reduced-precision mode: not bit-identical to fp32 parity
    assert e_y > 1e-6


@pytest.mark.parametrize("name,B", [("SMALL", 4), ("MEDIUM", 2)])
def test_bf16_channel_mlp_train_step_vs_oracle(name, B, bf16_mlp):
    """one optimiser step (T_ar = 1: rollout, masked relative-L2 loss, backward, clip + Adam) in the bf16 channel-MLP
    mode against the fp32 oracle's step: loss, global gradient norm, and the parameter update"""
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam, train_step
    cfg = R.DPOTConfig(**getattr(R, name))
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=91)
    yy = R.recipe_input((B, S, S, 1, cfg.out_channels), salt=92)
    msk = torch.ones(B, S, S, 1, cfg.out_channels)
    sd0 = _recipe_sd(name, 4)
    m = DPOTNet(**getattr(R, name))
    m.load_state_dict(sd0)
    m.cuda()
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    loss, pred = train_step(m, opt, xx.cuda(), yy.cuda(), msk.cuda())
    st = R.TrainState(params={k: v.clone() for k, v in sd0.items()})
    ref = R.train_step(st, xx, yy, msk, cfg, lr=1e-3)
    e_l = _rel(loss.item(), ref["loss"].item())
    e_g = _rel(opt.grad_norm().item(), ref["grad_norm"].item())
    e_p = _nrel(pred, ref["pred"])
    print(f"[{name} B={B} bf16-MLP train step] loss rel err {e_l:.2e}, |g| rel err {e_g:.2e}, pred {e_p:.2e}")
    assert e_l <= 5e-3 and e_g <= BF16_OUT_TOL and e_p <= BF16_OUT_TOL
    # Adam's first step moves every parameter by ~lr * sign(g): compare the UPDATE direction where |g| is not tiny
    upd_ok, upd_n = 0, 0
    for k, p in m.named_parameters():
        if k.startswith("cls_head"):
            continue
        d_hip = (p.detach().cpu() - sd0[k]).flatten()
        d_ref = (st.params[k].detach() - sd0[k]).flatten()
        big = d_ref.abs() > 0.5e-3
        upd_n += int(big.sum())
        upd_ok += int((torch.sign(d_hip[big]) == torch.sign(d_ref[big])).sum())
    assert upd_ok >= 0.97 * upd_n, f"only {upd_ok}/{upd_n} parameter updates point the oracle's way"


def _oracle_rollout_ckpt(sd, xx, yy, msk, cfg):
    """R.rollout_loss with every AR step under torch.utils.checkpoint: the same arithmetic, one step of activations
    alive at a time (the 20-step DPOT-L rollout would otherwise keep ~100 GB of CPU activations)"""
    from torch.utils.checkpoint import checkpoint
    names = list(sd.keys())

    def fwd(x, *ps):
        return R.dpot_forward(OrderedDict(zip(names, ps)), x, cfg)[0]

    loss, preds = 0.0, []
    for t in range(yy.shape[-2]):
        im = checkpoint(fwd, xx, *sd.values(), use_reentrant=False)
        loss = loss + R.rel_l2_loss(im, yy[..., t:t + 1, :], msk)
        preds.append(im.detach())
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    return loss, torch.cat(preds, dim=-2)


def _gpu_rollout_grads(kw, salt, xx, yy, msk, recompute, keep_last=0):
    import gc
    from dpot_amd.train import FlatParams, FusedAdam, rollout
    gc.collect()                                  # (reference cycles of earlier runs' autograd graphs can hold GiBs of activations)
    torch.cuda.empty_cache()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()          # whatever earlier tests of this process still hold is not this run's peak
    m, _ = build(kw, salt=salt)
    m.recompute_blocks = recompute
    m.recompute_keep_last = keep_last
    fp = FlatParams(m)
    opt = FusedAdam(fp, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    opt.zero_grad()
    loss, pred = rollout(m, xx.cuda(), yy.cuda(), msk.cuda())
    loss.backward()
    torch.cuda.synchronize()
    peak = (torch.cuda.max_memory_allocated() - base) / 2 ** 30
    norms = {k: p.grad.double().norm().item() for k, p in m.named_parameters()}
    return loss.item(), opt.grad_norm().item(), norms, pred.detach(), fp.grad.clone(), peak


def test_large_20_step_rollout_vs_reference_golden():
    """BASELINE configs[4]: DPOT-Large 256^2, modes 64, 20-step auto-regressive rollout (configs/pretrain_large.yaml,
    train_temporal.py:201-230), B=1: loss, global grad norm, per-tensor grad norms and the 20-step prediction against
    golden numbers produced by the imported reference (oracle/make_golden_large.py - the CPU run takes ~10 min, so it
    is a committed fixture); with activation recomputation (BlockFn re-runs its forward in backward) and without -
    the two must agree bit for bit"""
    from helpers import assert_sub, load
    fx = load("g11_large_rollout")
    T_ar, B = int(fx["T_ar"]), int(fx["B"])
    cfg = R.DPOTConfig(**R.LARGE)
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(B, S, S, 1, cfg.out_channels)
    res = {}
    for recompute in (True, False):
        loss, gn, norms, pred, flat, peak = _gpu_rollout_grads(R.LARGE, 6, xx, yy, msk, recompute)
        print(f"[LARGE T_ar={T_ar} B={B}] recompute={recompute}: loss {loss:.6f} (reference {float(fx['loss']):.6f}), "
              f"|g| {gn:.6e} (reference {float(fx['grad_norm']):.6e}), peak memory {peak:.2f} GiB")
        assert _rel(loss, float(fx["loss"])) <= RTOL
        assert _rel(gn, float(fx["grad_norm"])) <= RTOL
        assert_sub(pred, fx, "pred", "20-step prediction")
        for n, want in zip(fx["names"], fx["grad_norms"]):
            assert _rel(norms[str(n)], float(want)) <= RTOL + 1e-7 / (float(want) + 1e-30), str(n)
        res[recompute] = (loss, flat, peak)
        del pred
    assert res[True][0] == res[False][0]
    assert torch.equal(res[True][1], res[False][1]), "recomputation must not change a single bit"
    assert res[True][2] < 0.6 * res[False][2], "recomputation should cut the activation memory"
    # selective recomputation (DPOTNet.recompute_keep_last: the last AR steps keep their activations - what `bench.py --config L20`
    # runs): same bits, memory between the two
    loss, gn, norms, pred, flat, peak = _gpu_rollout_grads(R.LARGE, 6, xx, yy, msk, True, keep_last=7)
    print(f"[LARGE T_ar={T_ar} B={B}] recompute all but the last 7 AR steps: peak memory {peak:.2f} GiB")
    assert loss == res[True][0] and torch.equal(flat, res[True][1])
    assert res[True][2] < peak < res[False][2]


@pytest.mark.parametrize("name,B", REF_GOLDEN_CASES)
def test_vs_reference_golden(name, B):
    """DPOT-S / -M at batch 32 (BASELINE configs[2] / [3]), DPOT-L at batch 4 (`--config L20`) and 16 (`--config L`: B-direct
    bf16 GEMM super-blocks, 128 x 192 tiles, pair-grid rules, panel heights and split-K factors all depend on the batch)
    against golden numbers from the imported REFERENCE model (oracle/make_golden_large_b16.py B micro NAME; up to 50 TFLOP on
    the CPU, hence committed fixtures tests/golden/g13_<name>_b<B>.npz): fp32 path at rtol 1e-4 - prediction / dx subsamples +
    checksums, cls, and for every parameter gradient a strided subsample element-wise plus the float64 norm; then the bf16
    channel-MLP mode (what the bench lines of these configs run) against that verified fp32 result with the norm-wise
    sqrt(depth) bounds of `test_bf16_channel_mlp_mode_vs_oracle`, asserting that the packed-operand bf16 kernels ran"""
    from helpers import assert_sub, load
    from dpot_amd import DPOTNet, ops
    from dpot_amd.functional import mlp_pack_kind
    fx = load(f"g13_{name.lower()}_b{B}")
    assert int(fx["B"]) == B
    kw = getattr(R, name)
    cfg = R.DPOTConfig(**kw)
    S = cfg.img_size
    x = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=71)
    up_y = (R.recipe_input((B, S, S, cfg.out_timesteps, cfg.out_channels), salt=72) * 0.3).cuda()
    up_c = (R.recipe_input((B, cfg.n_cls), salt=73) * 0.3).cuda()

    def run(mlp, gemm=None, info=None):
        torch.cuda.empty_cache()
        ops.set_mlp_precision(mlp)
        try:
            m = DPOTNet(**kw)
            m.gemm_precision = gemm
            m.load_state_dict(_recipe_sd(name, 4))
            m.cuda()
            xg = x.cuda().requires_grad_(True)
            y, c = m(xg)
            ((y * up_y).sum() + (c * up_c).sum()).backward()
            torch.cuda.synchronize()
            if info is not None:
                info["p6"] = getattr(m.packs.get("afno"), "fwd6", None) is not None
        finally:
            ops.set_mlp_precision(None)
        return y.detach(), c.detach(), xg.grad, OrderedDict((k, p.grad) for k, p in m.named_parameters())

    if name in ("SMALL", "MEDIUM") and tune_value("afno_layer", -1) == -1 and tune_value("mixer", 3) == 3:
        # these two cases are the parity gate of the one-launch AFNO layer forward in its `auto` selection (256 workgroups)
        assert ops.afno_fused_supported(16, 16, cfg.embed_dim, cfg.n_blocks, 16, 9, B=B), "one-launch AFNO layer not selected"
    y, c, dx, grads = run(None)
    assert_sub(y, fx, "y", f"{name} B={B} pred")
    assert_close(c, fx["c"], f"{name} B={B} cls")
    assert_sub(dx, fx, "dx", f"{name} B={B} dx")
    want = dict(zip([str(n) for n in fx["names"]], fx["grad_norms"]))
    assert set(want) == set(grads)
    worst = 0.0
    for k, g in grads.items():
        assert_sub(g, fx, f"g/{k}", f"{name} B={B} d{k}")
        e = _rel(g.double().norm().item(), float(want[k]))
        worst = max(worst, e)
        assert e <= RTOL, f"{name} B={B} |d{k}|: {e:.2e}"
    print(f"[{name} B={B} fp32 vs reference golden] worst gradient-norm error {worst:.2e}")

    if name == "LARGE" and tune_value("mixer6", 1) != 0 and tune_value("mixer", 3) != 0:
        # round 6: gemm_precision 'auto' (what bench.py runs DPOT-S / -M / -L with) - the large GEMMs as bf16x6 and, at 96
        # channels per block, the AFNO mixer's MLP on the bf16x6 kernel (csrc/afno_mlp6.hip): fp32-accurate, so it meets the
        # SAME reference golden at the same rtol 1e-4
        info = {}
        ya, ca, dxa, ga = run(None, gemm="auto", info=info)
        assert info["p6"], "bf16x6 mixer packs not built under gemm_precision 'auto'"
        assert_sub(ya, fx, "y", f"{name} B={B} pred (auto)")
        assert_close(ca, fx["c"], f"{name} B={B} cls (auto)")
        assert_sub(dxa, fx, "dx", f"{name} B={B} dx (auto)")
        worst = 0.0
        for k, g in ga.items():
            assert_sub(g, fx, f"g/{k}", f"{name} B={B} d{k} (auto)")
            e = _rel(g.double().norm().item(), float(want[k]))
            worst = max(worst, e)
            assert e <= RTOL, f"{name} B={B} |d{k}| (auto): {e:.2e}"
        print(f"[{name} B={B} gemm_precision auto (bf16x6 GEMMs + bf16x6 mixer) vs reference golden] worst gradient-norm "
              f"error {worst:.2e}")
        del ya, ca, dxa, ga

    tok = (cfg.img_size // cfg.patch_size) ** 2
    ops.set_mlp_precision("bf16")
    try:
        assert mlp_pack_kind(cfg.embed_dim, cfg.mlp_hidden, B * tok) == "bf16", "bf16 panel kernels not selected"
    finally:
        ops.set_mlp_precision(None)
    yb, cb, dxb, gb = run("bf16")
    sd = cfg.depth ** 0.5
    e_y, e_c, e_dx = _nrel(yb, y), _nrel(cb, c), _nrel(dxb, dx)
    worst, worst_k = max((_nrel(gb[k], grads[k]), k) for k in grads)
    print(f"[{name} B={B} bf16-MLP vs the verified fp32 path] pred {e_y:.2e} cls {e_c:.2e} dx {e_dx:.2e}; worst parameter "
          f"gradient {worst:.2e} ({worst_k})")
    assert all(torch.isfinite(g).all() for g in gb.values())
    assert e_y <= BF16_OUT_TOL and e_c <= BF16_OUT_TOL and e_dx <= BF16_DX_PER_SQRT_DEPTH * sd
    assert worst <= BF16_GRAD_PER_SQRT_DEPTH * sd, worst_k
    assert e_y > 1e-6


# bf16 channel-MLP mode over a 20-step rollout (BASELINE configs[4] as bench.py --config L20 runs it: bf16 channel MLP +
# activation recomputation).  Each AR step feeds its prediction back, so the per-step forward error (5-6.5e-3 norm-wise,
# see above) compounds over the window: measured on MI355X against the reference's fp32 golden numbers (g11) - loss
# 7.8e-5, global gradient norm 2.9e-4, worst per-tensor gradient NORM 4.7e-3, 20-step prediction 8.2e-3 (a norm comparison: rounding errors
# that are orthogonal to the gradient do not show in it - the norm-wise gradient ERROR is bounded at one step by the tests above).
BF16_L20_LOSS_TOL = 5e-4
BF16_L20_GNORM_TOL = 2e-3
BF16_L20_TENSOR_NORM_TOL = 2e-2
BF16_L20_PRED_TOL = 3e-2


def test_large_20_step_rollout_bf16_recompute_vs_reference_golden(bf16_mlp):
    """`bench.py --config L20`'s mode - DPOT-L, 20-step rollout, bf16 channel MLP, activation recomputation - against
    the reference's golden numbers (g11: loss, global / per-tensor gradient norms, 20-step prediction) with explicit
    reduced-precision bounds; recomputation must stay bit-identical to the stored-activation run in this mode too"""
    from helpers import load
    fx = load("g11_large_rollout")
    T_ar, B = int(fx["T_ar"]), int(fx["B"])
    cfg = R.DPOTConfig(**R.LARGE)
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(B, S, S, 1, cfg.out_channels)
    res = {}
    for recompute in (True, False):
        loss, gn, norms, pred, flat, peak = _gpu_rollout_grads(R.LARGE, 6, xx, yy, msk, recompute)
        e_l, e_g = _rel(loss, float(fx["loss"])), _rel(gn, float(fx["grad_norm"]))
        stride = int(fx["pred.stride"])
        ps = pred.cpu().reshape(-1)[::stride].double()
        pr = torch.as_tensor(fx["pred.sub"]).double()
        e_p = ((ps - pr).norm() / pr.norm()).item()
        worst, worst_k = max((_rel(norms[str(n)], float(w)), str(n)) for n, w in zip(fx["names"], fx["grad_norms"]))
        print(f"[LARGE T_ar={T_ar} B={B} bf16-MLP] recompute={recompute}: loss err {e_l:.2e}, |g| err {e_g:.2e}, "
              f"20-step prediction (subsample, norm-wise) {e_p:.2e}, worst per-tensor gradient norm {worst:.2e} ({worst_k}), "
              f"peak memory {peak:.2f} GiB")
        assert e_l <= BF16_L20_LOSS_TOL and e_g <= BF16_L20_GNORM_TOL and worst <= BF16_L20_TENSOR_NORM_TOL
        assert e_p <= BF16_L20_PRED_TOL and e_p > 1e-6
        res[recompute] = (loss, flat, peak)
        del pred
    assert res[True][0] == res[False][0]
    assert torch.equal(res[True][1], res[False][1]), "recomputation must not change a single bit (bf16 mode)"
    assert res[True][2] < 0.6 * res[False][2]


def test_tiny_5_step_rollout_vs_oracle():
    """T_ar=5 DPOT-Tiny rollout (B=2) against the CPU oracle run live: loss, grad norms, prediction; +- recomputation"""
    kw, T_ar, B = R.TINY, 5, 2
    cfg = R.DPOTConfig(**kw)
    S = cfg.img_size
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81)
    yy = R.recipe_input((B, S, S, T_ar, cfg.out_channels), salt=82)
    msk = torch.ones(B, S, S, 1, cfg.out_channels)
    sd = OrderedDict((k, v.clone().requires_grad_(True)) for k, v in R.recipe_state_dict(cfg, salt=6).items())
    loss_ref, pred_ref = _oracle_rollout_ckpt(sd, xx, yy, msk, cfg)
    loss_ref.backward()
    ref_norms = {k: v.grad.double().norm().item() for k, v in sd.items() if v.grad is not None}
    ref_total = sum(v ** 2 for v in ref_norms.values()) ** 0.5
    res = {}
    for recompute in (True, False):
        loss, gn, norms, pred, flat, peak = _gpu_rollout_grads(kw, 6, xx, yy, msk, recompute)
        print(f"[TINY T_ar={T_ar} B={B}] recompute={recompute}: loss {loss:.6f} (oracle {loss_ref.item():.6f}), "
              f"|g| {gn:.6e} (oracle {ref_total:.6e}), peak memory {peak:.2f} GiB")
        assert _rel(loss, loss_ref.item()) <= RTOL
        assert _rel(gn, ref_total) <= RTOL
        assert_close(pred, pred_ref, "rollout pred")
        for k, want in ref_norms.items():
            assert _rel(norms[k], want) <= RTOL + 1e-7 / (want + 1e-30), k
        res[recompute] = (loss, flat, peak)
    assert res[True][0] == res[False][0] and torch.equal(res[True][1], res[False][1])
    assert res[True][2] < res[False][2]


def test_recompute_with_noise_and_graph_capture():
    """recomputation inside a captured T_ar=3 step with in-kernel noise: replays are reproducible and the step trains"""
    from dpot_amd.train import FlatParams, FusedAdam, GraphedTrainStep
    m, cfg = build(R.MINI, salt=2)
    m.recompute_blocks = True
    S = cfg.img_size
    xx = R.recipe_input((2, S, S, cfg.in_timesteps, cfg.in_channels), salt=3).cuda()
    yy = R.recipe_input((2, S, S, 3, cfg.out_channels), salt=4).cuda()
    msk = torch.ones(2, S, S, 1, cfg.out_channels, device="cuda")
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=1e4)
    g = GraphedTrainStep(m, opt, xx, yy, msk, noise_scale=0.01, warmup=1)
    losses = [g.replay(1e-3).item() for _ in range(6)]
    assert all(torch.isfinite(torch.tensor(losses)))
    assert losses[-1] < losses[0]
