#!/usr/bin/env python
"""Bit-level fingerprint of the models' training step (DPOTNet, DPOTNet3D, CDPOTNet, FNO2d, FNO3d), of the block path
(functional.BlockFn / AFNO2DFn / AFNO3DFn / block3d) and of the FNO mixing operators, for comparing two trees that must compute
the same thing:
python scripts/grad_fingerprint.py > a.txt   in each tree, on the same machine with the same built library (DPOT_HIP_LIB),
then `diff`.  Run it a second time under DPOT_TUNE=gn_fuse=0,panel=0 (the C library reads those two keys once per process);
the Python-side DPOT_TUNE keys are set per case here.

One line per case: name, the loss (or sum of the output) as hex, SHA-256 over the bytes of every gradient - and of the flat
parameter buffer after one FusedAdam step where the case is a model -, and the launch counts that show which route ran.  A
case asserts its route where the code offers a way to see it.  Inputs and weights: the recipes of oracle/dpot_ref.py,
tests/afno3d_ref.py and tests/cdpot_ref.py, as the tests use them."""
import hashlib
import itertools
import math
import os
import sys
from collections import OrderedDict

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import afno3d_ref as A3  # noqa: E402
import cdpot_ref as CR  # noqa: E402
import dft_cases as DC  # noqa: E402
import eval3d_ref as E3  # noqa: E402
import eval_ref as E2  # noqa: E402
import fno3d_ref as F3  # noqa: E402
import fno3d_time  # noqa: E402  (scripts/: the shapes it times)
import fno_ref as FR  # noqa: E402
import fno_time  # noqa: E402  (scripts/)
from dpot_amd import CDPOTNet, DPOTNet, DPOTNet3D, FNO2d, FNO3d, RolloutEvaluator, _lib, load_3d_components_from_2d, ops  # noqa: E402
from dpot_amd.functional import AFNO2DFn, AFNO3DFn, block3d  # noqa: E402
from dpot_amd.train import FlatParams, FusedAdam, rollout, rollout_total, train_step  # noqa: E402
from oracle import dpot_ref as R  # noqa: E402
from resize_ref import hash_field  # noqa: E402

BASE_TUNE = os.environ.get("DPOT_TUNE", "")
COUNTED = ("block_finalize", "wgrad_batch_finalize", "groupnorm_param_grads", "afno_fused_fwd", "afno_mlp2", "gn_rfft2",
           "bf16_pack_both", "groupnorm_bwd_packs", "afno_wgrad2", "mlp_wgrad2", "linear_fwd", "linear_bwd_data", "linear_bwd_wb",
           "patchify", "patchify3", "unpatchify", "unpatchify3", "fold3", "group_rowsum", "token_mean", "token_mean_bwd", "colsum",
           "gemm")


def set_tune(**kv):
    cur = dict(x.split("=") for x in BASE_TUNE.split(",") if x)
    cur.update({k: str(v) for k, v in kv.items()})
    os.environ["DPOT_TUNE"] = ",".join(f"{k}={v}" for k, v in cur.items())


class Counts(dict):
    """calls of the COUNTED ops entry points (looked up on the module at call time, as the library's callers do), and the
    layouts afno_mlp2 was called with"""

    def __enter__(self):
        self.real, self.layouts = {n: getattr(ops, n) for n in COUNTED}, []
        for n, f in self.real.items():
            self[n] = 0
            setattr(ops, n, self._wrap(n, f))
        return self

    def _wrap(self, n, f):
        def g(*a, **k):
            self[n] += 1
            if n == "afno_mlp2":
                self.layouts.append(k.get("layout", 0))
            return f(*a, **k)
        return g

    def __exit__(self, *exc):
        for n, f in self.real.items():
            setattr(ops, n, f)

    def __str__(self):
        return " ".join(f"{n}={v}" for n, v in self.items() if v) + f" layouts={sorted(set(self.layouts))}"


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def report(name, value, tensors, c):
    torch.cuda.synchronize()
    print(f"{name}: {float(value.detach()).hex()} {digest(tensors)} {c}", flush=True)


def model_case(name, kw, B, T_ar, salt=6, tune=None, check=None, model=DPOTNet, cls_weight=0.0, **attrs):
    """one rollout + backward on flat-bound parameters (cls_weight: with the classification output in the loss), one FusedAdam step"""
    set_tune(**(tune or {}))
    hook = attrs.pop("hook", False)
    cfg = R.DPOTConfig(**kw)
    m = model(**kw)
    if model is DPOTNet:
        m.load_state_dict(R.recipe_state_dict(cfg, salt=salt))
    else:
        m.load_state_dict(CR.recipe_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, kw, salt))
    m.cuda()
    for k, v in attrs.items():
        setattr(m, k, v)
    if hook:
        m._boundary_hook = lambda b, lat: lat
    S, Tb = cfg.img_size, cfg.out_timesteps
    xx = R.recipe_input((B, S, S, cfg.in_timesteps, cfg.in_channels), salt=81).cuda()
    yy = R.recipe_input((B, S, S, T_ar * Tb, cfg.out_channels), salt=82).cuda()
    msk = torch.ones(B, S, S, 1, cfg.out_channels, device="cuda")
    opt = FusedAdam(FlatParams(m), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
    opt.zero_grad()
    with Counts() as c:
        if cls_weight:
            labels = torch.arange(B, device="cuda") % cfg.n_cls
            loss = rollout_total(m, xx, yy, msk, Tb, cls=labels, cls_weight=cls_weight)[2]
        else:
            loss, _ = rollout(m, xx, yy, msk, Tb)
        loss.backward()
    torch.cuda.synchronize()
    left = [k for k, p in zip(opt.fp.names, opt.fp.pending) if p != 0 and (cls_weight or not k.startswith("cls_head."))]
    assert not left, f"{name}: gradient sinks never delivered: {left}"
    grads = [p.grad.clone() for _, p in m.named_parameters() if p.grad is not None]
    opt.step()
    if check is not None:
        check(c, cfg, T_ar)
    report(name, loss, grads + [opt.fp.flat], c)


def lib_batches():
    lib = _lib.load()
    return lib.dpot_tune(b"wgrad_gauss", 1) != 0 and lib.dpot_tune(b"panel", 1) != 0


def expect_finalize(batch, per_block):
    def check(c, cfg, T_ar):
        want = {"wgrad_batch_finalize": T_ar * batch, "block_finalize": T_ar * cfg.depth * per_block}
        if not lib_batches():       # the fused weight-gradient launches may be off altogether: nothing left to finalise per block
            want.pop("block_finalize")
        assert {k: c[k] for k in want} == want, (want, dict(c))
    return check


def wgrad_cases():
    kw = dict(R.TINY, embed_dim=256, n_blocks=2, depth=3)          # 128 channels per block, 16 x 16 grid, Mm = 288
    for fs in (0, 1, 2, 3):
        batched = fs in (1, 3) and lib_batches()
        model_case(f"wgrad fused_small={fs}", kw, 2, 2, tune=dict(fused_small=fs),
                   check=expect_finalize(int(batched), int(fs != 0 and not batched)))
    model_case("wgrad fused_small=1 recompute", kw, 2, 2, tune=dict(fused_small=1), check=expect_finalize(0, 1),
               recompute_blocks=True)
    model_case("wgrad fused_small=1 hook", kw, 2, 2, tune=dict(fused_small=1), check=expect_finalize(0, 1), hook=True)


def bf16_cases():
    def check_for(pack_both):
        def check(c, cfg, T_ar):
            M = 4 * (cfg.img_size // cfg.patch_size) ** 2
            if pack_both and ops.bf16_pack_both_supported(M, cfg.embed_dim):
                assert c["bf16_pack_both"] > 0, dict(c)
            if not pack_both:
                assert c["bf16_pack_both"] == 0 and c["groupnorm_bwd_packs"] == 0, dict(c)
        return check
    for tag, tune in (("", {}), (" packs=0", dict(packs=0)), (" pack_both=0", dict(pack_both=0))):
        model_case("bf16 small afno_layer=1" + tag, R.SMALL, 4, 1, salt=3, tune=dict(afno_layer=1, **tune),
                   check=check_for("pack_both" not in tune), mlp_precision="bf16")
    model_case("bf16 small", R.SMALL, 4, 1, salt=3, check=check_for(True), mlp_precision="bf16")


def mixer6_cases():
    def check(c, cfg, T_ar):
        if ops.afno_mlp6_supported(cfg.n_blocks, cfg.embed_dim // cfg.n_blocks):
            assert c.layouts and all(l == 2 for l in c.layouts), c.layouts
    for bs in (96, 128):
        kw = dict(R.MINI, img_size=256, patch_size=8, embed_dim=2 * bs, out_layer_dim=32, depth=2, mlp_ratio=1, n_blocks=2, modes=32)
        for rec in (False, True):
            model_case(f"mixer6 bs={bs} recompute={int(rec)}", kw, 2, 1, salt=4, tune=dict(mixer6=2), check=check,
                       gemm_precision="auto", recompute_blocks=rec)


def generic_case():
    def check(c, cfg, T_ar):
        assert c["afno_mlp2"] == 0 and c["gn_rfft2"] == 0 and c["afno_fused_fwd"] == 0 and c["afno_wgrad2"] == 0, dict(c)
    model_case("generic mini", R.MINI, 2, 1, salt=3, check=check)
    # linear_fwd on the generic GEMM route instead of small_linear (which takes K % 512 == 0: the cls_head at 512 channels)
    model_case("generic mini fused_small=0", R.MINI, 2, 1, salt=3, tune=dict(fused_small=0))
    for fs in (0, 1):
        model_case(f"mini E512 cls fused_small={fs}", dict(R.MINI, embed_dim=512), 2, 1, salt=3, tune=dict(fused_small=fs),
                   cls_weight=0.5)


def plain_stage_cases():
    """the stages built from chains of dense layers: normalize=True, HeadFn's unfused tail (ops.out_tail_supported needs
    out_layer_dim 32) with and without the classification output in the loss, and both CDPOTNet mini models"""
    model_case("mini normalize", dict(R.MINI, normalize=True), 2, 2, salt=3)
    kw = dict(R.MINI, out_layer_dim=16)
    assert not ops.out_tail_supported(16, kw["out_channels"], 2 * kw["img_size"] ** 2)
    model_case("mini unfused tail", kw, 2, 2, salt=3)
    model_case("mini unfused tail cls", kw, 2, 2, salt=3, cls_weight=0.5)
    for tag, kw in (("mini1", CR.MINI1), ("mini2 normalize", CR.MINI2)):
        model_case("cdpot " + tag, kw, CR.MODEL_B, 2, salt=CR.STEP["salt"], model=CDPOTNet, cls_weight=0.5)


def afno2d_case(name, one_launch):
    """AFNO2DFn alone at the shape of the golden g1_afno_tiny: B 2, 16 x 16 grid, E 512, 4 blocks, all modes"""
    set_tune(**(dict(afno_layer=1) if one_launch else {}))
    B, h, E, nb, modes = 2, 16, 512, 4, 32
    cfg = R.DPOTConfig(img_size=h * 8, patch_size=8, embed_dim=E, n_blocks=nb, modes=modes, depth=1)
    pre = "blocks.0.filter."
    sd = {k[len(pre):]: v.cuda().requires_grad_(True) for k, v in R.recipe_state_dict(cfg, salt=3).items() if k.startswith(pre)}
    x = R.recipe_input((B, h, h, E), salt=11).cuda().view(B, h * h, E).requires_grad_(True)
    up = (R.recipe_input((B, h, h, E), salt=12) * 0.3).cuda().view(B, h * h, E)
    with Counts() as c:
        y = AFNO2DFn.apply(x, sd["w1"], sd["b1"], sd["w2"], sd["b2"], h, h, nb, modes, 1)
        (y * up).sum().backward()
    if one_launch and ops.afno_mlp3_supported(nb, E // nb) and ops.afno_fused_supported(h, h, E, nb, 16, 9, G=0):
        assert c["afno_fused_fwd"] == 1, dict(c)
    if not one_launch:
        assert c["afno_fused_fwd"] == 0, dict(c)
    assert c["block_finalize"] == 0 and c["wgrad_batch_finalize"] == 0, dict(c)
    report(name, y.sum(), [y, x.grad] + [sd[k].grad for k in ("w1", "b1", "w2", "b2")], c)


def cases_3d():
    set_tune()
    act = ops.ACT_IDS["gelu"]
    for i, (name, (Bc, dims, E, nb, modes)) in enumerate(A3.AFNO_CASES.items()):
        x = R.recipe_input((Bc, *dims, E), 171 + i).reshape(Bc, -1, E).cuda().requires_grad_(True)
        g = R.recipe_input((Bc, *dims, E), 221 + i).reshape(Bc, -1, E).cuda()
        ws = [w.cuda().requires_grad_(True) for w in A3.afno_recipe(E, nb, 171 + i)]
        with Counts() as c:
            y = AFNO3DFn.apply(x, *ws, dims, nb, modes, act)
            y.backward(g)
        assert c["block_finalize"] == 0 and c["wgrad_batch_finalize"] == 0, dict(c)
        report(f"afno3d {name}", y.sum(), [y, x.grad] + [w.grad for w in ws], c)
    bc = A3.BLOCK_CASE
    E, nb, mh = bc["E"], bc["nb"], int(bc["E"] * bc["mlp_ratio"])
    p = {k: v.cuda().requires_grad_(True) for k, v in A3.block_recipe(E, nb, mh, 175).items()}
    x = R.recipe_input((bc["B"], *bc["dims"], E), 175).reshape(bc["B"], -1, E).cuda().requires_grad_(True)
    g = R.recipe_input((bc["B"], *bc["dims"], E), 225).reshape(bc["B"], -1, E).cuda()
    with Counts() as c:
        y = block3d(x, p["norm1.weight"], p["norm1.bias"], p["filter.w1"], p["filter.b1"], p["filter.w2"], p["filter.b2"],
                    p["norm2.weight"], p["norm2.bias"], p["mlp.0.weight"], p["mlp.0.bias"], p["mlp.2.weight"], p["mlp.2.bias"],
                    bc["dims"], nb, bc["modes"], act)
        y.backward(g)
    report("block3d", y.sum(), [y, x.grad] + [v.grad for v in p.values()], c)
    step3d("dpot3d mini fine-tune step", A3.MINI3D, True)
    step3d("dpot3d mini normalize step", A3.MINI3D_NORM, False)


def step3d(name, cfg, from_2d):
    """one step of a mini DPOTNet3D (from_2d: with a 2-D model's blocks and time aggregator loaded): two AR steps, clip, fused Adam"""
    st, B = A3.STEP, 2
    m = DPOTNet3D(**cfg)
    m.load_state_dict(A3.recipe_sd({k: tuple(v.shape) for k, v in m.state_dict().items()}, cfg["n_blocks"], 182))
    m.cuda()
    if from_2d:
        load_3d_components_from_2d(m, R.recipe_state_dict(R.DPOTConfig(**A3.MINI2D), 183), ["blocks", "time_agg"])
    S, T, C = cfg["img_size"], cfg["in_timesteps"], cfg["in_channels"]
    xx = R.recipe_input((B, S, S, S, T, C), 182).cuda()
    yy = R.recipe_input((B, S, S, S, st["T_ar"], C), 183).cuda()
    msk = A3.recipe_mask((B, S, S, S, 1, C), 182).cuda()
    opt = FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"])
    opt.zero_grad()
    with Counts() as c:
        loss, _ = rollout(m, xx, yy, msk)
        loss.backward()
    grads = [p.grad.clone() for p in m.parameters() if p.grad is not None]
    opt.step()
    report(name, loss, grads + [opt.fp.flat], c)


def fno_case():
    """the recorded two-AR-step training step of tests/test_gpu_fno.py (csrc/fno.hip)"""
    set_tune()
    st = FR.STEP
    m = FNO2d(**FR.MINI1)
    m.load_state_dict(FR.recipe_sd(OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items()), st["salt"]), strict=True)
    m.cuda()
    xx, yy, msk = (t.cuda() for t in FR.step_inputs())
    opt = FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"])
    with Counts() as c:
        loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"])
    report("fno2d mini step", loss, [pred] + [p.grad for p in m.parameters() if p.grad is not None] + [opt.fp.flat], c)


def fno3d_case():
    """the recorded two-AR-step training step of tests/test_gpu_fno3d.py (csrc/fno3.hip)"""
    set_tune()
    st = F3.STEP
    m = FNO3d(**F3.MINI1)
    m.load_state_dict(F3.recipe_sd(OrderedDict((k, (tuple(v.shape), v.dtype)) for k, v in m.state_dict().items()), st["salt"]),
                      strict=True)
    m.cuda()
    xx, yy, msk = (t.cuda() for t in F3.step_inputs())
    opt = FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"])
    with Counts() as c:
        loss, pred = train_step(m, opt, xx, yy, msk, lr=st["lr"])
    report("fno3d mini step", loss, [pred] + [p.grad for p in m.parameters() if p.grad is not None] + [opt.fp.flat], c)


def device_hash(shape, salt):
    """fp32 in [-0.5, 0.5) from exact int64 arithmetic on the element index, drawn on the device: the weights of the timed 3-D
    shape are gigabytes"""
    i = torch.arange(math.prod(shape), device="cuda", dtype=torch.int64)
    return (((i * 2654435761 + salt * 40503) % 65521).float() / 65521.0 - 0.5).view(shape)


def mix_cases():
    """ops.fno_mix / fno3_mix (forward and adjoint) and ops.fno_mix_wgrad / fno3_mix_wgrad (plain, and accumulate=True onto a
    hashed base) over every mixing case of the GPU tests and at the four shapes scripts/fno_time.py and scripts/fno3d_time.py
    time; every weight and every base its own salt"""
    set_tune()
    timed2 = [(B, C, C, m1, m2) for _, B, _, _, C, m1, m2 in fno_time.SHAPES]
    timed3 = [(B, C, C, m, m, m) for _, B, _, C, m in fno3d_time.SHAPES]
    with Counts() as c:
        for cases, planar in ((list(FR.MIX_CASES) + timed2, True), (list(F3.MIX_CASES) + timed3, False)):
            for B, Cin, Cout, *modes in cases:
                kept = tuple(2 * m for m in modes[:-1]) + (modes[-1],)
                wshape = (2, Cin, Cout, *modes) if planar else (Cin, Cout, *modes, 2)
                X, dO = device_hash((B, *kept, 2, Cin), 41), device_hash((B, *kept, 2, Cout), 42)
                ws = [device_hash(wshape, 43 + k) for k in range(2 if planar else 4)]
                if planar:
                    op, fwd, adj = "fno_mix", ops.fno_mix(X, *ws), ops.fno_mix(dO, *ws, adjoint=True)
                    ds = ops.fno_mix_wgrad(X, dO)
                    acc = ops.fno_mix_wgrad(X, dO, *(device_hash(wshape, 47 + k) for k in range(2)), accumulate=True)
                else:
                    op, fwd, adj = "fno3_mix", ops.fno3_mix(X, ws), ops.fno3_mix(dO, ws, adjoint=True)
                    ds = ops.fno3_mix_wgrad(X, dO)
                    acc = ops.fno3_mix_wgrad(X, dO, [device_hash(wshape, 47 + k) for k in range(4)], accumulate=True)
                tag = f"B{B} {Cin}->{Cout} modes {'x'.join(map(str, modes))}"
                report(f"{op} {tag}", fwd.sum(), [fwd], c)
                report(f"{op} adjoint {tag}", adj.sum(), [adj], c)
                report(f"{op}_wgrad {tag}", ds[0].sum(), ds, c)
                report(f"{op}_wgrad accumulate {tag}", acc[0].sum(), acc, c)
                del X, dO, ws, fwd, adj, ds, acc


def operator_cases():
    """the spectral operators no model case reaches, each at the smallest shapes its GPU test uses: the Fourier resize (one even
    and one odd size pair, scalar and 16-byte loads), the rollout evaluator in 2-D and 3-D, rfft2 / irfft2 once per compiled
    kernel kind (the smallest case tests/dft_cases.py has for it) and at a 20 x 20 grid of the generic kernels, rfft3 / irfft3"""
    set_tune()
    with Counts() as c:
        for (nx, ny, mx, my), TC in itertools.product([(16, 16, 9, 9), (10, 10, 16, 16)], (1, 4)):
            x = torch.from_numpy(hash_field((1, nx, ny, TC), 8 + TC)).cuda()
            y = ops.spectral_resize(x, (mx, my))
            report(f"spectral_resize {nx}x{ny}->{mx}x{my} TC={TC}", y.sum(), [y], c)
        for shape, ilow, ihigh in (((1, 16, 16, 1, 1), 2, 5), ((1, 16, 16, 10, 4), 2, 5), ((1, 6, 5, 7, 1, 1), 1, 2),
                                   ((1, 6, 5, 7, 10, 4), 1, 2)):
            p, t = E3.independent_pair(shape, 5) if len(shape) == 6 else E2.hashed_pair(shape, 5, hash_field)
            ev = RolloutEvaluator("cuda", n_channels=shape[-1], T_max=12, ilow=ilow, ihigh=ihigh)
            ev.update(torch.from_numpy(p).cuda(), torch.from_numpy(t).cuda())
            report(f"evaluator {'x'.join(map(str, shape))}", ev.acc[0], [ev.acc], c)
        for inverse in (False, True):
            cases = [min((d for d in DC.RUNNABLE if (d.kind_inv if inverse else d.kind_fwd) == k), key=lambda d: d.B * d.h * d.w * d.E)
                     for k in ops.dft2_kernel_kinds(inverse)] + [DC.Case(2, 20, 20, 24, 3, 20, 11, 0, 0)]
            for d in cases:
                kind = ops.dft2_kernel_kind(d.B, d.h, d.w, d.E, d.nb, d.mx, d.my, inverse)
                assert kind == (d.kind_inv if inverse else d.kind_fwd), (d, kind)
                x = R.recipe_input((d.B, d.h * d.w, d.E), 31).cuda()
                if inverse:
                    spec = R.recipe_input((d.B * d.mx * d.my, 2 * d.E), 32).cuda()
                    out = ops.irfft2(spec, d.B, d.h, d.w, d.E, d.nb, d.mx, d.my, 1, res=x)
                else:
                    out = ops.rfft2(x, d.h, d.w, d.nb, d.mx, d.my, 1)
                report(f"{'irfft2' if inverse else 'rfft2'} kind={kind} {DC.case_id(d)}", out.sum(), [out], c)
        B, dims, E, nb, m3 = 2, (5, 3, 7), 16, 1, (2, 2, 4)
        x = R.recipe_input((B, dims[0] * dims[1] * dims[2], E), 33).cuda()
        spec = ops.rfft3(x, dims, nb, m3, 1)
        report("rfft3 5x3x7", spec.sum(), [spec], c)
        y = ops.irfft3(R.recipe_input(tuple(spec.shape), 34).cuda(), B, dims, E, nb, m3, 1, res=x)
        report("irfft3 5x3x7", y.sum(), [y], c)


def main():
    if not torch.cuda.is_available():
        raise SystemExit("grad_fingerprint: needs the GPU")
    print(f"# DPOT_TUNE={BASE_TUNE!r}", flush=True)
    fno_case()
    fno3d_case()
    mix_cases()
    operator_cases()
    wgrad_cases()
    bf16_cases()
    mixer6_cases()
    afno2d_case("afno2d one-launch layer", True)
    generic_case()
    plain_stage_cases()
    afno2d_case("afno2d g1_afno_tiny", False)
    cases_3d()


if __name__ == "__main__":
    main()
