"""GPU tests of the 3-D fine-tuning path: the transforms of csrc/dft3.hip (ops.rfft3 / ops.irfft3) against their float64
definitions, functional.AFNO3DFn / block3d and DPOTNet3D against the reference's records (g17_dpot3d) and the float64
restatement tests/afno3d_ref.py, one fine-tune step after load_3d_components_from_2d, graph capture, the unsupported grid.
Everything runs on the guarded, poisoned allocator (tests/guard.py) at the default fp32 precision, B = 2 throughout."""
import functools
from collections import OrderedDict

import numpy as np
import pytest
import torch

import afno3d_ref as A3
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import assert_close, assert_sub, load
from oracle import dpot_ref as R

pytestmark = pytest.mark.gpu

B = 2
# (X, Y, Z), E, nb, kept (mx, my, mz) and what each shape exercises
SHAPES = [((4, 4, 4), 32, 4, (4, 4, 3)),        # channel blocks of 8 inside a wider slab: blk, ci per channel
          ((6, 5, 4), 64, 2, (3, 3, 3)),        # non-cubic, odd y, truncation in x and y
          ((5, 3, 7), 16, 1, (2, 2, 4)),        # all odd: no Nyquist bin, weight 2 on the last kept bin
          ((4, 3, 16), 32, 1, (2, 2, 8)),       # z truncation active: the Nyquist bin is dropped
          ((8, 8, 8), 96, 3, (8, 8, 5)),        # the design cube, E / CC not a power of two
          ((16, 16, 16), 32, 4, (5, 5, 8))]     # the largest supported cube: the LDS-limit path, narrowest slab
IDS = ["x".join(map(str, s[0])) for s in SHAPES]


@functools.lru_cache(maxsize=None)
def transform_case(i):
    """inputs and float64 expectations of SHAPES[i], computed once and shared (never modified)"""
    dims, E, nb, m3 = SHAPES[i]
    x = R.recipe_input((B, *dims, E), 300 + i)
    res = R.recipe_input((B, *dims, E), 320 + i)
    gen = torch.Generator().manual_seed(1700 + i)
    S = torch.complex(torch.randn(B, *m3, E, generator=gen, dtype=torch.float64),
                      torch.randn(B, *m3, E, generator=gen, dtype=torch.float64))      # not Hermitian
    fwd = {cw: A3.to_rows(A3.rfft3_def(x, m3, cw), nb) for cw in (0, 1)}
    inv = {cw: A3.irfft3_def(S, dims, cw) for cw in (0, 1)}
    return dict(x=x, res=res, S=S, rows=A3.to_rows(S, nb).float(), fwd=fwd, inv=inv, irfftn=A3.irfftn_padded(S, dims))


@pytest.mark.parametrize("cw", [0, 1])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_rfft3_vs_float64_definition(i, cw, guarded):
    from dpot_amd import ops
    dims, E, nb, m3 = SHAPES[i]
    c = transform_case(i)
    assert ops.dft3_supported(dims, E, m3)
    x = guard.wrap(c["x"].reshape(B, -1, E), "cuda")
    got = ops.rfft3(x, dims, nb, m3, cw)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B * m3[0] * m3[1] * m3[2], 2 * E)
    assert_close(got, c["fwd"][cw], f"rfft3 {dims} cw={cw}")


@pytest.mark.parametrize("with_res", [False, True], ids=["nores", "res"])
@pytest.mark.parametrize("cw", [0, 1])
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_irfft3_vs_float64_definition(i, cw, with_res, guarded):
    from dpot_amd import ops
    dims, E, nb, m3 = SHAPES[i]
    c = transform_case(i)
    rows = guard.wrap(c["rows"], "cuda")
    res = guard.wrap(c["res"].reshape(B, -1, E), "cuda") if with_res else None
    got = ops.irfft3(rows, B, dims, E, nb, m3, cw, res=res)
    torch.cuda.synchronize()
    want = c["inv"][cw] + (c["res"].double() if with_res else 0.0)
    assert_close(got.view(B, *dims, E), want, f"irfft3 {dims} cw={cw} res={with_res}")
    if cw == 1 and not with_res:       # ... which is torch.fft.irfftn of the zero-padded, non-Hermitian box
        assert_close(got.view(B, *dims, E), c["irfftn"], f"irfft3 {dims} vs irfftn")


# ---- AFNO3DFn ------------------------------------------------------------------------------------------------------------
def _cmp(t, fx, key, what):
    if key + ".sub" in fx.files:
        assert_sub(t, fx, key, what)
    else:
        assert_close(t, fx[key], what)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return (a - b).abs().max().item() / (b.abs().max().item() + 1e-300)


@pytest.mark.parametrize("name", list(A3.AFNO_CASES))
def test_afno3d_fn_vs_reference_and_float64(name, guarded):
    """A: generic-GEMM mixer (Mm = 96); B: fused afno_mlp2 path, N = 64, ragged row tile (Mm = 54); C: mz = 8 truncates"""
    from dpot_amd import ops
    from dpot_amd.functional import AFNO3DFn
    fx = load("g17_dpot3d")
    Bc, dims, E, nb, modes = A3.AFNO_CASES[name]
    salt = 171 + list(A3.AFNO_CASES).index(name)
    x0, g0 = R.recipe_input((Bc, *dims, E), salt), R.recipe_input((Bc, *dims, E), salt + 50)
    ws0 = A3.afno_recipe(E, nb, salt)
    x = guard.wrap(x0.reshape(Bc, -1, E), "cuda").requires_grad_(True)
    ws = [guard.wrap(w, "cuda").requires_grad_(True) for w in ws0]
    y = AFNO3DFn.apply(x, *ws, dims, nb, modes, ops.ACT_IDS["gelu"])
    y.backward(guard.wrap(g0.reshape(Bc, -1, E), "cuda"))
    torch.cuda.synchronize()
    got = [y.view(Bc, *dims, E), x.grad.view(Bc, *dims, E)] + [w.grad for w in ws]
    # float64 restatement on the same input
    x64 = x0.double().requires_grad_(True)
    w64 = [w.double().requires_grad_(True) for w in ws0]
    y64 = A3.afno3d_ref(x64, *w64, nb, modes)
    (y64 * g0.double()).sum().backward()
    ref64 = [y64, x64.grad] + [w.grad for w in w64]
    for k, t, r in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), got, ref64):
        print(f"afno3d.{name}.{k}: kernels {_rel(t, r):.2e}  reference-fp32 {float(fx[f'afno3d.{name}.err32.{k}']):.2e} "
              "(max|d| / max|float64|)")
    for k, t, r in zip(("y", "dx", "dw1", "db1", "dw2", "db2"), got, ref64):
        _cmp(t, fx, f"afno3d.{name}.{k}", f"afno3d.{name}.{k} vs reference")
        assert_close(t, r, f"afno3d.{name}.{k} vs float64")


# ---- Block3D -------------------------------------------------------------------------------------------------------------
def _run_block(p0, x0, g0, nb, modes, act):
    from dpot_amd import ops
    from dpot_amd.functional import block3d
    Bc, E = x0.shape[0], x0.shape[-1]
    dims = tuple(x0.shape[1:4])
    x = guard.wrap(x0.reshape(Bc, -1, E), "cuda").requires_grad_(True)
    p = OrderedDict((k, guard.wrap(v, "cuda").requires_grad_(True)) for k, v in p0.items())
    y = block3d(x, p["norm1.weight"], p["norm1.bias"], p["filter.w1"], p["filter.b1"], p["filter.w2"], p["filter.b2"],
                p["norm2.weight"], p["norm2.bias"], p["mlp.0.weight"], p["mlp.0.bias"], p["mlp.2.weight"], p["mlp.2.bias"],
                dims, nb, modes, ops.ACT_IDS[act])
    y.backward(guard.wrap(g0.reshape(Bc, -1, E), "cuda"))
    torch.cuda.synchronize()
    return y.view(Bc, *dims, E), x.grad.view(Bc, *dims, E), OrderedDict((k, v.grad) for k, v in p.items())


def _block_inputs():
    c = A3.BLOCK_CASE
    E, nb, mh = c["E"], c["nb"], int(c["E"] * c["mlp_ratio"])
    return (A3.block_recipe(E, nb, mh, 175), R.recipe_input((c["B"], *c["dims"], E), 175),
            R.recipe_input((c["B"], *c["dims"], E), 225), nb, c["modes"])


def test_block3d_vs_reference(guarded):
    fx = load("g17_dpot3d")
    p0, x0, g0, nb, modes = _block_inputs()
    y, dx, dp = _run_block(p0, x0, g0, nb, modes, "gelu")
    assert_close(y, fx["block3d.y"], "block3d.y")
    assert_close(dx, fx["block3d.dx"], "block3d.dx")
    for k, g in dp.items():
        assert g is not None, k
        assert_close(g, fx[f"block3d.d.{k}"], f"block3d.d.{k}")


def test_block3d_leaky_relu_vs_float64(guarded):
    p0, x0, g0, nb, modes = _block_inputs()
    y, dx, dp = _run_block(p0, x0, g0, nb, modes, "leaky_relu")
    x64 = x0.double().requires_grad_(True)
    p64 = OrderedDict((k, v.double().requires_grad_(True)) for k, v in p0.items())
    y64 = A3.block3d_ref(x64, p64, nb, modes, "leaky_relu")
    (y64 * g0.double()).sum().backward()
    assert_close(y, y64, "block3d leaky y")
    assert_close(dx, x64.grad, "block3d leaky dx")
    for k, g in dp.items():
        assert_close(g, p64[k].grad, f"block3d leaky d.{k}")


# ---- the model -----------------------------------------------------------------------------------------------------------
def _shapes(m):
    return OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())


def build3d(cfg, salt):
    from dpot_amd import DPOTNet3D
    m = DPOTNet3D(**cfg)
    sd = A3.recipe_sd(_shapes(m), cfg["n_blocks"], salt)
    m.load_state_dict(sd)
    return m.cuda(), sd


@pytest.mark.parametrize("tag,cfg,salt", [("mini", A3.MINI3D, 176), ("mini_norm", A3.MINI3D_NORM, 178)])
def test_mini_model_vs_reference(tag, cfg, salt, guarded):
    from dpot_amd.functional import rel_l2_loss
    fx = load("g17_dpot3d")
    m, _ = build3d(cfg, salt)
    S, T, C = cfg["img_size"], cfg["in_timesteps"], cfg["in_channels"]
    x = guard.wrap(R.recipe_input((B, S, S, S, T, C), salt), "cuda")
    y = guard.wrap(R.recipe_input((B, S, S, S, cfg["out_timesteps"], cfg["out_channels"]), salt + 1), "cuda")
    msk = guard.wrap(A3.recipe_mask(tuple(y.shape), salt), "cuda")
    pred = m(x)
    assert torch.is_tensor(pred) and tuple(pred.shape) == tuple(y.shape)          # one tensor, not a pair
    loss = rel_l2_loss(pred, y, msk)
    loss.backward()
    torch.cuda.synchronize()
    print(f"{tag}: pred max|d| / max|ref| {_rel(pred, torch.from_numpy(fx[f'{tag}.pred'])):.2e}  "
          f"reference-fp32 vs float64 {float(fx[f'{tag}.err32.pred']):.2e}")
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred")
    assert abs(loss.item() - float(fx[f"{tag}.loss"])) <= 1e-4 * float(fx[f"{tag}.loss"])
    grads = {k: p.grad for k, p in m.named_parameters()}
    assert sorted(str(n) for n in fx[f"{tag}.names"]) == sorted(k for k in grads if not k.startswith("cls_head."))
    for n in fx[f"{tag}.names"]:
        n = str(n)
        assert grads[n] is not None, n
        assert_close(grads[n], fx[f"{tag}.g.{n}"], f"{tag}.g.{n}")
    for n in fx[f"{tag}.nograd"]:                                                  # cls_head: None or zero, as the reference
        g = grads[str(n)]
        assert g is None or not g.any(), n


def test_odd_patch_forward_vs_float64(guarded):
    """img_size 12, patch_size 3: latent 4^3 from an odd patch, against torch CPU convolutions around the restatement"""
    cfg = dict(A3.MINI3D, img_size=12, patch_size=3, modes=32, act="leaky_relu", time_agg="mlp")
    m, sd = build3d(cfg, 190)
    x0 = R.recipe_input((B, 12, 12, 12, 3, 2), 191)
    with torch.no_grad():
        pred = m(guard.wrap(x0, "cuda"))
    torch.cuda.synchronize()
    assert_close(pred, A3.model3d_ref(sd, x0, cfg), "odd patch forward")


def test_one_finetune_step(guarded):
    """2-D blocks and time aggregator loaded, two AR steps as finetune3d.py:205-222, backward, clip, fused Adam"""
    from dpot_amd import load_3d_components_from_2d
    from dpot_amd.functional import rel_l2_loss
    from dpot_amd.train import FlatParams, FusedAdam
    fx = load("g17_dpot3d")
    cfg, st = A3.MINI3D, A3.STEP
    m, _ = build3d(cfg, 182)
    load_3d_components_from_2d(m, R.recipe_state_dict(R.DPOTConfig(**A3.MINI2D), 183), ["blocks", "time_agg"])
    S, T, C = cfg["img_size"], cfg["in_timesteps"], cfg["in_channels"]
    xx = guard.wrap(R.recipe_input((B, S, S, S, T, C), 182), "cuda")
    yy = R.recipe_input((B, S, S, S, st["T_ar"], C), 183).cuda()
    msk = guard.wrap(A3.recipe_mask((B, S, S, S, 1, C), 182), "cuda")
    opt = FusedAdam(FlatParams(m), lr=st["lr"], betas=st["betas"], weight_decay=st["weight_decay"], max_norm=st["max_norm"])
    cls_before = [p.detach().clone() for p in m.cls_head.parameters()]
    opt.zero_grad()
    loss = 0.
    for t in range(st["T_ar"]):
        im = m(xx)
        loss = loss + rel_l2_loss(im, yy[..., t:t + 1, :].contiguous(), msk)
        xx = torch.cat((xx[..., 1:, :], im), dim=-2)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    assert abs(loss.item() - float(fx["step.loss"])) <= 1e-4 * float(fx["step.loss"])
    assert abs(opt.grad_norm().item() - float(fx["step.grad_norm"])) <= 1e-4 * float(fx["step.grad_norm"])
    sd = m.state_dict()
    for n in fx["step.names"]:
        n = str(n)
        stride = int(fx[f"step.p.{n}.stride"])
        got = sd[n].detach().cpu().reshape(-1)[::stride]
        assert (got - torch.from_numpy(fx[f"step.p.{n}.sub"])).abs().max().item() <= 0.05 * st["lr"], n
    for p, q in zip(m.cls_head.parameters(), cls_before):                          # no gradient -> skipped, as the reference
        assert torch.equal(p.detach(), q)


def test_forward_graph_capture_replays_bit_for_bit(guarded):
    m, _ = build3d(A3.MINI3D, 176)
    x = R.recipe_input((B, 8, 8, 8, 3, 2), 176).cuda()
    with torch.no_grad():
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            eager = m(x).clone()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            out = m(x)
        out.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
    assert torch.equal(out, eager)


def test_unsupported_grid_raises_and_launches_nothing(guarded):
    from dpot_amd import _lib, ops
    dims = (40, 40, 40)
    m3 = ops.kept_modes3(dims, 32)
    assert not ops.dft3_supported(dims, 32, m3)
    dummy = guard.wrap(torch.zeros(1), "cuda")          # a launch would read 2 * 40^3 * 32 floats from a 1-element buffer
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.rfft3(dummy.view(1, 1, 1).expand(1, 1, 32), dims, 4, m3)
    with pytest.raises((ValueError, _lib.DpotHipError)):
        ops.irfft3(dummy, 1, dims, 32, 4, m3)
    lib = _lib.load()                                   # the C entry points themselves: DPOT_EUNSUP before any launch
    s = torch.cuda.current_stream().cuda_stream
    assert lib.dpot_rfft3(dummy.data_ptr(), dummy.data_ptr(), 1, 40, 40, 40, 32, 4, *m3, 0, s) == -2
    assert lib.dpot_irfft3(dummy.data_ptr(), None, dummy.data_ptr(), 1, 40, 40, 40, 32, 4, *m3, 1, s) == -2
    torch.cuda.synchronize()
    assert dummy.item() == 0.0
