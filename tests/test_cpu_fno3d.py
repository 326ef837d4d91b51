"""CPU tests of the 3-D FNO baseline's host side: the float64 restatement (tests/fno3d_ref.py) against the reference's records
(tests/golden/g23_fno3d.npz) and against torch.fft, its autograd against the dense gradient formulas, the twiddle tables of
ops.FNO3Plan, the constructor and the complex state_dict against the records, the pair rule of Adam against the recorded step,
the ABI tables and the host checks."""
import inspect
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fno3d_ref as FR
from helpers import assert_close, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SMALL = [c for c in FR.TRANSFORM_CASES if c[1] <= 17]


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_layer_restatement_equals_the_reference_float32_records(name):
    """the float64 restatement against what the reference's own class computed in float32, at the project contract"""
    fx = load("g23_fno3d")
    assert [str(n) for n in fx["layer.names"]] == list(FR.LAYER_CASES)
    x, g, ws = FR.layer_inputs(name)
    xd = x.double().requires_grad_(True)
    wd = [w.to(torch.complex128).requires_grad_(True) for w in ws]
    y = FR.spectral_conv(xd, wd)
    (y * g.double()).sum().backward()
    res = [("y", y.detach()), ("dx", xd.grad)] + [(f"dw{k + 1}", FR.pairs(w.grad)) for k, w in enumerate(wd)]
    for k, t in res:
        assert_close(t, fx[f"layer.{name}.{k}32"], f"layer.{name}.{k} vs the reference's float32")
        assert_close(t, fx[f"layer.{name}.{k}64"], f"layer.{name}.{k} vs its record", rtol=1e-12, atol_scale=1e-12)
        assert float(fx[f"layer.{name}.e32.{k}"]) < 1e-5


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_autograd_of_the_restatement_equals_the_dense_gradient_formulas(name):
    x, g, ws = FR.layer_inputs(name)
    x, g, ws = x.double(), g.double(), [w.to(torch.complex128) for w in ws]
    xd, wd = x.clone().requires_grad_(True), [w.clone().requires_grad_(True) for w in ws]
    (FR.spectral_conv(xd, wd) * g).sum().backward()
    dx, dws = FR.spectral_conv_grads(x, ws, g)
    assert_close(dx, xd.grad, f"{name} dx", rtol=1e-11, atol_scale=1e-11)
    for k, (d, w) in enumerate(zip(dws, wd)):
        assert_close(FR.pairs(d), FR.pairs(w.grad), f"{name} dweights{k + 1}", rtol=1e-11, atol_scale=1e-11)


@pytest.mark.parametrize("case", SMALL, ids=str)
def test_dft_matrices_and_twiddle_tables_equal_torch_fft(case):
    """the restatement's matrices, and the tables the kernels read, against torch.fft in float64: the four kept corners of
    rfftn, and irfftn of the zero-filled half spectrum (which is not Hermitian on the kz = 0 and the Nyquist plane)"""
    from dpot_amd import ops
    B, X, Y, Z, C, m1, m2, m3 = case
    x, Sp = FR.transform_inputs(case)
    x, S = x.double(), FR.from_planes(Sp.double())
    Xf = torch.fft.rfftn(x, dim=(1, 2, 3))
    want = Xf[:, torch.from_numpy(FR.kept(X, m1))][:, :, torch.from_numpy(FR.kept(Y, m2))][:, :, :, :m3]
    got = FR.rfft3_kept(x, m1, m2, m3)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    half = FR.scatter(S, (B, X, Y, Z // 2 + 1, C), X, Y, m1, m2, m3)
    inv = torch.fft.irfftn(half, s=(X, Y, Z), dim=(1, 2, 3))
    assert (FR.irfft3_kept(S, X, Y, Z) - inv).abs().max() <= 1e-12 * inv.abs().max()
    tabs = ops.fno3_twiddles(X, Y, Z, m1, m2, m3)
    mats = FR.dft_matrices(X, Y, Z, m1, m2, m3)
    for t, F_, n, k in zip(tabs, mats, (X, Y, Z), (2 * m1, 2 * m2, m3)):
        assert t.shape == (n, k, 2) and t.dtype == np.float64
        assert np.abs((t[..., 0] - 1j * t[..., 1]) - F_.numpy()).max() <= 1e-15
    assert np.array_equal(ops.fno_col_weights(Z, m3), FR.plane_weights(Z, m3).numpy())


def test_one_hot_dc_and_nyquist_planes_ignore_the_imaginary_part():
    """a spectrum with ONE purely imaginary entry on the kz = 0 plane, or on the Nyquist plane of an even Z, at a self-conjugate
    (kx, ky): irfftn gives zero, and so does the restatement; off those planes the same entry gives a sine wave"""
    X, Y, Z, m1, m2, m3 = 4, 4, 6, 2, 2, 4
    for kz, dead in ((0, True), (3, True), (1, False)):
        S = torch.zeros(1, 2 * m1, 2 * m2, m3, 1, dtype=torch.complex128)
        S[0, 0, 0, kz, 0] = 1j
        half = torch.zeros(1, X, Y, Z // 2 + 1, 1, dtype=torch.complex128)
        half[0, 0, 0, kz, 0] = 1j
        want = torch.fft.irfftn(half, s=(X, Y, Z), dim=(1, 2, 3))
        got = FR.irfft3_kept(S, X, Y, Z)
        assert (got - want).abs().max() <= 1e-15
        assert (want.abs().max() < 1e-15) == dead


def test_adjoint_roles_are_adjoints():
    """<rfft3_kept x, S> = <x, irfft3_kept(S, weights off, scale 1)> and <irfft3_kept S, g> = <S, w / (X Y Z) rfft3_kept g>"""
    for case in SMALL:
        r = FR.transform_ref(case)
        x, Sp = (t.double() for t in FR.transform_inputs(case))
        a, b = (r["fwd"] * Sp).sum(), (x * r["adj_fwd"]).sum()
        assert abs(a - b) <= 1e-12 * abs(a)
        a, b = (r["inv"] * x).sum(), (Sp * r["adj_inv"]).sum()
        assert abs(a - b) <= 1e-12 * abs(a)


def test_constructor_signature_equals_the_reference():
    from dpot_amd import FNO3d
    sig = inspect.signature(FNO3d.__init__)
    got = [f"{k}={v.default!r}" for k, v in sig.parameters.items() if k != "self"]
    assert got == [str(s) for s in load("g23_fno3d")["signature"]]
    assert FNO3d.cls_output is False


@pytest.mark.parametrize("normalize,use_ln", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_state_dict_layout_strict_load_and_round_trip(normalize, use_ln, capsys):
    from dpot_amd import FNO3d
    from dpot_amd.infer import load_model_from_checkpoint
    from dpot_amd.train import FlatParams
    fx = load("g23_fno3d")
    cfg = dict(FR.MINI1, normalize=bool(normalize), use_ln=bool(use_ln))
    m = FNO3d(**cfg)
    assert capsys.readouterr().out == ""
    tag = f"sd{normalize}{use_ln}"
    names, dtypes = [str(n) for n in fx[f"{tag}.names"]], [str(d) for d in fx[f"{tag}.dtypes"]]
    got = OrderedDict((k, (tuple(v.shape), v.dtype)) for k, v in m.state_dict().items())
    assert list(got) == names
    for (k, (s, d)), row, dt in zip(got.items(), fx[f"{tag}.shapes"], dtypes):
        assert list(s) + [0] * (5 - len(s)) == [int(v) for v in row], k
        assert str(d) == dt, k
    assert list(got.items()) == list(FR.expected_layout(cfg).items())              # the restated layout is the recorded one
    weights = FR.recipe_sd(got, 7)                                                 # reference-shaped: complex64 spectral weights
    res = m.load_state_dict(weights, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    back = m.state_dict()
    for k, v in weights.items():
        assert back[k].dtype == v.dtype and torch.equal(back[k], v), k             # bit-exact round trip
    m2 = FNO3d(**cfg)
    load_model_from_checkpoint(m2, {"model": OrderedDict(("module." + k, v) for k, v in back.items())})
    assert all(torch.equal(a, b) for a, b in zip(m2.state_dict().values(), back.values()))
    for n, p in m.named_parameters():                                              # parameters are real pairs
        assert p.dtype == torch.float32
        if ".weights" in n:
            assert p.shape[-1] == 2 and p._dpot_complex_pairs and torch.equal(p.detach(), FR.pairs(weights[n]))
    with pytest.raises(RuntimeError, match="weights3"):
        m.load_state_dict(OrderedDict((k, v) for k, v in weights.items() if not k.endswith("0.weights3")), strict=True)
    with pytest.raises(RuntimeError, match="size mismatch"):
        m.load_state_dict(OrderedDict((k, v.real if v.is_complex() else v) for k, v in weights.items()), strict=True)
    fp = FlatParams(m)
    assert not any(n.startswith("scale_feats") for n in fp.names)                  # no gradient in the reference: not optimised
    assert len(fp.params) == len(got) - 2 * normalize
    assert all(o % 4 == 0 for o in fp.offsets)


@pytest.mark.parametrize("tag", list(FR.MODELS))
def test_model_restatement_equals_the_reference(tag):
    """the record is the reference's float32 run: compared at the project contract"""
    fx = load("g23_fno3d")
    cfg, size, _ = FR.MODELS[tag]
    pred, grads, dx = FR.run_model_ref(tag)
    assert tuple(pred.shape) == (FR.MODEL_B, *size, cfg["out_timesteps"], cfg["n_channels"])
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred")
    assert_close(dx.reshape(-1)[::FR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx")
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    assert [str(n) for n in fx[f"{tag}.nograd"]] == (["scale_feats.weight", "scale_feats.bias"] if cfg["normalize"] else [])
    for k, g in grads.items():
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}")


def test_pair_adam_restatement_reproduces_the_recorded_step_and_the_per_component_rule_does_not():
    """the float64 pair rule from the RECORDED gradient reproduces the recorded parameters; Adam on the real view does not, by
    the printed margin: the fixture tells the two apart"""
    fx = load("g23_fno3d")
    names = [str(n) for n in fx["step.names"]]
    losses, grads, gnorm, start = FR.run_step_ref()
    assert names == list(grads) and [str(n) for n in fx["step.nograd"]] == []
    np.testing.assert_allclose(losses, fx["step.losses"], rtol=1e-5)
    assert abs(gnorm - float(fx["step.grad_norm"])) <= 1e-5 * gnorm
    assert_close(torch.cat([FR.pair_stride(g) for g in grads.values()]), fx["step.grad"], "step gradient")
    ref_g, ref_p = torch.from_numpy(fx["step.grad"]).double(), torch.from_numpy(fx["step.params"]).double()
    owner = torch.cat([torch.full((FR.pair_stride(start[n]).numel(),), i, dtype=torch.int64) for i, n in enumerate(names)])
    p0 = torch.cat([FR.pair_stride(start[n]) for n in names]).double()
    tol = FR.step_param_tolerance(ref_g, ref_p, p0, owner, names, float(fx["step.grad_norm"]))
    worst_pair = worst_comp = 0.0
    for i, n in enumerate(names):
        sel = owner == i
        is_pair = ".weights" in n
        got = FR.adam_first_step(p0[sel], ref_g[sel], float(fx["step.grad_norm"]), is_pair)
        err = (got - ref_p[sel]).abs()
        assert (err <= tol[sel]).all(), (n, float((err / tol[sel]).max()))
        if is_pair:
            wrong = FR.adam_first_step(p0[sel], ref_g[sel], float(fx["step.grad_norm"]), True, per_component=True)
            worst_pair = max(worst_pair, float((err / tol[sel]).max()))
            worst_comp = max(worst_comp, float(((wrong - ref_p[sel]).abs() / tol[sel]).max()))
    print(f"pair rule: worst err / tol {worst_pair:.2e}; per-component rule: worst err / tol {worst_comp:.1f}")
    assert worst_comp > 10.0


def test_header_ctypes_table_and_exported_symbols_agree():
    from dpot_amd import _lib
    with open(os.path.join(ROOT, "include", "dpot_hip.h")) as f:
        header = f.read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(dpot_fno3_\w+|dpot_adam_step_pairs)\(", header, flags=re.M)))
    assert declared == ["dpot_adam_step_pairs", "dpot_fno3_irfft3", "dpot_fno3_max_size", "dpot_fno3_mix",
                        "dpot_fno3_mix_wgrad", "dpot_fno3_rfft3", "dpot_fno3_ws_elems"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("dpot_fno3_") or n == "dpot_adam_step_pairs") == declared
    lib = _lib.load()
    assert lib.dpot_version() >= 277
    for name in declared:
        assert hasattr(lib, name)
        proto = re.search(r"^(?:int|int64_t)\s+" + name + r"\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name           # one ctypes entry per C argument
    assert lib.dpot_fno3_max_size(0) >= 64 and lib.dpot_fno3_max_size(1) >= 16
    # the workspace is (2 m2 / Y)(2 m3 / Z) of the field: 0.14 at the reference default, and at most (Z + 2) / Z of it (every
    # ky kept and the Nyquist plane too: the half spectrum of a real axis has Z + 2 reals)
    assert lib.dpot_fno3_ws_elems(4, 64, 256, 12, 12) == 4 * 64 * 24 * 12 * 2 * 256 <= 0.15 * 4 * 64 ** 3 * 256
    assert lib.dpot_fno3_ws_elems(1, 8, 4, 4, 5) == 8 * 8 * 5 * 2 * 4 == (8 * 8 * 8 * 4) * 10 // 8


def test_the_two_refusals_and_the_limits():
    import dpot_amd
    from dpot_amd import FNO3d, _lib, ops
    assert "FNO3d" in dpot_amd.__all__ and dpot_amd.FNO3d is FNO3d
    with pytest.raises(ValueError, match=r"modes1 = 6.*X = 10"):
        FNO3d(6, 4, 4, 8, img_size=10)
    with pytest.raises(ValueError, match=r"modes2 = 6.*Y = 10"):
        FNO3d(4, 6, 4, 8, img_size=10)
    with pytest.raises(ValueError, match=r"modes3 = 7.*Z = 10"):
        FNO3d(4, 4, 7, 8, img_size=10)
    FNO3d(5, 5, 6, 8, img_size=10)                                                 # 2 m = N and the Nyquist plane: allowed
    x = torch.zeros(1, 6, 6, 6, 2)                                                 # CPU tensors: the size checks come first
    with pytest.raises(ValueError, match="modes1 = 4"):
        ops.fno3_rfft3(x, 4, 2, 2)
    with pytest.raises(ValueError, match="modes2 = 4"):
        ops.fno3_rfft3(x, 2, 4, 2)
    with pytest.raises(ValueError, match="modes3 = 5"):
        ops.fno3_rfft3(x, 2, 2, 5)
    with pytest.raises(ValueError, match="modes3 = 5"):
        ops.fno3_irfft3(torch.zeros(1, 4, 4, 5, 2, 2), 6, 6, 6)
    n, m = _lib.load().dpot_fno3_max_size(0), _lib.load().dpot_fno3_max_size(1)
    assert ops.fno3_supported(64, 64, 64, 12, 12, 12) and ops.fno3_supported(n, n, n, m, m, m)
    assert ops.fno3_supported(6, 5, 7, 3, 2, 2)
    assert not ops.fno3_supported(2 * n, 64, 64, 8, 8, 8) and not ops.fno3_supported(8, 8, 8, 5, 2, 2)
    assert not ops.fno3_supported(8, 8, 8, 2, 2, 6) and not ops.fno3_supported(4 * m, 4 * m, 4 * m, m + 1, 2, 2)
    with pytest.raises(ValueError, match=f"{2 * n}x64x64"):
        ops.FNO3Plan(2 * n, 64, 64, 8, 8, 8, "cpu")


def test_cpu_tensors_raise_the_no_cpu_fallback_error():
    from dpot_amd import FNO2d, FNO3d, _lib
    m = FNO3d(**FR.MINI1)
    with pytest.raises(_lib.DpotHipError, match="There is no CPU fallback") as e3:
        m(torch.zeros(1, 6, 5, 7, 3, 2))
    with pytest.raises(_lib.DpotHipError, match="There is no CPU fallback") as e2:
        FNO2d(2, 2, 8, img_size=6, n_channels=2, in_timesteps=3, n_cls=1)(torch.zeros(1, 6, 6, 3, 2))
    assert str(e3.value).replace("FNO3d", "FNO2d") == str(e2.value)


def test_complex_pair_ranges_are_the_spectral_weights():
    """what FusedAdam turns into its device table and FusedLamb refuses: the spectral weights, whole pairs on 4-float offsets"""
    from dpot_amd import FNO2d, FNO3d
    from dpot_amd.train import complex_pair_ranges

    class _Flat:
        def __init__(self, m):
            self.names = [n for n, _ in m.named_parameters()]
            self.params = [p for _, p in m.named_parameters()]
            self.offsets, self.total = [], 0
            for p in self.params:
                self.offsets.append(self.total)
                self.total += (p.numel() + 3) // 4 * 4

    fl = _Flat(FNO3d(**FR.MINI1))
    pairs = complex_pair_ranges(fl, fl.total)
    assert [n for n, _ in pairs] == [n for n in fl.names if ".weights" in n] and len(pairs) == 8
    assert all(lo % 4 == 0 and (hi - lo) % 2 == 0 for _, (lo, hi) in pairs)
    assert complex_pair_ranges(fl, pairs[2][1][0]) == pairs[:2]                    # only what the optimiser updates
    f2 = _Flat(FNO2d(2, 2, 8, img_size=6, n_channels=2, in_timesteps=3, n_cls=1))
    assert complex_pair_ranges(f2, f2.total) == []                                 # [2, ...] planes are not pairs
