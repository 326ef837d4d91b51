"""CPU tests of the FNO baseline's host side: the float64 restatement (tests/fno_ref.py) against the reference's records
(tests/golden/g22_fno.npz) and against torch.fft, its autograd against the dense gradient formulas, the twiddle tables of
ops.FNOPlan, the constructor and state_dict layout against the records, the ABI tables and the host checks."""
import inspect
import os
import re
from collections import OrderedDict

import numpy as np
import pytest
import torch

import fno_ref as FR
from helpers import assert_close, load

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_layer_restatement_equals_the_reference_float32_records(name):
    """the float64 restatement against what the reference's own class computed in float32, at the project contract; the recorded
    norm-wise error of that float32 run is a float32 figure"""
    fx = load("g22_fno")
    assert [str(n) for n in fx["layer.names"]] == list(FR.LAYER_CASES)
    x, g, w1, w2 = FR.layer_inputs(name)
    xd, w1d, w2d = (t.double().requires_grad_(True) for t in (x, w1, w2))
    y = FR.spectral_conv(xd, w1d, w2d)
    (y * g.double()).sum().backward()
    for k, t in (("y", y.detach()), ("dx", xd.grad), ("dw1", w1d.grad), ("dw2", w2d.grad)):
        assert_close(t, fx[f"layer.{name}.{k}32"], f"layer.{name}.{k} vs the reference's float32")
        assert_close(t, fx[f"layer.{name}.{k}64"], f"layer.{name}.{k} vs its record", rtol=1e-12, atol_scale=1e-12)
        assert float(fx[f"layer.{name}.e32.{k}"]) < 1e-5


@pytest.mark.parametrize("name", list(FR.LAYER_CASES))
def test_autograd_of_the_restatement_equals_the_dense_gradient_formulas(name):
    x, g, w1, w2 = (t.double() for t in FR.layer_inputs(name))
    xd, w1d, w2d = (t.clone().requires_grad_(True) for t in (x, w1, w2))
    (FR.spectral_conv(xd, w1d, w2d) * g).sum().backward()
    dx, d1, d2 = FR.spectral_conv_grads(x, w1, w2, g)
    assert_close(dx, xd.grad, f"{name} dx", rtol=1e-11, atol_scale=1e-11)
    assert_close(d1, w1d.grad, f"{name} dweights1", rtol=1e-11, atol_scale=1e-11)
    assert_close(d2, w2d.grad, f"{name} dweights2", rtol=1e-11, atol_scale=1e-11)


@pytest.mark.parametrize("case", [c for c in FR.TRANSFORM_CASES if c[1] <= 72], ids=str)
def test_dft_matrices_and_twiddle_tables_equal_torch_fft(case):
    """the restatement's matrices, and the tables the kernels read, against torch.fft in float64: the kept rows and columns of
    rfft2, and irfft2 of the zero-filled half spectrum (which is not Hermitian on column 0 and the Nyquist column)"""
    from dpot_amd import ops
    B, H, W, C, m1, m2 = case
    x, Sp = FR.transform_inputs(case)
    x, S = x.double(), FR.from_planes(Sp.double())
    Xf = torch.fft.rfft2(x, dim=(1, 2))
    want = torch.cat([Xf[:, :m1, :m2], Xf[:, H - m1:, :m2]], dim=1)
    got = FR.rfft2_kept(x, m1, m2)
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()
    half = torch.zeros(B, H, W // 2 + 1, C, dtype=torch.complex128)
    half[:, :m1, :m2], half[:, H - m1:, :m2] = S[:, :m1], S[:, m1:]
    inv = torch.fft.irfft2(half, s=(H, W), dim=(1, 2))
    assert (FR.irfft2_kept(S, H, W) - inv).abs().max() <= 1e-12 * inv.abs().max()
    tx, ty = ops.fno_twiddles(H, W, m1, m2)
    Fx, Fy = FR.dft_matrices(H, W, m1, m2)
    assert tx.shape == (H, 2 * m1, 2) and ty.shape == (W, m2, 2) and tx.dtype == np.float64
    assert np.abs((tx[..., 0] - 1j * tx[..., 1]).T - Fx.numpy()).max() <= 1e-15
    assert np.abs((ty[..., 0] - 1j * ty[..., 1]) - Fy.numpy()).max() <= 1e-15
    assert np.array_equal(ops.fno_kept_rows(H, m1), FR.kept_rows(H, m1))
    assert np.array_equal(ops.fno_col_weights(W, m2), FR.col_weights(W, m2).numpy())


def test_adjoint_roles_are_adjoints():
    """<rfft2_kept x, S> = <x, irfft2_kept(S, weights off, scale 1)> and <irfft2_kept S, g> = <S, w / (H W) rfft2_kept g>"""
    for case in FR.TRANSFORM_CASES[:5]:
        B, H, W, C, m1, m2 = case
        r = FR.transform_ref(case)
        x, Sp = (t.double() for t in FR.transform_inputs(case))
        a, b = (r["fwd"] * Sp).sum(), (x * r["adj_fwd"]).sum()
        assert abs(a - b) <= 1e-12 * abs(a)
        a, b = (r["inv"] * x).sum(), (Sp * r["adj_inv"]).sum()
        assert abs(a - b) <= 1e-12 * abs(a)


def test_constructor_signature_equals_the_reference():
    from dpot_amd import FNO2d
    sig = inspect.signature(FNO2d.__init__)
    got = [f"{k}={v.default!r}" for k, v in sig.parameters.items() if k != "self"]
    assert got == [str(s) for s in load("g22_fno")["signature"]]


@pytest.mark.parametrize("normalize,use_ln", [(0, 0), (0, 1), (1, 0), (1, 1)])
def test_state_dict_layout_and_strict_load(normalize, use_ln, capsys):
    from dpot_amd import FNO2d
    from dpot_amd.train import FlatParams
    fx = load("g22_fno")
    cfg = dict(FR.MINI1, normalize=bool(normalize), use_ln=4 * use_ln)
    m = FNO2d(**cfg)
    assert capsys.readouterr().out == ""
    names = [str(n) for n in fx[f"sd{normalize}{use_ln}.names"]]
    shapes = fx[f"sd{normalize}{use_ln}.shapes"]
    got = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    assert list(got) == names
    for (k, s), row in zip(got.items(), shapes):
        assert list(s) + [0] * (5 - len(s)) == [int(v) for v in row], k
    assert list(got.items()) == list(FR.expected_shapes(cfg).items())             # the restated layout is the recorded one
    weights = FR.recipe_sd(got, 7)
    res = m.load_state_dict(weights, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    fp = FlatParams(m)
    assert len(fp.params) == len(got) and [n for n in fp.names if n.startswith("cls_head.")] == fp.names[-6:]


@pytest.mark.parametrize("tag", list(FR.MODELS))
def test_model_restatement_equals_the_reference(tag):
    """the record is the reference's float64 run, whose spectrum is rounded to complex64 (5e-8) and which is stored as float32:
    compared at 1e-6"""
    fx = load("g22_fno")
    cfg = FR.MODELS[tag][0]
    got = OrderedDict((str(n), tuple(int(v) for v in s if v) or (0,)) for n, s in zip(fx[f"{tag}.names"], fx[f"{tag}.shapes"]))
    assert list(got) == list(FR.expected_shapes(cfg))
    pred, cls_pred, grads, dx = FR.run_model_ref(tag)
    h = cfg["img_size"] // cfg["patch_size"]
    assert tuple(pred.shape) == (FR.MODEL_B, h, h, cfg["out_timesteps"], cfg["n_channels"])
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred", rtol=1e-6, atol_scale=1e-6)
    assert_close(cls_pred, fx[f"{tag}.cls_pred"], f"{tag}.cls_pred", rtol=1e-6, atol_scale=1e-6)
    assert_close(dx.reshape(-1)[::FR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx", rtol=1e-6, atol_scale=1e-6)
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    for k, g in grads.items():
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}", rtol=1e-6, atol_scale=1e-6)


def test_header_ctypes_table_and_exported_symbols_agree():
    from dpot_amd import _lib
    with open(os.path.join(ROOT, "include", "dpot_hip.h")) as f:
        header = f.read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(dpot_fno_\w+)\(", header, flags=re.M)))
    assert declared == ["dpot_fno_dact", "dpot_fno_irfft2", "dpot_fno_max_size", "dpot_fno_mix", "dpot_fno_mix_wgrad",
                        "dpot_fno_rfft2"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("dpot_fno_")) == declared
    lib = _lib.load()
    assert lib.dpot_version() >= 275
    for name in declared:
        assert hasattr(lib, name)
        proto = re.search(r"^(?:int|int64_t)\s+" + name + r"\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        assert len(proto.split(",")) == len(_lib.SIGNATURES[name][1]), name           # one ctypes entry per C argument
    assert lib.dpot_fno_max_size(0) >= 256 and lib.dpot_fno_max_size(1) >= 32


def test_the_two_refusals_and_the_limits():
    import dpot_amd
    from dpot_amd import FNO2d, ops
    assert "FNO2d" in dpot_amd.__all__ and dpot_amd.FNO2d is FNO2d
    with pytest.raises(ValueError, match=r"modes1 = 6.*H = 10"):
        FNO2d(6, 4, 8, img_size=10)
    with pytest.raises(ValueError, match=r"modes2 = 7.*W = 10"):
        FNO2d(4, 7, 8, img_size=10)
    with pytest.raises(ValueError, match=r"modes1 = 3.*H = 4"):
        FNO2d(3, 2, 8, img_size=12, patch_size=3)                                  # the field is the 4 x 4 latent grid
    FNO2d(5, 6, 8, img_size=10)                                                    # 2 m1 = H and the Nyquist column: allowed
    x = torch.zeros(1, 6, 6, 2)                                                    # CPU tensors: the size checks come first
    with pytest.raises(ValueError, match="modes1 = 4"):
        ops.fno_rfft2(x, 4, 2)
    with pytest.raises(ValueError, match="modes2 = 5"):
        ops.fno_rfft2(x, 2, 5)
    with pytest.raises(ValueError, match="modes2 = 5"):
        ops.fno_irfft2(torch.zeros(1, 4, 5, 2, 2), 6, 6)
    assert ops.fno_supported(256, 256, 32, 32) and ops.fno_supported(64, 128, 32, 32) and ops.fno_supported(7, 9, 3, 4)
    assert not ops.fno_supported(512, 64, 8, 8) and not ops.fno_supported(8, 8, 5, 2) and not ops.fno_supported(8, 8, 2, 6)
    with pytest.raises(ValueError, match="512x64"):
        ops.FNOPlan(512, 64, 8, 8, "cpu")


def test_cpu_tensors_raise_the_no_cpu_fallback_error():
    from dpot_amd import FNO2d, _lib, ops
    m = FNO2d(**FR.MINI1)
    with pytest.raises(_lib.DpotHipError, match="no CPU fallback"):
        m(torch.zeros(1, 10, 10, 3, 2))
    with pytest.raises(_lib.DpotHipError):
        ops.fno_rfft2(torch.zeros(1, 6, 6, 2), 2, 2)
    w = torch.zeros(2, 2, 2, 2, 2)
    with pytest.raises(_lib.DpotHipError):
        ops.fno_mix(torch.zeros(1, 4, 2, 2, 2), w, w)
    with pytest.raises(_lib.DpotHipError):
        ops.fno_mix_wgrad(torch.zeros(1, 4, 2, 2, 2), torch.zeros(1, 4, 2, 2, 2))
    with pytest.raises(_lib.DpotHipError):
        ops.act_bwd_mul(torch.zeros(4), torch.zeros(4), 1)
