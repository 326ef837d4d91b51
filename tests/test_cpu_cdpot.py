"""CPU tests of the CDPOT model's host side: the anti-aliased resize matrices against torch, the constructor and state_dict
layout against the reference's record (tests/golden/g21_cdpot.npz), the float64 restatement (tests/cdpot_ref.py) against the
reference's recorded float64 results, the kink condition of every backward test input, and the host checks."""
import inspect
from collections import OrderedDict

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import cdpot_ref as CR
from helpers import assert_close, load

PAIRS = ([(n, 2 * n) for n in (1, 2, 3, 5, 8, 16, 32)] + [(2 * n, n) for n in (1, 2, 3, 5, 8, 16, 32)]
         + [(5, 20), (7, 28), (7, 30), (8, 32), (16, 128)])


@pytest.mark.parametrize("n,m", PAIRS)
def test_aa_resize_matrix_equals_torch_interpolate(n, m):
    from dpot_amd import ops
    eye = torch.eye(n, dtype=torch.float64).reshape(1, n, 1, n)                      # channel j = the j-th unit vector
    ref = F.interpolate(eye, size=(1, m), mode="bilinear", antialias=True)[0, :, 0, :].t().numpy()
    A = ops.aa_resize_matrix(n, m)
    assert A.shape == (m, n) and A.dtype == np.float64
    assert np.abs(A - ref).max() <= 1e-15
    assert np.abs(A.sum(1) - 1.0).max() <= 1e-15 and (A >= 0).all()
    taps = (A != 0).sum(1).max()
    assert taps <= (2 if m >= n else 4)


def test_tap_tables_reproduce_the_matrices():
    from dpot_amd import ops
    for h, w, H, W in [(1, 1, 8, 8), (5, 7, 20, 30), (16, 16, 128, 128), (64, 64, 64, 64)]:
        core = ops.aa_core_tables(h, w)
        assert core.dtype == np.int32 and len(core) == 32 * (h + w)
        off = 0
        for n in (h, w):
            U, D = ops.aa_resize_matrix(n, 2 * n), ops.aa_resize_matrix(2 * n, n)
            for A, K in ((U, 2), (D, 4), (U.T, 4), (D.T, 2)):
                rows = A.shape[0]
                idx = core[off:off + rows * K].reshape(rows, K)
                wt = core[off + rows * K:off + 2 * rows * K].view(np.float32).reshape(rows, K)
                off += 2 * rows * K
                assert idx.min() >= 0 and idx.max() < A.shape[1]
                dense = np.zeros(A.shape)
                for r in range(rows):
                    for k in range(K):
                        dense[r, idx[r, k]] += wt[r, k]
                assert np.abs(dense - A).max() <= 2.0 ** -24
        up = ops.aa_up_tables(h, w, H, W)
        assert len(up) == 8 * (H + W) + h + w + 2
        for (n, m, o_tap, o_csr) in ((h, H, 0, 4 * H + 4 * W), (w, W, 4 * H, 4 * H + 4 * W + h + 1 + 4 * H)):
            V = ops.aa_resize_matrix(n, m)
            idx = up[o_tap:o_tap + 2 * m].reshape(m, 2)
            assert idx.min() >= 0 and idx.max() < n
            ptr = up[o_csr:o_csr + n + 1]
            ci = up[o_csr + n + 1:o_csr + n + 1 + 2 * m]
            cw = up[o_csr + n + 1 + 2 * m:o_csr + n + 1 + 4 * m].view(np.float32)
            assert ptr[0] == 0 and (np.diff(ptr) >= 0).all() and ptr[-1] <= 2 * m
            dense = np.zeros((n, m))
            for i in range(n):
                for r in range(ptr[i], ptr[i + 1]):
                    assert 0 <= ci[r] < m
                    dense[i, ci[r]] += cw[r]
            assert np.abs(dense - V.T).max() <= 2.0 ** -24


def test_constructor_signature_equals_the_reference():
    from dpot_amd import CDPOTNet
    sig = inspect.signature(CDPOTNet.__init__)
    got = [f"{k}={v.default!r}" for k, v in sig.parameters.items() if k != "self"]
    assert got == [str(s) for s in load("g21_cdpot")["signature"]]


@pytest.mark.parametrize("tag,cfg", [("sd", dict(CR.MINI1, depth=1)), ("m1", CR.MINI1), ("m2", CR.MINI2), ("m3", CR.MINI3)])
def test_state_dict_layout_shared_bias_and_strict_load(tag, cfg, capsys):
    from dpot_amd import CDPOTNet
    from dpot_amd.train import FlatParams
    fx = load("g21_cdpot")
    m = CDPOTNet(**cfg)
    assert capsys.readouterr().out == ""                                          # the constructor prints nothing
    want = CR.ref_shapes(fx, tag)
    got = OrderedDict((k, tuple(v.shape)) for k, v in m.state_dict().items())
    assert list(got.items()) == list(want.items())
    named = dict(m.named_parameters())
    assert len(named) == int(fx[f"{tag}.n_params"]) == len(got) - 1
    sd = m.state_dict(keep_vars=True)
    assert sd["patch_embed.proj.1.bias"] is sd["patch_embed.act_patching.bias"]
    assert m.patch_embed.proj[1] is m.patch_embed.act_patching
    weights = CR.recipe_sd(want, cfg, 7)
    res = m.load_state_dict(weights, strict=True)
    assert not res.missing_keys and not res.unexpected_keys
    for k, v in m.state_dict().items():
        assert torch.equal(v, weights[k]), k
    fp = FlatParams(m)
    assert len(fp.params) == len(named) and sum(n.endswith("act_patching.bias") for n in fp.names) == 1
    assert not any(n == "patch_embed.proj.1.bias" for n in fp.names)
    assert fp.total >= sum(p.numel() for p in named.values())
    assert m.patch_embed.proj[1].bias.data_ptr() == fp.params[fp.names.index("patch_embed.act_patching.bias")].data_ptr()


def test_drop_arguments_change_nothing():
    from dpot_amd import CDPOTNet
    a = CDPOTNet(**CR.MINI1)
    b = CDPOTNet(**CR.MINI1, representation_size=5, uniform_drop=True, drop_rate=0.3, drop_path_rate=0.2, dropcls=0.5)
    assert list(a.state_dict()) == list(b.state_dict())
    assert [tuple(v.shape) for v in a.state_dict().values()] == [tuple(v.shape) for v in b.state_dict().values()]


@pytest.mark.parametrize("name", list(CR.OP_CASES))
def test_operator_restatement_equals_the_reference_float64(name):
    fx = load("g21_cdpot")
    assert [str(n) for n in fx["op.names"]] == list(CR.OP_CASES)
    N, h, C, out = CR.OP_CASES[name]
    x, g, bias = CR.op_inputs(name)
    y, dx, db = CR.run_op_ref(x, g, bias, out)
    for k, t in (("y", y), ("dx", dx), ("db", db)):
        ref = fx[f"op.{name}.{k}64"]
        assert ref.dtype == np.float64
        assert_close(t, ref, f"op.{name}.{k}", rtol=1e-12, atol_scale=1e-12)


@pytest.mark.parametrize("tag", list(CR.MODELS))
def test_model_restatement_equals_the_reference_float64(tag):
    """the record is the reference's float64 run rounded to float32 for storage: 2^-24 per element, compared at 1e-6"""
    fx = load("g21_cdpot")
    pred, cls_pred, grads, dx = CR.run_model_ref(tag)
    assert_close(pred, fx[f"{tag}.pred"], f"{tag}.pred", rtol=1e-6, atol_scale=1e-6)
    assert_close(cls_pred, fx[f"{tag}.cls_pred"], f"{tag}.cls_pred", rtol=1e-6, atol_scale=1e-6)
    assert_close(dx.reshape(-1)[::CR.DX_STRIDE], fx[f"{tag}.dx"], f"{tag}.dx", rtol=1e-6, atol_scale=1e-6)
    assert sorted(grads) == sorted(str(n) for n in fx[f"{tag}.gnames"])
    for k, g in grads.items():
        assert_close(g, fx[f"{tag}.g.{k}"], f"{tag}.g.{k}", rtol=1e-6, atol_scale=1e-6)


def test_kink_condition_of_every_backward_input():
    """no float64 up-sampled value in (0, KINK): there fp32 and float64 could disagree on the sign and the derivative would jump
    between 1 and the slope.  A violation is fixed by another salt, never by a tolerance."""
    fx = load("g21_cdpot")
    for name in CR.OP_CASES:
        assert CR.kink_margin(CR.op_inputs(name)[0]) >= CR.KINK, name
        assert float(fx[f"op.{name}.kink"]) >= CR.KINK
    for case in CR.GPU_OP_CASES:
        assert CR.kink_margin(CR.gpu_op_inputs(case)[0]) >= CR.KINK, case
    for tag in CR.MODELS:
        probe = []
        CR.run_model_ref(tag, probe=probe)
        assert len(probe) == 2
        for i, f in enumerate(probe):
            assert CR.kink_margin(f) >= CR.KINK, (tag, i)
    probe = CR.step_probe()
    assert len(probe) == 2 * CR.STEP["T_ar"]
    for i, f in enumerate(probe):
        assert CR.kink_margin(f) >= CR.KINK, ("step", i)


def test_gpu_case_list_covers_what_the_operator_must_handle():
    cases = CR.GPU_OP_CASES
    assert {(c[1], c[2]) for c in cases} >= {(1, 1), (2, 2), (5, 7), (8, 8), (16, 16), (32, 32), (7, 7)}
    assert {c[3] for c in cases} == {1, 3, 35, 36, 40} and {c[0] for c in cases} == {1, 2, 3}
    assert any(c[4] < c[3] for c in cases) and any(c[4] == c[3] for c in cases)
    mults = {None if c[5] is None else c[5][0] // c[1] for c in cases if c[5] is None or c[5][0] % c[1] == 0}
    assert mults >= {None, 2, 4, 5, 8} and any(c[1] == 7 and c[5] == (30, 30) for c in cases)
    for size in [(1, 1), (2, 2), (5, 7), (8, 8), (16, 16), (32, 32)]:               # every size: with and without an output size,
        sub = [c for c in cases if (c[1], c[2]) == size]                          # scalar and 16-byte channel counts
        assert any(c[5] is None for c in sub) and any(c[5] is not None for c in sub)
        assert any(c[3] % 4 for c in sub) and any(c[3] % 4 == 0 for c in sub)


def test_host_checks():
    import dpot_amd
    from dpot_amd import CDPOTNet, _lib, ops
    assert "CDPOTNet" in dpot_amd.__all__ and dpot_amd.CDPOTNet is CDPOTNet
    lib = _lib.load()
    assert lib.dpot_version() >= 273
    for name in ("dpot_aa_lrelu_fwd", "dpot_aa_lrelu_bwd", "dpot_aa_up_fwd", "dpot_aa_up_adj", "dpot_aa_tab_words",
                 "dpot_aa_vtab_words", "dpot_aa_max_size"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.dpot_aa_max_size(0) == 64 and lib.dpot_aa_tab_words(5, 7) == 32 * 12
    m = CDPOTNet(**CR.MINI1)
    with pytest.raises(_lib.DpotHipError):
        m(torch.zeros(1, 20, 20, 6, 3))
    with pytest.raises(_lib.DpotHipError):
        ops.aa_lrelu(torch.zeros(1, 4, 4, 3), torch.zeros(3))
    with pytest.raises(_lib.DpotHipError):
        ops.aa_lrelu_bwd(torch.zeros(1, 4, 4, 3), torch.zeros(1, 4, 4, 3), 3)
    with pytest.raises(ValueError):
        ops.aa_resize_matrix(0, 4)
