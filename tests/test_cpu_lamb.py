"""The float64 LAMB restatement (tests/lamb_ref.py) against the reference's Lamb (g14_lamb, scripts/make_golden_lamb.py):
per-step updates, final moments, per-tensor norms and trust ratios in the three configurations, and the reference's
state_dict layout that train.FusedLamb mirrors."""
import numpy as np
import pytest

from helpers import assert_close, load
from lamb_ref import LambState, config, lamb_step


def _run(fx, c):
    names = [str(n) for n in fx["names"]]
    params = [fx[f"p0.{n}"].astype(np.float64) for n in names]
    st = LambState(params)
    kw = config(fx, c)
    hist = [list(params)]
    norms = []
    for k in range(int(fx["steps"])):
        params = lamb_step(list(params), [fx[f"g{k}.{n}"] for n in names], st, **kw)
        hist.append(list(params))
        norms.append((st.weight_norm, st.adam_norm, st.trust_ratio))
    return names, hist, norms, st


@pytest.mark.parametrize("c", ["a", "b", "c"])
def test_restatement_matches_reference_lamb(c):
    fx = load("g14_lamb")
    names, hist, norms, st = _run(fx, c)
    prev = {n: fx[f"p0.{n}"].astype(np.float64) for n in names}
    for k in range(1, int(fx["steps"]) + 1):
        for i, n in enumerate(names):
            ref = fx[f"{c}.p{k}.{n}"].astype(np.float64)
            # compare the UPDATE (a 1e-2-relative step hides in p): norm-wise, then element-wise
            du_ref, du = ref - prev[n], hist[k][i] - hist[k - 1][i]
            rel = np.linalg.norm(du - du_ref) / np.linalg.norm(du_ref)
            assert rel <= 1e-4, (c, k, n, rel)         # (the fixture is fp32: p rounds to ~1e-7 of |p|)
            # element-wise, with the fp32 rounding of the fixture's p on top
            tol = 1e-3 * np.abs(du_ref) + 1e-4 * np.abs(du_ref).max() + 2.0 ** -23 * np.abs(ref).max()
            assert (np.abs(du - du_ref) <= tol).all(), (c, k, n, np.abs(du - du_ref).max())
            prev[n] = ref
            for j, key in enumerate(("weight_norm", "adam_norm", "trust_ratio")):
                want = float(fx[f"{c}.{key}{k}.{n}"])
                assert abs(norms[k - 1][j][i] - want) <= 1e-5 * abs(want) + 1e-12, (c, k, n, key)
    for i, n in enumerate(names):
        assert_close(st.m[i], fx[f"{c}.exp_avg.{n}"], f"{c} exp_avg {n}")
        assert_close(st.v[i], fx[f"{c}.exp_avg_sq.{n}"], f"{c} exp_avg_sq {n}")


def test_fixture_covers_the_edge_cases():
    """the zero tensor takes the trust_ratio = 1 branch (kept by the reference as a plain number), the big tensor the
    clamp, the x100 pair lies two orders apart, and configuration c actually clips"""
    fx = load("g14_lamb")
    assert int(fx["b.trust_is_number1.zero"]) == 1 and float(fx["b.trust_ratio1.zero"]) == 1.0
    assert float(fx["b.weight_norm1.big"]) == float(fx["clamp_value"])
    r = float(fx["b.weight_norm1.small_x100"]) / float(fx["b.weight_norm1.small"])
    assert 99.0 < r < 101.0
    assert float(fx["c.total_norm0"]) > float(fx["c.max_norm"])


def test_state_dict_layout_of_reference_lamb():
    fx = load("g14_lamb")
    for c in "abc":
        assert [str(k) for k in fx[f"{c}.state_keys"]] == ["adam_norm", "exp_avg", "exp_avg_sq", "step", "trust_ratio",
                                                          "weight_norm"]
        assert [str(k) for k in fx[f"{c}.group_keys"]] == ["betas", "eps", "lr", "params", "weight_decay"]
        assert int(fx[f"{c}.state_step"]) == int(fx["steps"])


def test_fused_lamb_surface():
    """FusedLamb has the constructor of the reference's Lamb (its defaults) plus the flat-buffer options, and the surface
    the train steps duck-type on (shared with FusedAdam)"""
    import inspect
    from dpot_amd.train import FlatOptimizer, FusedAdam, FusedLamb
    sig = inspect.signature(FusedLamb.__init__)
    want = dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-6, weight_decay=0.0, clamp_value=10.0, adam=False, debias=False,
                max_norm=None, update_tail=False)
    assert {k: sig.parameters[k].default for k in want} == want
    assert issubclass(FusedLamb, FlatOptimizer) and issubclass(FusedAdam, FlatOptimizer)
    for name in ("zero_grad", "stage_hyper", "launch", "step", "grad_norm", "snapshot", "restore", "state_dict",
                 "load_state_dict", "n_active"):
        assert hasattr(FusedLamb, name), name
