"""CPU-side checks of the lane table's C ABI (csrc/gemm_tn.hip dpot_lane_*): the new entry points are declared in the header,
exported by the library and bound in the ctypes table with the header's argument lists; without a device nothing is pending
and a join is a no-op that may be repeated; the dpot_wgrad_* entry points, now users of lane 0, keep their declarations."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpot_lane_init", "dpot_lane_ready", "dpot_lane_pending", "dpot_lane_shutdown", "dpot_lane_fork", "dpot_lane_join")
# the weight-gradient lane's declarations as they stood before the lane table (whitespace squeezed)
WGRAD = {
    "dpot_wgrad_lane_init": "void",
    "dpot_wgrad_lane_ready": "void",
    "dpot_wgrad_lane_pending": "void",
    "dpot_wgrad_lane_shutdown": "void",
    "dpot_wgrad_wait": "dpot_stream_t stream",
    "dpot_wgrad_flush_async": (
        "const float* const* do2, const float* const* Hh, const float* const* xn2, const float* const* dHpre, int n, int T, "
        "int E, int mh, float* mlp_ws, int mlp_splitk, const float* const* S, const float* const* dO1pre, "
        "const float* const* O1, const float* const* dO2, int ld, int Mm, int nb, int bs, float* afno_ws, int per_launch, "
        "int afno_splits12, int afno_splitk, const dpot_wgrad_block* blocks, int gn_jobs, int B, int Egn, int mlp_chain, "
        "int afno_chain, dpot_stream_t stream"),
}


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


def _header():
    return open(os.path.join(ROOT, "include", "dpot_hip.h")).read()


def _params(hdr: str, name: str):
    m = re.search(r"\bint " + name + r"\(([^)]*)\);", hdr)
    assert m, name
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def _ctype_of(decl: str):
    """ctypes type of one parameter declaration of include/dpot_hip.h, as dpot_amd/_lib.py spells it"""
    from dpot_amd import _lib
    if decl.startswith("dpot_stream_t*"):
        return C.POINTER(C.c_void_p)
    if decl.startswith("dpot_stream_t "):
        return _lib.c_fp
    if decl.startswith("int "):
        return _lib.c_i
    raise AssertionError(f"unexpected parameter {decl!r}")


def test_lane_symbols_in_header_table_and_library(built_lib):
    from dpot_amd import _lib
    hdr = _header()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name in NEW:
        params = _params(hdr, name)
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_i, name
        assert args == [_ctype_of(p) for p in params], name
        assert params[0] == "int lane", name
        assert f" T {name}\n" in exported, name
    assert _params(hdr, "dpot_lane_fork") == ["int lane", "dpot_stream_t caller", "dpot_stream_t* lane_stream"]
    assert _params(hdr, "dpot_lane_join") == ["int lane", "dpot_stream_t caller"]
    assert _lib.load().dpot_version() >= 272


def test_wgrad_symbols_are_unchanged(built_lib):
    from dpot_amd import _lib
    hdr = _header()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name, want in WGRAD.items():
        assert ", ".join(_params(hdr, name)) == want, name
        assert f" T {name}\n" in exported, name
        assert name in _lib.SIGNATURES and _lib.SIGNATURES[name][0] is _lib.c_i, name
    assert len(_lib.SIGNATURES["dpot_wgrad_flush_async"][1]) == len(_params(hdr, "dpot_wgrad_flush_async"))
    assert _lib.SIGNATURES["dpot_wgrad_wait"][1] == [_lib.c_fp]


def test_nothing_pending_and_join_repeats_without_a_device(built_lib):
    from dpot_amd import _lib
    lib = _lib.load()
    for lane in (0, 1):
        assert lib.dpot_lane_pending(lane) == 0 and lib.dpot_lane_ready(lane) == 0
        assert lib.dpot_lane_join(lane, None) == 0 and lib.dpot_lane_join(lane, None) == 0
        assert lib.dpot_lane_pending(lane) == 0
        assert lib.dpot_lane_shutdown(lane) == 0          # nothing to destroy
    assert lib.dpot_wgrad_lane_pending() == 0 and lib.dpot_wgrad_wait(None) == 0


def test_lane_index_is_checked(built_lib):
    from dpot_amd import _lib
    lib = _lib.load()
    handle = C.c_void_p()
    for lane in (-1, 2):
        assert lib.dpot_lane_pending(lane) == 0 and lib.dpot_lane_ready(lane) == 0
        assert lib.dpot_lane_join(lane, None) != 0
        assert lib.dpot_lane_fork(lane, None, C.byref(handle)) != 0
        assert lib.dpot_lane_init(lane) != 0 and lib.dpot_lane_shutdown(lane) != 0


def test_sites_and_switch():
    """fused_small=5 is the default and selects the default sites; 4 is the schedule without the side lane"""
    from dpot_amd import ops
    assert ops.TUNE_KEYS["fused_small"][0] == 5 and "side lane" in ops.TUNE_KEYS["fused_small"][1]
    assert set(ops.SIDE_SITES_DEFAULT) == set(ops.SIDE_SITES) == {"weights", "patch"}
    with ops.side_lane_scope(("patch",)):
        assert ops.side_lane_enabled("patch") and not ops.side_lane_enabled("weights")
        with ops.side_lane_scope(()):
            assert not any(ops.side_lane_enabled(s) for s in ops.SIDE_SITES)
        assert ops.side_lane_enabled("patch")
    for gone in ("cls", "embed"):          # `cls` failed its ablation (profiles/side_lane_ab.txt): no such site
        with pytest.raises(ValueError):
            with ops.side_lane_scope((gone,)):
                pass
    ops.side_lane_join()                                   # nothing forked: no library call, no device needed
