"""CPU-side checks of the weight-gradient lane's C ABI (csrc/gemm_tn.hip): the new entry points are declared in the header,
exported by the library and bound in the ctypes table with the header's argument lists; without a device nothing is pending,
and the wait is a no-op that may be repeated."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpot_wgrad_lane_init", "dpot_wgrad_lane_ready", "dpot_wgrad_lane_pending", "dpot_wgrad_lane_shutdown",
       "dpot_wgrad_flush_async", "dpot_wgrad_wait")


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


def _ctype_of(decl: str):
    """ctypes type of one parameter declaration of include/dpot_hip.h, as dpot_amd/_lib.py spells it"""
    from dpot_amd import _lib
    decl = " ".join(decl.split())
    if decl.startswith("const float* const*"):
        return C.POINTER(C.c_void_p)
    if decl.startswith("const dpot_wgrad_block*"):
        return C.POINTER(_lib.WgradBlock)
    if decl.startswith(("float*", "const float*", "dpot_stream_t")):
        return _lib.c_fp
    if decl.startswith("int "):
        return _lib.c_i
    raise AssertionError(f"unexpected parameter {decl!r}")


def test_lane_symbols_in_header_table_and_library(built_lib):
    from dpot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpot_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name in NEW:
        m = re.search(r"\bint " + name + r"\(([^)]*)\);", hdr)
        assert m, name
        params = [p for p in m.group(1).split(",") if p.strip() != "void"]
        res, args = _lib.SIGNATURES[name]
        assert res is _lib.c_i, name
        assert args == [_ctype_of(p) for p in params], name
        assert f" T {name}\n" in exported, name
    assert _lib.load().dpot_version() >= 268


def test_flush_takes_what_the_three_launch_sets_take(built_lib):
    """dpot_wgrad_flush_async's parameters are those of dpot_mlp_wgrad_batch, dpot_afno_wgrad_batch and
    dpot_wgrad_batch_finalize, each name once (the stream last)"""
    hdr = open(os.path.join(ROOT, "include", "dpot_hip.h")).read()

    def names(fn):
        body = re.search(r"\bint " + fn + r"\(([^)]*)\);", hdr).group(1)
        return [re.sub(r".*[ *]", "", " ".join(p.split())) for p in body.split(",")]

    three = names("dpot_mlp_wgrad_batch") + names("dpot_afno_wgrad_batch") + names("dpot_wgrad_batch_finalize")
    rename = {"workspace": None, "splitk": None, "splits12": "afno_splits12"}       # per-launch names: mlp_ / afno_ prefixed
    want = {rename.get(n, n) for n in three} - {None} | {"mlp_ws", "afno_ws", "mlp_splitk", "afno_splitk"}
    got = names("dpot_wgrad_flush_async")
    assert len(got) == len(set(got)) and set(got) == want, set(got) ^ want
    assert got[-1] == "stream"


def test_nothing_pending_without_a_flush(built_lib):
    from dpot_amd import _lib
    lib = _lib.load()
    assert lib.dpot_wgrad_lane_pending() == 0
    assert lib.dpot_wgrad_wait(None) == 0 and lib.dpot_wgrad_wait(None) == 0
    assert lib.dpot_wgrad_lane_pending() == 0
