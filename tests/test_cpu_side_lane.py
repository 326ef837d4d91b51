"""CPU-side checks of the lane table's C ABI (csrc/lane.hip dpot_lane_*): the entry points are declared in the header,
exported by the library and bound in the ctypes table with the header's argument lists; without a device nothing is pending
and a join is a no-op that may be repeated; the lane-0-only dpot_wgrad_* entry points are gone everywhere; the host
bookkeeping of the one lane object of dpot_amd.ops (forks, forking streams, held tensors) with the library stubbed."""
import ctypes as C
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpot_lane_init", "dpot_lane_ready", "dpot_lane_pending", "dpot_lane_shutdown", "dpot_lane_fork", "dpot_lane_join")
# the lane-0-only entry points that the lane table replaced
REMOVED = ("dpot_wgrad_lane_init", "dpot_wgrad_lane_ready", "dpot_wgrad_lane_pending", "dpot_wgrad_lane_shutdown",
           "dpot_wgrad_wait", "dpot_wgrad_flush_async")


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


def test_wgrad_symbols_are_gone(built_lib):
    """lane 0 is used through dpot_lane_*: none of its own entry points is declared, bound or exported any more"""
    from dpot_amd import _lib
    hdr = _header()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name in REMOVED:
        assert not re.search(r"\b" + name + r"\s*\(", hdr), name
        assert name not in _lib.SIGNATURES, name
        assert f" {name}\n" not in exported, name
        assert not hasattr(_lib.load(), name), name
    assert _lib.load().dpot_version() >= 274


def test_nothing_pending_and_join_repeats_without_a_device(built_lib):
    from dpot_amd import _lib
    lib = _lib.load()
    for lane in (0, 1):
        assert lib.dpot_lane_pending(lane) == 0 and lib.dpot_lane_ready(lane) == 0
        assert lib.dpot_lane_join(lane, None) == 0 and lib.dpot_lane_join(lane, None) == 0
        assert lib.dpot_lane_pending(lane) == 0
        assert lib.dpot_lane_shutdown(lane) == 0          # nothing to destroy


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


class _StubLib:
    """dpot_lane_fork / dpot_lane_join as the library answers them, recorded instead of run"""

    def __init__(self):
        self.forks, self.joins = [], []

    def dpot_lane_fork(self, lane, caller, handle):
        self.forks.append((lane, caller))
        handle._obj.value = 0x1000 + lane           # the lane's stream handle
        return 0

    def dpot_lane_join(self, lane, caller):
        self.joins.append((lane, caller))
        return 0


def test_lane_object_bookkeeping(monkeypatch):
    """the host side of fork and join, no device: what a block leaves behind, one join per distinct forking stream, nesting,
    exceptions, and the join that costs nothing"""
    from dpot_amd import _lib, ops
    lib, step = _StubLib(), [0x10]
    monkeypatch.setattr(_lib, "load", lambda: lib)
    monkeypatch.setattr(ops, "_step_stream", lambda: step[0])
    wg, side = ops._WGRAD, ops._SIDE
    assert (wg.index, side.index) == (0, ops.SIDE_LANE) and wg.forks == side.forks == 0

    ops.wgrad_lane_join()                                  # nothing forked: no library call
    ops.side_lane_join()
    assert lib.forks == [] and lib.joins == []

    a, b, c = object(), object(), object()
    with wg.block(join=False):                             # lane 0, left forked
        assert ops._stream() == 0x1000
        assert ops._scratch(a) is a                        # a workspace its op drops
        ops._hold(b)
        with wg.block(), side.block():                     # nested, either lane: no fork, no join, launches stay on lane 0
            assert ops._stream() == 0x1000
            ops._hold(c)
    assert ops._stream() == 0x10                           # back on the step's stream
    assert lib.forks == [(0, 0x10)] and lib.joins == []
    assert wg.forks == 1 and wg.streams == [0x10] and wg.held == [a, b, c] and side.forks == 0 and side.held == []
    ops._scratch(a)                                        # outside a block nothing is held
    assert wg.held == [a, b, c]

    with wg.block(join=False):                             # the same stream again, then another one
        pass
    step[0] = 0x20
    with wg.block(join=False):
        pass
    assert wg.forks == 3 and wg.streams == [0x10, 0x10, 0x20]
    ops.wgrad_lane_join()                                  # one join per distinct forking stream, whatever is current now
    assert lib.joins == [(0, 0x10), (0, 0x20)]
    assert wg.forks == 0 and wg.streams == [] and wg.held == []
    ops.wgrad_lane_join()
    assert len(lib.joins) == 2

    del lib.joins[:]
    with pytest.raises(RuntimeError, match="boom"):        # an exception inside a block joins, also with join=False
        with wg.block(join=False):
            ops._hold(a)
            raise RuntimeError("boom")
    assert lib.joins == [(0, 0x20)] and wg.forks == 0 and wg.held == [] and ops._stream() == 0x20

    del lib.joins[:], lib.forks[:]
    calls = []
    real_join = ops.side_lane_join
    monkeypatch.setattr(ops, "side_lane_join", lambda: (calls.append(side.forks), real_join()))
    with ops.side_lane("patch", on=False):                 # site off: nothing
        assert ops._stream() == 0x20
    with ops.side_lane("patch", on=True):                  # joins when the block ends, through the module's name
        assert ops._stream() == 0x1001
        with ops.side_lane("weights", on=True):
            pass
        assert calls == []                                 # the nested block neither forked nor joined
    assert lib.forks == [(1, 0x20)] and lib.joins == [(1, 0x20)] and calls == [1] and side.forks == 0
    with ops.side_lane("weights", on=True, join=False):
        pass
    assert side.forks == 1 and calls == [1]
    with pytest.raises(RuntimeError, match="boom"):
        with ops.side_lane("patch", on=True, join=False):  # nested in nothing: the lane is forked a second time
            raise RuntimeError("boom")
    assert calls == [1, 2] and side.forks == 0 and len(lib.joins) == 2
