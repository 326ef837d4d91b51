"""CPU tests of the table plans' shared host path (ops._TablePlan, ops._plan): the order and the dtypes of every class's host
tables (for EvalPlan the order is ABI: eval_metrics_update passes the tables positionally), the upload rule and the cache on the
"cpu" device with the capture query stubbed (a machine without a GPU cannot answer it), and every refusal a plan raises before
it allocates anything."""
import numpy as np
import pytest
import torch

# class name, the smallest sizes its checks admit, and (key, host dtype) of its tables in order
HOST = [
    ("ResizePlan", (4, 4, 6, 6), [("axT", "float32"), ("ayT", "float32"), ("byT", "float32"), ("u", "float32"), ("v", "float32")]),
    ("ResizePlan", (3, 3, 5, 5), [("axT", "float32"), ("ayT", "float32"), ("byT", None), ("u", None), ("v", None)]),
    ("Resize3Plan", (4, 4, 4, 6, 6, 6), [("rxT", "float32"), ("ryT", "float32"), ("rzT", "float32"), ("izT", "float32"),
                                         ("nux", "float32"), ("vx", "float32"), ("uy2", "float32"), ("vy", "float32")]),
    ("Resize3Plan", (3, 3, 3, 5, 5, 5), [("rxT", "float32"), ("ryT", "float32"), ("rzT", "float32"), ("izT", None), ("nux", None),
                                         ("vx", None), ("uy2", None), ("vy", None)]),
    # include/dpot_hip.h, dpot_eval_metrics_stats(pred, target, cxT, sxT, cy, sy, jlo, ...)
    ("EvalPlan", (4, 4), [("cxT", "float32"), ("sxT", "float32"), ("cy", "float32"), ("sy", "float32"), ("jlo", "int32")]),
    # dpot_eval3_stats(pred, target, cxT, sxT, cy, sy, czT, szT, jlo, ...)
    ("EvalPlan", (4, 4, 4), [("cxT", "float32"), ("sxT", "float32"), ("cy", "float32"), ("sy", "float32"), ("czT", "float32"),
                             ("szT", "float32"), ("jlo", "int32")]),
    ("AAPlan", (2, 2, 0, 0), [("tab", "int32"), ("vtab", None)]),
    ("AAPlan", (2, 2, 3, 3), [("tab", "int32"), ("vtab", "int32")]),
    ("FNOPlan", (4, 4, 1, 1), [("tx", "float64"), ("ty", "float64")]),
    ("FNOPlan", (4, 4, 4, 1, 1, 1), [("tx", "float64"), ("ty", "float64"), ("tz", "float64")]),
]
IDS = [f"{name}-{'x'.join(map(str, sizes))}" for name, sizes, _ in HOST]
ACCESSOR = {"ResizePlan": "resize_plan", "Resize3Plan": "resize3_plan", "EvalPlan": "eval_plan", "AAPlan": "aa_plan"}


def accessor(ops, name, sizes):
    return getattr(ops, ACCESSOR.get(name) or ("fno_plan" if len(sizes) == 4 else "fno3_plan"))


def host_tables(ops, name, sizes):
    """what the class hands the upload: its host hook"""
    return getattr(ops, name)._host(*sizes)


@pytest.mark.parametrize("name,sizes,want", HOST, ids=IDS)
def test_host_tables_keep_their_order_and_dtypes(name, sizes, want):
    from dpot_amd import ops
    h = host_tables(ops, name, sizes)
    assert [(k, None if a is None else str(a.dtype)) for k, a in h.items()] == want
    public = {"ResizePlan": "host_matrices", "Resize3Plan": "host_matrices", "EvalPlan": "host_tables"}.get(name)
    if public:                                               # the hook IS the public static method
        assert getattr(getattr(ops, name), public) is getattr(ops, name)._host


@pytest.mark.parametrize("name,sizes,want", HOST, ids=IDS)
def test_upload_and_cache_on_the_cpu_device(name, sizes, want, monkeypatch):
    """with the capture query stubbed to False: `dev` holds the host tables in their order, int32 as int32, everything else
    rounded once to fp32, None kept; the accessor returns one object for plain, numpy and torch.Size integers; with the query
    stubbed to True a new size refuses and leaves nothing behind, a cached one is returned"""
    from dpot_amd import _lib, ops
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    get = accessor(ops, name, sizes)
    plan = get(*sizes, "cpu")
    assert type(plan) is getattr(ops, name) and plan.sizes == sizes and all(type(n) is int for n in plan.sizes)
    h = host_tables(ops, name, sizes)
    assert list(plan.dev) == [k for k, _ in want]
    for (key, dtype), a, t in zip(want, h.values(), plan.dev.values()):
        if dtype is None:
            assert a is None and t is None, key
            continue
        assert t.dtype == (torch.int32 if dtype == "int32" else torch.float32) and t.device.type == "cpu", key
        assert np.array_equal(t.numpy(), a if dtype == "int32" else a.astype(np.float32)), key
    assert get(*sizes, torch.device("cpu")) is plan
    assert get(*(np.int64(n) for n in sizes), "cpu") is plan and get(*torch.Size(sizes), "cpu") is plan
    if name == "FNOPlan":
        assert plan.tables == list(plan.dev.values()) and plan.tx is plan.dev["tx"] and hasattr(plan, "tz") == (len(sizes) == 6)
    if name == "AAPlan":
        assert plan.tab is plan.dev["tab"] and plan.vtab is plan.dev["vtab"]
    new = tuple(n + 1 if n else 0 for n in sizes[:-1]) + sizes[-1:]          # another admissible tuple, not yet built
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
    with pytest.raises(_lib.DpotHipError, match="before capturing"):
        get(*new, "cpu")
    assert get(*sizes, "cpu") is plan
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", lambda: False)
    assert get(*new, "cpu").sizes == new                     # the refused build left no entry behind


def test_refusals_come_before_the_capture_query_and_any_allocation(monkeypatch):
    """every refusal the CPU tests of the operators reach on the "cpu" device, with its present type - and none of them gets as
    far as asking for the capture state"""
    from dpot_amd import _lib, ops

    def asked():
        raise AssertionError("a refused plan asked for the capture state")
    monkeypatch.setattr(torch.cuda, "is_current_stream_capturing", asked)
    with pytest.raises(_lib.DpotHipError, match=">= 2"):
        ops.resize3_plan(8, 8, 1, 8, 8, 8, "cpu")
    cap = _lib.load().dpot_spectral_resize3_max_size()
    with pytest.raises(_lib.DpotHipError, match=str(cap + 1)):
        ops.resize3_plan(8, 8, 8, 8, cap + 1, 8, "cpu")
    with pytest.raises(ValueError, match="512x64"):
        ops.FNOPlan(512, 64, 8, 8, "cpu")
    with pytest.raises(ValueError, match="would overlap"):
        ops.fno_plan(8, 8, 5, 2, "cpu")
    n = _lib.load().dpot_fno3_max_size(0)
    with pytest.raises(ValueError, match=f"{2 * n}x64x64"):
        ops.FNO3Plan(2 * n, 64, 64, 8, 8, 8, "cpu")
    with pytest.raises(ValueError, match="need the 2 or 3 spatial sizes"):
        ops.eval_plan(8, "cpu")
    big = _lib.load().dpot_eval_metrics_max_size(0) + 1
    with pytest.raises(_lib.DpotHipError, match="beyond the supported size"):
        ops.eval_plan(big, 8, "cpu")
    with pytest.raises(ValueError, match="latent size 0x4"):
        ops.aa_plan(0, 4, 0, 0, "cpu")
    with pytest.raises(ValueError, match="output size 3x8"):
        ops.aa_plan(4, 4, 3, 8, "cpu")


def test_size_tuple_and_the_callers_that_word_its_refusal():
    from dpot_amd import infer, ops
    assert ops.size_tuple(5, 3) == (5, 5, 5) and ops.size_tuple([np.int64(4), 6], 2) == (4, 6)
    assert ops.size_tuple(torch.Size((4, 6, 8)), 2) == (4, 6)               # the 2-D callers have always read the first two
    assert ops.size_tuple((4, 6), 3, strict=True) is None and ops.size_tuple((4, 6, 8), 3, strict=True) == (4, 6, 8)
    assert infer._size2(7) == (7, 7) and infer.Resized3D(torch.nn.Identity(), 8).model_res == (8, 8, 8)
    with pytest.raises(ValueError, match="model_res"):
        infer.Resized3D(torch.nn.Identity(), (8, 8))
