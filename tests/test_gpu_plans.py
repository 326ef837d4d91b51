"""GPU tests of the one cache and the one capture guard behind the six plan accessors (ops._plan, ops._TablePlan): one object
per (sizes, device) however the device and the integers are spelled, and a refusal to build under capture that leaves no cache
entry behind.  The capture state is stubbed: no test starts a real capture to provoke the error."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

# accessor, the smallest sizes its checks admit, and a second admissible tuple that no other test of the suite builds
CASES = [
    ("resize_plan", (4, 4, 6, 6), (4, 5, 6, 7)),
    ("resize3_plan", (4, 4, 4, 6, 6, 6), (4, 5, 4, 6, 6, 7)),
    ("eval_plan", (4, 4), (4, 5)),
    ("eval_plan", (4, 4, 4), (4, 5, 4)),
    ("aa_plan", (2, 2, 0, 0), (2, 3, 0, 0)),
    ("aa_plan", (2, 2, 3, 3), (2, 3, 3, 4)),
    ("fno_plan", (4, 4, 1, 1), (4, 5, 1, 2)),
    ("fno3_plan", (4, 4, 4, 1, 1, 1), (4, 5, 4, 1, 1, 2)),
]


@pytest.mark.parametrize("name,sizes,unseen", CASES, ids=[f"{n}-{'x'.join(map(str, s))}" for n, s, _ in CASES])
def test_one_plan_per_sizes_and_device_and_none_built_under_capture(name, sizes, unseen, monkeypatch):
    from dpot_amd import _lib, ops
    get = getattr(ops, name)
    plan = get(*sizes, "cuda")
    assert get(*sizes, "cuda") is plan
    here = torch.device("cuda", torch.cuda.current_device())
    assert get(*sizes, torch.device("cuda")) is plan and get(*sizes, here) is plan
    assert get(*(np.int64(n) for n in sizes), "cuda") is plan and get(*torch.Size(sizes), here) is plan
    assert plan.sizes == sizes and all(t is None or t.device == here for t in plan.dev.values())
    with monkeypatch.context() as mp:
        mp.setattr(torch.cuda, "is_current_stream_capturing", lambda: True)
        with pytest.raises(_lib.DpotHipError, match="before capturing"):
            get(*unseen, "cuda")
        assert get(*sizes, "cuda") is plan                   # a size seen before needs no upload: returned
    late = get(*unseen, "cuda")                              # the refused build left nothing in the cache
    assert late.sizes == unseen and get(*unseen, here) is late
