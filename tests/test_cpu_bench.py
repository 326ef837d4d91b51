"""bench.py options on the host: a plain run measures only the headline (`--full` off by default) and `--dump-outputs`
writes the last step's arrays as fp32 .npy files, large ones as the same seeded sample every time, under 64 MB in all."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import bench  # noqa: E402


def test_plain_run_is_default(monkeypatch):
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "7", "--warmup", "2"])
    a = bench.parse()
    assert (a.steps, a.warmup, a.full, a.dump_outputs) == (7, 2, False, None)
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--dump-outputs", "out"])
    a = bench.parse()
    assert a.full and a.dump_outputs == "out"


class _Flat:
    def __init__(self, n):
        self.flat = torch.arange(n, dtype=torch.float32) * 0.5


class _Opt:
    def __init__(self, n):
        self.fp = _Flat(n)

    def grad_norm(self, grad_scale=1.0):
        return torch.tensor([2.0]) * grad_scale


def test_dump_outputs_fp32_seeded_sample_and_size(tmp_path):
    n = bench.DUMP_MAX_PARAMS + 12345
    pred = torch.randn(2, 8, 8, 1, 4)
    for d in ("a", "b"):
        bench.dump_outputs(str(tmp_path / d), torch.tensor(1.25), pred, _Opt(n), 1.0)
    names = sorted(os.listdir(tmp_path / "a"))
    assert names == ["grad_norm.npy", "loss.npy", "params.npy", "pred.npy"]
    for f in names:
        x, y = np.load(tmp_path / "a" / f), np.load(tmp_path / "b" / f)
        assert x.dtype == np.float32
        assert np.array_equal(x, y)                      # the same sample in every run
    assert np.load(tmp_path / "a" / "loss.npy") == np.float32(1.25)
    assert np.array_equal(np.load(tmp_path / "a" / "pred.npy"), pred.numpy())
    p = np.load(tmp_path / "a" / "params.npy")
    assert p.shape == (bench.DUMP_MAX_PARAMS,)
    assert np.all(np.diff(p) > 0) and p[-1] <= (n - 1) * 0.5   # ascending indices, values of the array itself
    assert (bench.DUMP_MAX_PRED + bench.DUMP_MAX_PARAMS) * 4 < 64 * 2 ** 20
