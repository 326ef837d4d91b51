"""CPU-side checks of the training metrics and the dataset-classification loss: the new C-ABI symbols and struct layouts,
StepMetrics.read() normalisations against hand-computed dicts, the refusal of CPU tensors, the cls_weight / update_tail
error, and read(group) summing over two gloo ranks with one collective."""
import ctypes
import math
import os
import socket
import subprocess
import sys
import tempfile

import pytest
import torch

from oracle import dpot_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("dpot_cls_ce_fwd", "dpot_cls_ce_bwd", "dpot_rel_l2_combine", "dpot_metrics_accum")


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


def test_new_symbols_in_header_table_and_library(built_lib):
    from dpot_amd import _lib
    hdr = open(os.path.join(ROOT, "include", "dpot_hip.h")).read()
    exported = subprocess.check_output(["nm", "-D", "--defined-only", built_lib], text=True)
    for name in NEW:
        assert f"int {name}(" in hdr, name
        assert name in _lib.SIGNATURES, name
        assert f" T {name}\n" in exported, name
    assert "metrics.hip" in __import__("dpot_amd.build", fromlist=["SOURCES"]).SOURCES
    assert _lib.load().dpot_version() >= 263


def test_struct_layouts_match_the_word_views(built_lib):
    """ops addresses dpot_cls_ce_out as 4 and dpot_metrics as 12 eight-byte words (4 doubles, then the int64 counters in
    METRICS_INTS order): compare with the C structs compiled by the host compiler"""
    from dpot_amd import ops
    fields = ["l2_step", "l2_full", "cls_loss", "grad_norm"] + list(ops.METRICS_INTS) + ["reserved"]
    src = '#include <stdio.h>\n#include <stddef.h>\n#include "dpot_hip.h"\nint main(){printf("%zu %zu %zu %zu %zu",' \
          'sizeof(dpot_cls_ce_out),offsetof(dpot_cls_ce_out,loss),offsetof(dpot_cls_ce_out,correct),' \
          'offsetof(dpot_cls_ce_out,valid),offsetof(dpot_cls_ce_out,invalid));printf(" %zu",sizeof(dpot_metrics));' \
          + "".join(f'printf(" %zu",offsetof(dpot_metrics,{f}));' for f in fields) + 'return 0;}\n'
    with tempfile.TemporaryDirectory() as td:
        c = os.path.join(td, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(td, "t")
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), c, "-o", exe])
        got = [int(v) for v in subprocess.check_output([exe]).split()]
    assert got[:5] == [8 * ops.CLS_OUT_WORDS, 0, 8, 16, 24]
    assert got[5] == 8 * ops.METRICS_WORDS
    assert got[6:] == [8 * i for i in range(ops.METRICS_WORDS)]
    assert tuple(fields[:4]) == ops.METRICS_FLOATS and ctypes.sizeof(ctypes.c_double) == 8


def _fill(m, row, floats, ints):
    from dpot_amd import ops
    m.acc[row, :4] = torch.tensor(floats, dtype=torch.float64).view(torch.int64)
    m.acc[row, 4:4 + len(ops.METRICS_INTS)] = torch.tensor(ints, dtype=torch.int64)


def test_read_normalisations_against_hand_computed_dict():
    """5 optimiser steps of batch 8 with 3 AR steps each: the reference divides train_l2_step by ntrain and by the AR steps
    per sample (train_temporal.py:232), train_l2_full by ntrain (:233); accuracy = cls_correct / cls_total"""
    from dpot_amd import StepMetrics
    m = StepMetrics("cpu", 3)
    #            l2_step l2_full cls_loss grad_norm | correct total invalid samples ar_steps opt_steps nonfinite
    _fill(m, 0, [60.0, 30.0, 240.0, 12.5], [90, 118, 2, 40, 15, 5, 1])
    d = m.read()
    assert d["l2_step"] == 60.0 and d["l2_full"] == 30.0 and d["cls_loss"] == 240.0 and d["grad_norm"] == 12.5
    assert (d["cls_correct"], d["cls_total"], d["cls_invalid"]) == (90, 118, 2)
    assert (d["samples"], d["ar_steps"], d["opt_steps"], d["nonfinite_steps"]) == (40, 15, 5, 1)
    assert all(isinstance(d[k], int) for k in ("cls_correct", "samples", "opt_steps"))
    assert d["ar_steps_per_sample"] == 3.0
    assert d["train_l2_step_avg"] == 60.0 / 40 / 3 and d["train_l2_full_avg"] == 30.0 / 40
    assert d["test_l2_step_avg"] == d["train_l2_step_avg"] and d["test_l2_full_avg"] == d["train_l2_full_avg"]
    assert d["cls_acc"] == 90 / 118 and d["cls_loss_avg"] == 240.0 / 118 and d["grad_norm_avg"] == 2.5
    # last(): the second struct, as views (no copy)
    _fill(m, 1, [1.5, 0.5, 7.0, 2.0], [3, 8, 0, 8, 3, 1, 0])
    last = m.last()
    assert float(last["l2_step"]) == 1.5 and float(last["grad_norm"]) == 2.0 and int(last["cls_total"]) == 8
    assert last["l2_full"].data_ptr() == m.acc[1, 1:2].data_ptr()
    # reset() zeroes the accumulator; an empty one divides by nothing
    m.reset()
    e = m.read()
    assert e["samples"] == 0 and e["l2_step"] == 0.0 and math.isnan(e["train_l2_step_avg"]) and math.isnan(e["cls_acc"])
    with pytest.raises(ValueError):
        StepMetrics("cpu", 0)
    with pytest.raises(ValueError, match="AR steps"):
        m._check_steps(4)


def test_cpu_tensors_raise(built_lib):
    """no CPU fallback in the product path: the loss, the combine and the accumulate refuse CPU tensors"""
    from dpot_amd import StepMetrics, cls_ce_loss, ops
    from dpot_amd._lib import DpotHipError
    with pytest.raises(DpotHipError, match="no CPU path"):
        cls_ce_loss(torch.randn(4, 5), torch.zeros(4, dtype=torch.int64))
    with pytest.raises(DpotHipError, match="no CPU path"):
        ops.rel_l2_combine(torch.zeros(2, 64), 2, 4)
    m = StepMetrics("cpu", 1)
    m._pending = (torch.zeros(1), 1, 2, 0)
    with pytest.raises(DpotHipError, match="no CPU path"):
        m.accumulate()
    with pytest.raises(RuntimeError, match="no rollout"):
        m.accumulate()


def test_cls_weight_needs_labels_and_update_tail():
    """a weighted classification loss with an optimiser that skips cls_head would silently freeze the head: it raises"""
    from dpot_amd import DPOTNet
    from dpot_amd.train import FlatParams, FusedAdam, FusedLamb, check_cls_args, rollout, train_step
    model = DPOTNet(**R.MINI)
    fp = FlatParams(model)
    frozen, moving = FusedAdam(fp, update_tail=False), FusedLamb(fp, update_tail=True)
    cls = torch.zeros(2, 1, dtype=torch.int64)
    xx = torch.zeros(2, 32, 32, 4, 3)
    with pytest.raises(ValueError, match="update_tail=True"):
        train_step(model, frozen, xx, xx[..., :1, :], None, cls=cls, cls_weight=1.0)
    with pytest.raises(ValueError, match="needs the dataset labels"):
        train_step(model, moving, xx, xx[..., :1, :], None, cls=None, cls_weight=0.5)
    with pytest.raises(ValueError, match="needs the dataset labels"):
        rollout(model, xx, xx[..., :1, :], None, cls_weight=1.0)
    check_cls_args(moving, cls, 1.0)            # fine
    check_cls_args(frozen, cls, 0.0)            # an observer needs no tail update
    check_cls_args(frozen, None, 0.0)


# ---- read(group): two gloo ranks -------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    import torch.distributed as dist
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dpot_amd import StepMetrics
    m = StepMetrics("cpu", 2)
    _fill(m, 0, [1.0 + rank, 2.0 * (rank + 1), 0.25, 3.0], [5 + rank, 8, rank, 8, 16, 8, 0])
    calls = []
    real = dist.all_reduce

    def counting(*a, **kw):
        calls.append(1)
        return real(*a, **kw)

    dist.all_reduce = counting
    try:
        local, summed = m.read(), m.read(dist.group.WORLD)
    finally:
        dist.all_reduce = real
    assert len(calls) == 1                       # ONE collective, at read time
    assert local["l2_step"] == 1.0 + rank and local["samples"] == 8
    torch.save(summed, os.path.join(out_dir, f"r{rank}.pt"))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.timeout(300)
def test_read_group_sums_over_two_gloo_ranks(tmp_path):
    import torch.multiprocessing as mp
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    a, b = (torch.load(os.path.join(str(tmp_path), f"r{r}.pt")) for r in (0, 1))
    assert a == b
    assert a["l2_step"] == 3.0 and a["l2_full"] == 6.0 and a["cls_loss"] == 0.5 and a["grad_norm"] == 6.0
    assert (a["cls_correct"], a["cls_total"], a["cls_invalid"], a["samples"], a["ar_steps"], a["opt_steps"]) == \
        (11, 16, 1, 16, 32, 16)
    assert a["train_l2_step_avg"] == 3.0 / 16 / 2 and a["cls_acc"] == 11 / 16
