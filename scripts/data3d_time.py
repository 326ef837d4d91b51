#!/usr/bin/env python
"""Time the 3-D input pipeline (csrc/data3d.hip: dpot_resize_pad_window3, data.DeviceBatcher3D) against the same transform
composed from torch ops on the device.

    python scripts/data3d_time.py [--reps 10] [--batches 6] [--kernel-only] [--out profiles/data3d.txt]

Batches of raw trajectories as the reference's 3-D datasets store them (utils/make_master_file.py:204-241):
[4 x (64,64,64,21,5)] and [2 x (128,128,128,21,5)], both to 64^3 with t_in 10, t_ar 1, n_channels 5, random window starts.
Yardstick, kept here: per sample, the window's frames as [1, T*C, H, W, L] (a permuted view), F.interpolate(mode='trilinear'),
permute back, a ones-filled [res,res,res,T,n_channels] block with the data copied in, and the two slices copied into xx / yy -
the reference's pad_data + window restricted to the frames that are used.
Per kernel: a hipGraph of `reps` launches between two events, median of 5 replays; microseconds, yardstick over ours, the
algorithmic bytes (the window of every raw sample read once, xx and yy written once) and the same number of bytes moved by a
plain device copy IN THE SAME RUN: 'of copy rate' is the copy's time over the kernel's.
Batcher: `batches` batches from host arrays through submit / get / release with the next submit in flight, host clock around
the loop ending in a device synchronise; per batch the wall time, the host time inside submit() (the strided copy of the
window's frames into the pinned staging buffer, everything else there is asynchronous) and the bytes sent."""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import _lib  # noqa: E402
from dpot_amd.data import DESC_BYTES, DeviceBatcher3D, _fill_table, staged_floats  # noqa: E402

CASES = [(4, (64, 64, 64, 21, 5)), (2, (128, 128, 128, 21, 5))]
RES, T_IN, T_AR, NC = 64, 10, 1, 5


def median5(run, reps):
    out = []
    for _ in range(5):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        run()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) * 1e3 / reps)
    return sorted(out)[2]


def time_graph(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    t = median5(g.replay, reps)
    del g
    return t


def composed(samples, starts, xx, yy):
    """the transform from torch ops, written into xx / yy"""
    win = T_IN + T_AR
    for b, (s, t0) in enumerate(zip(samples, starts)):
        H, W, L, _, C = s.shape
        w = s[..., t0:t0 + win, :].reshape(H, W, L, win * C).permute(3, 0, 1, 2).unsqueeze(0)
        w = F.interpolate(w, size=(RES, RES, RES), mode="trilinear").squeeze(0).permute(1, 2, 3, 0)
        out = torch.ones(RES, RES, RES, win, NC, device=s.device)
        out[..., :C] = w.reshape(RES, RES, RES, win, C)
        xx[b].copy_(out[..., :T_IN, :])
        yy[b].copy_(out[..., T_IN:, :])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batches", type=int, default=6)
    ap.add_argument("--kernel-only", action="store_true", help="skip the DeviceBatcher3D part")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "data3d.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("data3d_time: needs the GPU (nothing is measured without one)")
    dev, reps = "cuda", args.reps
    lib = _lib.load()
    lines = [f"device: {torch.cuda.get_device_name(0)}   reps {reps}, median of 5   raw [B x (H,W,L,T,C)] -> {RES}^3, "
             f"t_in {T_IN}, t_ar {T_AR}, n_channels {NC}"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:                     # the record as far as the run got
            f.write("\n".join(lines) + "\n")

    big = torch.empty(1 << 28, device=dev)
    big2 = torch.empty_like(big)
    rate = 2.0 * big.numel() * 4 / (time_graph(lambda: big2.copy_(big), 10) * 1e-6)
    emit(f"measured copy rate (1 GiB read + 1 GiB write): {rate / 1e12:.2f} TB/s")
    del big, big2
    emit(f"{'batch':28s} {'kernel us':>10s} {'torch us':>10s} {'torch/kernel':>12s} {'MB moved':>9s} {'same-bytes copy us':>18s} "
         f"{'of copy rate':>12s} {'TB/s':>6s}")
    win = T_IN + T_AR
    for B, shape in CASES:
        torch.manual_seed(0)
        rng = np.random.default_rng(0)
        samples = [torch.randn(*shape, device=dev) for _ in range(B)]
        starts = [int(rng.integers(shape[3] - win + 1)) for _ in range(B)]
        host = np.zeros(B * DESC_BYTES, dtype=np.uint8)
        _fill_table(host, [s.data_ptr() for s in samples], [shape] * B, starts, T_IN, T_AR, NC, _lib.Sample3Desc)
        table = torch.from_numpy(host).to(dev)
        xx = torch.empty(B, RES, RES, RES, T_IN, NC, device=dev)
        yy = torch.empty(B, RES, RES, RES, T_AR, NC, device=dev)
        xr, yr = torch.empty_like(xx), torch.empty_like(yy)

        def ours():
            _lib.check(lib.dpot_resize_pad_window3(table.data_ptr(), B, xx.data_ptr(), yy.data_ptr(), RES, T_IN, T_AR, NC,
                                                   1, 1, 1, torch.cuda.current_stream().cuda_stream), "resize_pad_window3")

        ours()
        composed(samples, starts, xr, yr)
        for got, ref, what in ((xx, xr, "xx"), (yy, yr, "yy")):
            err = (got - ref).abs().max().item()
            assert err <= 1e-5 * ref.abs().max().item(), f"{what}: kernel and torch composition differ by {err}"
        nbytes = 4.0 * (B * shape[0] * shape[1] * shape[2] * win * shape[4] + xx.numel() + yy.numel())
        a = torch.empty(int(nbytes / 8), device=dev)
        c = torch.empty_like(a)
        tk = time_graph(ours, reps)
        tc = time_graph(lambda: c.copy_(a), reps)
        ty = time_graph(lambda: composed(samples, starts, xr, yr), max(2, reps // 5))
        emit(f"{f'[{B} x {shape}]':28s} {tk:10.1f} {ty:10.1f} {ty / tk:12.2f} {nbytes / 1e6:9.1f} {tc:18.1f} {tc / tk:12.3f} "
             f"{nbytes / (tk * 1e-6) / 1e12:6.2f}")
        del samples, xx, yy, xr, yr, a, c, table
        torch.cuda.empty_cache()

    if args.kernel_only:
        return
    emit("--- DeviceBatcher3D, end to end from host arrays (window-only staging, one H2D copy, the kernel; next submit in flight)")
    emit(f"{'batch':28s} {'wall ms/batch':>13s} {'submit() host ms':>16s} {'MB sent/batch':>13s} {'of the raw MB':>13s}")
    for B, shape in CASES:
        raw = np.random.default_rng(1).standard_normal(shape, dtype=np.float32)        # one trajectory, B times in a batch
        db = DeviceBatcher3D(B, RES, T_IN, T_AR, NC, max_raw_floats_per_sample=staged_floats(shape, T_IN, T_AR))
        starts = [[(3 * i + b) % (shape[3] - win + 1) for b in range(B)] for i in range(args.batches + 2)]
        for i in range(2):                                 # warm-up: both slots
            db.submit([raw] * B, starts[i])
            db.get()
            db.release()
        torch.cuda.synchronize()
        sink = torch.zeros((), device=dev)
        host_s = 0.0
        t0 = time.perf_counter()
        db.submit([raw] * B, starts[2])
        for i in range(args.batches):
            if i + 1 < args.batches:
                h0 = time.perf_counter()
                db.submit([raw] * B, starts[3 + i])
                host_s += time.perf_counter() - h0
            x, y, _ = db.get()
            sink += x[0, 0, 0, 0, 0, 0] + y[0, 0, 0, 0, 0, 0]          # "the step": a reader on the compute stream
            db.release()
        torch.cuda.synchronize()
        wall = (time.perf_counter() - t0) / args.batches
        sent = 4.0 * B * staged_floats(shape, T_IN, T_AR)
        emit(f"{f'[{B} x {shape}]':28s} {wall * 1e3:13.2f} {host_s / max(1, args.batches - 1) * 1e3:16.2f} {sent / 1e6:13.1f} "
             f"{sent / (4.0 * B * np.prod(shape)):13.3f}")
        del db
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
