#!/usr/bin/env python
"""bench.py - PDE samples/s of one DPOT auto-regressive training step (128^2 x 10 -> 1), DPOT-Tiny, on N MI355X.

    python bench.py --gpus 1 --steps 20 --warmup 5
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
           bench.py --gpus N --steps K --warmup W

A step = forward + masked relative-L2 loss + backward (+ RCCL gradient all-reduce) + global-norm clip + fused Adam,
T_ar = 1, on BASELINE.json configs[1]: DPOT-Tiny (embed 512, depth 4, 4 blocks, modes 32, patch 8), per-GPU batch 32,
fp32, synthetic N(0,1) fields already resident in HBM.  Weak scaling: every rank processes its own batch of 32.
Rank 0 prints ONE JSON line (metric / value / unit / ms_per_step / dtype + the run's configuration).

A plain run only sets up, warms up, times the `--steps` steps and prints that line.  `--full` adds everything else this
script measures, each in runs of its own: the sustained rate, the `roofline` of the dominant kernels, the other GEMM
precisions, inference, the input-pipeline-inclusive rate, `cpu_baseline` and BASELINE configs[2..4] as `other_configs`.
`--dump-outputs DIR` writes what the last timed step computed (loss, prediction, gradient norm, updated parameters) as
DIR/<name>.npy, fp32; the inputs and the initial weights are seeded, so two builds run with the same arguments can be
compared output for output.

`--gpus N` without a launcher (WORLD_SIZE unset) re-executes itself under torch.distributed.run on 127.0.0.1.
`--config {T,S,M,L,L20}` selects the other BASELINE.json configs (default T = configs[1], the headline):
S = configs[2] (DPOT-Small, bf16 channel-MLP), M = configs[3] (DPOT-Medium, 32 per GPU = 256 global on 8 GPUs, bf16
channel-MLP), L = DPOT-Large at 256^2 (T_ar = 1), L20 = configs[4] (DPOT-Large, 20-step auto-regressive rollout with
activation recomputation, per-GPU batch 16 = the largest power of two that fits; value = sample-steps/s).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch
import torch.distributed as dist

TINY = dict(img_size=128, patch_size=8, in_channels=4, out_channels=4, in_timesteps=10, out_timesteps=1, n_blocks=4,
            embed_dim=512, out_layer_dim=32, depth=4, modes=32, mlp_ratio=1, n_cls=12)
SMALL = dict(TINY, embed_dim=1024, depth=6, n_blocks=8)
MEDIUM = dict(TINY, embed_dim=1024, depth=12, n_blocks=8, mlp_ratio=4)
LARGE = dict(TINY, img_size=256, embed_dim=1536, depth=24, n_blocks=16, mlp_ratio=4, out_layer_dim=128, modes=64)
# name, model kwargs, per-GPU batch, T_ar, channel-MLP precision, activation recomputation, BASELINE.json entry
CONFIGS = {
    "T": ("DPOT-Tiny", TINY, 32, 1, None, False, "configs[1]"),
    "S": ("DPOT-Small", SMALL, 32, 1, "bf16", False, "configs[2]"),
    "M": ("DPOT-Medium", MEDIUM, 32, 1, "bf16", False, "configs[3]"),
    "L": ("DPOT-Large", LARGE, 16, 1, "bf16", False, "configs[4] model, one rollout step"),
    "L20": ("DPOT-Large", LARGE, 16, 20, "bf16", True, "configs[4]"),
}
# how the fp32 GEMMs OUTSIDE the channel MLP form their products: the headline (T) is native fp32 MFMA everywhere; the
# bf16-channel-MLP configs run `auto` - native fp32 MFMA below 3 GFLOP, the fp32-ACCURATE bf16x6 operand split above (de-embed
# GEMMs, embed fold: same accuracy class as native fp32, DESIGN.md "GEMM precision modes"; parity at these sizes incl. the
# DPOT-L batch-16 reference golden at rtol 1e-4 runs under it in tests/test_gpu_optout.py) - and report the all-native figure
# beside it (`gemm_f32`)
CONFIG_GEMM = {"T": "f32", "S": "auto", "M": "auto", "L": "auto", "L20": "auto"}
FP32_MFMA_PEAK_TFLOPS = 157.3      # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32, dense
BF16_MFMA_PEAK_TFLOPS = 2500.0     # MI355X_MICROARCH.md: dense bf16 MFMA
SUSTAINED_FP32_MFMA_TFLOPS = 132.8   # register-only MFMA loop, random operands (profiles/r02_mfma_f32_peak.txt)
HBM_PEAK_GBS = 8000.0              # MI355X_MICROARCH.md: HBM3E spec
# --dump-outputs: at most this many fp32 elements of the prediction / of the parameters (24 + 32 MB, < 64 MB in all; the
# DPOT-Tiny parameters, 7.5 M, are written whole)
DUMP_MAX_PRED, DUMP_MAX_PARAMS = 6 << 20, 8 << 20


def log(*a):
    print(*a, file=sys.stderr, flush=True)


def parse():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="T", choices=tuple(CONFIGS),
                    help="T (default, the headline: BASELINE configs[1]) | S | M | L | L20 - see the module docstring")
    ap.add_argument("--batch", type=int, default=None, help="per-GPU batch (default: the config's; T/S/M 32, L / L20 16)")
    ap.add_argument("--mlp-precision", default=None, choices=("f32", "bf16x6", "auto", "bf16"),
                    help="channel-MLP GEMM precision (default: the config's - f32 for T, bf16 for S/M/L/L20)")
    ap.add_argument("--no-graph", action="store_true", help="eager launches instead of hipGraph replay")
    ap.add_argument("--overlap", action="store_true",
                    help="N>1: EAGER step with the bucketed all-reduce driven by the backward's gradient-ready "
                         "notifications (default for N>1: the bucket-segmented hipGraph chain, which overlaps the same "
                         "all-reduces with the replayed backward segments)")
    ap.add_argument("--no-overlap", action="store_true",
                    help="N>1: one graph of fwd+bwd, then all buckets, then Adam (round-1 behaviour, for comparison)")
    ap.add_argument("--sustain-seconds", type=float, default=2.0,
                    help="--full, N=1: also time a sustained run of about this many seconds of replays (DVFS-honest)")
    ap.add_argument("--noise-scale", type=float, default=0.0005,
                    help="train_temporal.py:205 noise injection (configs/pretrain_tiny.yaml:71 uses 0.0005)")
    ap.add_argument("--skip-cpu-baseline", action="store_true")
    ap.add_argument("--no-pipeline", action="store_true", help="--full: skip the input-pipeline-inclusive timing")
    ap.add_argument("--gemm-precision", default=os.environ.get("DPOT_GEMM_PRECISION"),
                    choices=("f32", "bf16x6", "auto"),
                    help="how the fp32 GEMMs form their products (default: f32 = native fp32 MFMA for the headline config T, "
                         "auto for S / M / L / L20 - see CONFIG_GEMM)")
    ap.add_argument("--no-alt", action="store_true", help="--full: skip the extra timings at the other GEMM precisions")
    ap.add_argument("--cpu-seconds", type=float, default=15.0)
    ap.add_argument("--no-other-configs", action="store_true",
                    help="--full run (config T, N=1): do NOT append BASELINE configs[2..4] (S, M, L at batch 16, L20) as "
                         "`other_configs` (each is one short child run of this script)")
    ap.add_argument("--full-json", default=None, help="also write the VERBOSE record (every note / description) to this file")
    ap.add_argument("--brief", action="store_true",
                    help="with --full: only the step timing and the dominant-kernel roofline (what the `other_configs` "
                         "children run)")
    ap.add_argument("--full", action="store_true",
                    help="also run every measurement beyond the headline step timing (sustained rate, rooflines, other "
                         "precisions, inference, input pipeline, CPU baseline, other configs); off by default")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write what the last timed step computed as DIR/<name>.npy (fp32; a larger prediction or "
                         "parameter vector than DUMP_MAX_PRED / DUMP_MAX_PARAMS elements as a fixed, seeded sample)")
    return ap.parse_args()


# ------------------------------------------------------------------------------------------------------
def step_flops_per_sample(kw: dict, B: int, three_product: bool = True):
    """(algorithmic, executed) FLOP of ONE train step (fwd + bwd) per sample.  Algorithmic = 3 x the forward of the model
    as the reference computes it (SURVEY 8d accounting: 3.79 GFLOP forward at DPOT-Tiny).  Executed = what the kernels of
    this build run: the 1x1 conv of the patch embed folded into the time aggregation (K = T*hid_p instead of T*E), the
    three unit-grid channels folded into a bias table, Gauss's three-product complex multiply in the mixer data path
    (forward and data gradient; the weight gradients run four products), no input gradient for the patch conv, and the
    weight-only products (embed fold) once per step, i.e. divided by the batch."""
    E, depth, nb, P = kw["embed_dim"], kw["depth"], kw["n_blocks"], kw["patch_size"]
    T, C, Co = kw["in_timesteps"], kw["in_channels"], kw["out_channels"] * kw["out_timesteps"]
    h = kw["img_size"] // P
    tok, wf = h * h, h // 2 + 1
    mx, my = min(kw["modes"], h), min(kw["modes"], wf)
    bs, mh, old = E // nb, int(E * kw["mlp_ratio"]), kw["out_layer_dim"]
    hid = kw["out_channels"] * P + 3
    hidp = (hid + 3) // 4 * 4
    npx = tok * P * P
    # --- algorithmic forward (reference formulation)
    a_patch = 2.0 * tok * T * ((C + 3) * P * P * hid + hid * E)
    a_tagg = 2.0 * tok * T * E * E
    a_mix = depth * mx * my * nb * 2 * 4 * 2.0 * bs * bs
    a_fft = depth * 2 * 5.0 * tok * E * max(1.0, __import__("math").log2(tok)) / 2
    a_mlp = depth * 2 * 2.0 * tok * E * mh
    a_head = 2.0 * tok * E * P * P * old + 2.0 * npx * (old * old + old * Co)
    alg = 3.0 * (a_patch + a_tagg + a_mix + a_fft + a_mlp + a_head)
    # --- executed (this build), forward / backward listed separately
    e_patch_f = 2.0 * tok * T * (C * P * P) * hidp                      # implicit GEMM over the data channels only
    e_fold_f = 2.0 * tok * (T * hidp) * E
    e_mix_f = depth * mx * my * nb * 2 * (3 if three_product else 4) * 2.0 * bs * bs
    e_fwd = e_patch_f + e_fold_f + e_mix_f + a_fft + a_mlp + a_head
    e_bwd = (e_patch_f                                                # patch conv: weight gradient only
             + 2 * e_fold_f + e_mix_f + a_mix                         # mixer: 3-product data path + 4-product wgrad
             + a_fft + 2 * a_mlp + 2 * a_head)
    w_only = 3.0 * 2.0 * T * hidp * E * E + 3.0 * 2.0 * tok * E * E  # V = w2^T ws_t (T products) and c = posb wsum, + bwd
    # executed FLOPs that go through the generic GEMM entry (dpot_gemm_*: the fold of the patch conv's 1x1 into the time
    # aggregation and the de-embed ConvTranspose-as-GEMM, forward + data + weight gradient) - under gemm_precision `auto` a
    # launch of >= 3 GFLOP runs as the fp32-accurate bf16x6 split on the bf16 pipes (6 bf16 products per fp32 product)
    g_fold, g_head = 3.0 * e_fold_f, 3.0 * 2.0 * tok * E * P * P * old
    x6 = (g_fold if e_fold_f * B >= 3e9 else 0.0) + (g_head if 2.0 * tok * E * P * P * old * B >= 3e9 else 0.0)
    return alg, e_fwd + e_bwd + w_only / B, 3.0 * a_mlp, x6


def mixer_roofline(model, B: int):
    """Time the AFNO mixer kernel - both layers of the block-diagonal complex MLP, one launch of
    dpot::afno_mlp2_kernel (csrc/afno_mlp.hip) - with HIP events on the launch stream, in the form the train step runs
    (pre-activation and activated spectrum also stored for the backward), on a real-sized spectrum and random data."""
    from dpot_amd import ops
    E, nb, h = model.embed_dim, model.n_blocks, model.latent_size[0]
    bs = E // nb
    N = 2 * bs
    mx, my = min(model.modes, h), min(model.modes, h // 2 + 1)
    Mm = B * mx * my
    fused = ops.afno_mlp2_supported(nb, bs)
    with torch.no_grad():
        S = torch.randn(Mm, 2 * E, device="cuda")
        W1 = torch.randn(nb, N, N, device="cuda") * 0.05          # random data, not the near-zero init (DVFS-honest)
        W2 = torch.randn(nb, N, N, device="cuda") * 0.05
        b1 = torch.randn(nb, N, device="cuda") * 0.1
        b2 = torch.randn(nb, N, device="cuda") * 0.1

        three = fused and ops.afno_mlp3_supported(nb, bs)
        # round 6: under gemm_precision 'auto' / 'bf16x6' the model runs the mixer MLP as bf16x6 on the bf16 matrix cores where
        # that measured faster (csrc/afno_mlp6.hip, 96 channels per block: DPOT-L) - time what the model runs
        six = False
        if fused and getattr(model, "gemm_precision", None) in ("auto", "bf16x6"):
            with ops.precision_scope(model.gemm_precision, None):
                six = ops.afno_mlp6_supported(nb, bs) and ops.afno_mlp6_wanted()
                if six:
                    wc1 = torch.randn(2, nb, bs, bs, device="cuda") * 0.05
                    wc2 = torch.randn(2, nb, bs, bs, device="cuda") * 0.05
                    bc1 = torch.randn(2, nb, bs, device="cuda") * 0.1
                    bc2 = torch.randn(2, nb, bs, device="cuda") * 0.1
                    it1, it2 = ops.AfnoPacks([(wc1, bc1), (wc2, bc2)]).refresh()
                    six = it1.p6 is not None
                    if six:
                        b1, W1f, b2, W2f, three = it1[1], it1.p6[0], it2[1], it2.p6[0], False
        if six:
            pass
        elif three:
            # the three-product kernel takes the (Wr, Wi) fragment packs that the model's AfnoPacks writes
            wc1 = torch.randn(2, nb, bs, bs, device="cuda") * 0.05
            wc2 = torch.randn(2, nb, bs, bs, device="cuda") * 0.05
            bc1 = torch.randn(2, nb, bs, device="cuda") * 0.1
            bc2 = torch.randn(2, nb, bs, device="cuda") * 0.1
            pk = ops.AfnoPacks([(wc1, bc1), (wc2, bc2)])
            (_, b1, W1f, _), (_, b2, W2f, _) = pk.refresh()
        elif fused:
            W1f, _ = ops.afno_block_weights(W1)
            W2f, _ = ops.afno_block_weights(W2)

        def run(train: bool):
            if fused:
                # training form (round 3): only the pre-activation is saved; the backward launch re-derives act(pre)
                return ops.afno_mlp2(S, W1f, b1, W2f, b2, nb, bs, 1, mode=0, want_pre=train, want_mid=False,
                                     layout=2 if six else 1 if three else 0)
            O1, O1pre, O2 = torch.empty_like(S), torch.empty_like(S), torch.empty_like(S)
            kw = dict(lda=2 * E, ldb=N, ldc=2 * E, batch=nb, strideA=N, strideB=N * N, strideC=N, strideBias=N, tag=1)
            ops.gemm(S, W1, O1, Mm, N, N, bias=b1, act=1, mode=ops.EPI_ACT, preact=O1pre, ldpre=2 * E, stridePre=N, **kw)
            ops.gemm(O1, W2, O2, Mm, N, N, bias=b2, **kw)

        def timeit(train: bool, reps: int = 50):
            # `reps` launches captured in one hipGraph: the host cost of a Python -> ctypes launch (tens of us) must
            # not be what the events measure
            for _ in range(3):
                run(train)
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(reps):
                    run(train)
            g.replay()
            torch.cuda.synchronize()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) * 1e-3 / reps

        t = timeit(True)
        t_inf = timeit(False)
    flops = 2 * 2.0 * Mm * N * N * nb                          # = 151.0 MFLOP/sample (both MLP layers)
    # algorithmic bytes: spectrum in + spectrum out + the weights of both layers once
    bytes_alg = 2.0 * Mm * 2 * E * 4 + 2 * nb * N * N * 4
    achieved = flops / t / 1e12
    # HBM traffic per launch from the L2 memory-side counters: collected in separate rocprofv3 --pmc passes
    # (scripts/gpu_pmc.sh -> profiles/r02_pmc_mixer.json; bench.py itself cannot run the profiler).  Units and the
    # gfx950 correction follow MI355X_MICROARCH.md section HBM: bytes = (2 * FETCH_SIZE + WRITE_SIZE) * 1024
    traffic, pmc_file, mfma_util = None, "r06_pmc_mixer.json", None
    try:
        pdir = os.path.join(ROOT, "profiles")
        pmc_file = next((f for f in ("r06_pmc_mixer.json", "r05_pmc_mixer.json", "r04_pmc_mixer.json", "r03_pmc_mixer.json")
                         if os.path.exists(os.path.join(pdir, f))), "r03_pmc_mixer.json")
        pmc = json.load(open(os.path.join(pdir, pmc_file)))
        traffic = (2.0 * pmc["FETCH_SIZE"]["mean"] + pmc["WRITE_SIZE"]["mean"]) * 1024.0
        mfma_util = (pmc.get("tiny-train") or {}).get("mfma_util")
    except Exception:
        pass
    if six:
        return {
            "kernel": ("dpot::afno_mlp6_kernel<NT,PASSES> (AFNO mixer under gemm_precision auto: BOTH layers of the block-diagonal "
                       "complex MLP in one launch as bf16x6 - three bf16 planes per operand, six plane products on "
                       "v_mfma_f32_32x32x16_bf16, fp32-accurate; hidden layer kept in registers)"),
            "executed_flops_per_launch": flops * 6.0,
            "flops_note": "flops_per_launch / achieved / frac count the ALGORITHMIC fp32 work (SURVEY 8d); the kernel executes six "
                          "bf16 plane products per fp32 product: its roof is 2500 / 6 = 416.7 TFLOP/s of fp32-accurate work; `peak` "
                          "stays the fp32-MFMA 157.3 TFLOP/s the fp32 kernels are priced against, `frac_of_bf16x6_roof` prices "
                          "against its own",
            "bound": "mfma", "achieved": round(achieved, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
            "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "frac_of_bf16x6_roof": round(achieved / (2500.0 / 6.0), 4),
            "traffic": None, "mfma_util_pmc": 0.511 if (nb, bs, Mm) == (16, 96, 8704) else None,
            "traffic_note": "profiles/r06_pmc_mlp6.json (DPOT-L batch 16: 388 MB against 328 MB algorithmic)",
            "us_per_launch": round(t * 1e6, 2), "flops_per_launch": flops, "algorithmic_bytes_per_launch": bytes_alg,
            "hbm_frac": round(bytes_alg / t / 1e9 / HBM_PEAK_GBS, 4),
            "inference_form": {"us_per_launch": round(t_inf * 1e6, 2), "achieved": round(flops / t_inf / 1e12, 2),
                               "frac": round(flops / t_inf / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4)},
            "other_kernels": other_rooflines(model, B, timeit_graph),
        }
    return {
        "kernel": ("dpot::afno_mlp3_kernel<RT> (AFNO mixer: BOTH layers of the block-diagonal complex MLP in one launch, "
                   "each complex product as THREE real ones - P1 = Sr Wr, P2 = Si Wi, P3 = (Sr+Si)(Wr+Wi) - on "
                   "v_mfma_f32_16x16x4_f32, intermediate kept in LDS)") if three else
                  ("dpot::afno_mlp2_kernel<RT,NT> (AFNO mixer: BOTH layers of the block-diagonal complex MLP in one "
                   "launch - X W1 + b1 -> GELU -> W2 + b2 on v_mfma_f32_16x16x4_f32, intermediate kept in LDS)")
        if fused else "dpot::gemm_f32_kernel<64,64,NN,vec,TAG=1> x 2 (un-fused fallback)",
        "executed_flops_per_launch": flops * (0.75 if three else 1.0),
        "flops_note": ("flops_per_launch / achieved / frac count the ALGORITHMIC work (SURVEY 8d: 151.0 MFLOP per sample = "
                       "four real products per complex product); the kernel executes 3/4 of it (Gauss's three-product "
                       "complex multiplication), i.e. its matrix pipes run at 0.75 x achieved") if three else None,
        "bound": "mfma", "achieved": round(achieved, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
        "frac": round(achieved / FP32_MFMA_PEAK_TFLOPS, 4), "traffic": traffic, "mfma_util_pmc": mfma_util,
        "traffic_note": f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE (separate passes, profiles/{pmc_file}), "
                        "(2*FETCH+WRITE)*1024 B; the training form of the launch also stores the pre-activation (saved for "
                        "the backward): 2 spectrum-sized writes instead of the 1 that algorithmic_bytes counts (round 2 also "
                        "stored the activated spectrum: 3 writes, 80.7 MB)",
        "us_per_launch": round(t * 1e6, 2), "flops_per_launch": flops, "algorithmic_bytes_per_launch": bytes_alg,
        "hbm_frac": round(bytes_alg / t / 1e9 / HBM_PEAK_GBS, 4),
        "inference_form": {"us_per_launch": round(t_inf * 1e6, 2), "achieved": round(flops / t_inf / 1e12, 2),
                           "frac": round(flops / t_inf / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                           "what": "same launch without the saved-for-backward store (no_grad forward)"},
        "sustained_mfma_tflops": SUSTAINED_FP32_MFMA_TFLOPS,
        "frac_of_sustained": round(achieved / SUSTAINED_FP32_MFMA_TFLOPS, 4),
        "note": "FLOP-bound (128 FLOP/B >> 20 FLOP/B ridge): hbm_frac is reported because north_star asks for it; "
                "round 1 ran this as two launches of the generic GEMM (2 x 34.4 us, frac 0.446).  `peak` is the nominal "
                "157.3 TFLOP/s; a register-only v_mfma_f32_16x16x4_f32 loop on random data sustains 132.8 TFLOP/s on this "
                "part (power-limited clocks; profiles/r02_mfma_f32_peak.txt) - frac_of_sustained prices against that",
        "other_kernels": other_rooflines(model, B, timeit_graph),
    }


def bf16_mlp_roofline(model, B: int):
    """DPOT-S / -M / -L with the bf16 channel MLP: the dominant kernel is dpot::gemm_bf16p_kernel (csrc/gemm_bf16p.hip).
    Timed here in the form the forward launches it for fc1 (x W1^T + b -> GELU; row pack, transposed pack and act' pack of
    the hidden layer written, no fp32 output), HIP events around a hipGraph of 20 launches, random operands."""
    from dpot_amd import ops
    E, h = model.embed_dim, model.latent_size[0]
    M = B * h * h
    mh = model.blocks[0].mlp[0].weight.shape[0]
    x = torch.randn(M, E, device="cuda")
    W1 = torch.randn(mh, E, device="cuda") * 0.03
    b1 = torch.randn(mh, device="cuda") * 0.1
    pk = ops.PanelPacks([(W1, mh, E, E, False)], bf16=True)
    pk.refresh()
    xp = ops.bf16_pack_rows(x)
    t = timeit_graph(lambda: ops.gemm_bf16p_packed(xp, pk.bufs[0], M, mh, E, bias=b1, act=1, mode=ops.EPI_ACT, save_dact=True,
                                                    pack_rows=True, pack_trans=True, store=False), reps=20)
    fl = 2.0 * M * mh * E
    npk = 3
    by = 2.0 * M * E + 2.0 * mh * E + npk * 2.0 * M * mh          # packed A + packed W read once, the bf16 packs written
    traffic, tnote, util = None, "no PMC profile for this shape (profiles/r05_pmc_bf16p_{S,M,L16}.json)", None
    for tag in ("M", "L16", "S"):                        # counter profiles by shape (scripts/gpu_pmc_bf16p_r05.sh SHAPE)
        try:
            pf = next(f for f in (f"r06_pmc_bf16p_{tag}.json", f"r05_pmc_bf16p_{tag}.json")
                      if os.path.exists(os.path.join(ROOT, "profiles", f)))
            doc = json.load(open(os.path.join(ROOT, "profiles", pf)))
            sh = doc["shape"]
            if (M, E, mh) != (sh["tokens"], sh["E"], sh["hidden"]):
                continue
            pmc = doc["forms"]["fc1_fwd"]
            traffic = float(pmc["bytes_guide"])
            util = pmc.get("mfma_util")
            tnote = (f"rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE, separate passes (profiles/{pf}): (2*FETCH + "
                     "WRITE)*1024 B; un-doubled %.0f MB; algorithmic = A pack + W pack read once + three bf16 packs written"
                     % (pmc["bytes_raw"] / 1e6))
            break
        except Exception:
            continue
    kname = ops.gemm_bf16p_kernel_name(M, mh, E, packed_outputs=True)       # the library's own selection
    yard = None
    try:
        yard = _compact_yardstick(gemm_yardstick(M, E, mh))
    except Exception as e:                                     # pragma: no cover - the yardstick must never take the line down
        log(f"[bench] hipBLASLt yardstick failed: {type(e).__name__}: {e}")
    return {"kernel": kname + " - channel-MLP fc1 forward: bf16 operands pre-packed fragment-block-major, "
                      "v_mfma_f32_32x32x16_bf16, epilogue in the accumulator layout writes the activated hidden layer as a row-form "
                      "bf16 pack + a transposed one and act' as a bf16 pack",
            "shape": [M, mh, E], "bound": "mfma", "achieved": round(fl / t / 1e12, 1), "peak": 2500.0, "unit": "TFLOP/s",
            "frac": round(fl / t / 1e12 / 2500.0, 4), "us_per_launch": round(t * 1e6, 2), "flops_per_launch": fl,
            "algorithmic_bytes_per_launch": by, "hbm_frac": round(by / t / 1e9 / HBM_PEAK_GBS, 4), "traffic": traffic,
            "traffic_note": tnote, "mfma_util_pmc": util, "yardstick": yard,
            "note": "2.5 PFLOP/s = dense bf16 MFMA peak (MI355X_MICROARCH.md); a register-only MFMA loop sustains 1.4-1.8 "
                    "PFLOP/s on random operands on this part (profiles/r02_mfma_bf16_peak.txt).  This launch is the one with the "
                    "fattest epilogue (GELU + derivative on 33.5 M values, 201 MB of packs at DPOT-M); the same product with a plain "
                    "fp32 output runs at 0.9-1.1 PFLOP/s (profiles/r04_bf16p_train_bench.txt)"}


def timeit_graph(fn, reps: int = 30):
    """seconds per call of `fn`, `reps` launches captured in one hipGraph (the host cost of a Python launch excluded)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(reps):
            fn()
    g.replay()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    g.replay()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) * 1e-3 / reps


def other_rooflines(model, B: int, timeit):
    """the next kernels of the step by time share, timed the same way (random operands, graph-captured launches)"""
    from dpot_amd import ops
    out = []
    try:
        E, h = model.embed_dim, model.latent_size[0]
        M = B * h * h
        mh = model.blocks[0].mlp[0].weight.shape[0]
        A = torch.randn(M, E, device="cuda")
        W = torch.randn(mh, E, device="cuda") * 0.05
        b = torch.randn(mh, device="cuda") * 0.1
        dy = torch.randn(M, mh, device="cuda")
        fl = 2.0 * M * mh * E
        if ops.gemm_panel_supported(M, mh, E):
            pk = ops.PanelPacks([(W, mh, E, E, False)])
            pk.refresh()
            t = timeit(lambda: ops.gemm_panel(A, pk.bufs[0], mh, bias=b, act=1, mode=ops.EPI_ACT, save_pre=True))
            out.append({"kernel": "dpot::gemm_panel_kernel (channel-MLP fc1 forward: x W1^T + b -> GELU, pre-activation saved)",
                        "shape": [M, mh, E], "bound": "mfma", "us_per_launch": round(t * 1e6, 2),
                        "achieved": round(fl / t / 1e12, 2), "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                        "frac": round(fl / t / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                        "frac_of_sustained": round(fl / t / 1e12 / SUSTAINED_FP32_MFMA_TFLOPS, 4)})
        t = timeit(lambda: ops.linear_bwd_wb(dy, A))
        out.append({"kernel": "dpot::gemm_tn_kernel + splitk_reduce (ONE channel-MLP weight gradient dY^T X with its bias "
                              "gradient; the train step runs fc1's and fc2's as one launch)", "shape": [mh, E, M],
                    "bound": "mfma",
                    "us_per_launch": round(t * 1e6, 2), "achieved": round(fl / t / 1e12, 2),
                    "peak": FP32_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                    "frac": round(fl / t / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
                    "frac_of_sustained": round(fl / t / 1e12 / SUSTAINED_FP32_MFMA_TFLOPS, 4)})
        x = torch.randn(B, h * h, E, device="cuda")
        nb = model.n_blocks
        mx, my = min(model.modes, h), min(model.modes, h // 2 + 1)
        gw, gb_ = torch.randn(E, device="cuda"), torch.randn(E, device="cuda")
        fld, spc = x.numel() * 4, B * mx * my * 2 * E * 4
        if ops.gn_dft_supported(h, h, E):
            # GroupNorm fused with the mixer's DFTs (csrc/gn_dft.hip): the four launches around the mixer kernel
            S_, m1_, r1_ = ops.gn_rfft2(x, gw, gb_, h, h, nb, mx, my)
            y1_, xn2_, m2_, r2_ = ops.irfft2_gn(S_, x, m1_, r1_, gw, gb_, gw, gb_, h, h, nb, mx, my)
            dy_ = torch.randn_like(x)
            fused = [("gn_rfft2_kernel (GroupNorm1 statistics + rfft2; GroupNorm1(x) never written)",
                      lambda: ops.gn_rfft2(x, gw, gb_, h, h, nb, mx, my), fld + spc),
                     ("irfft2_gn_kernel (irfft2 + x_orig + GroupNorm2: y1 and xn2 written)",
                      lambda: ops.irfft2_gn(S_, x, m1_, r1_, gw, gb_, gw, gb_, h, h, nb, mx, my), spc + 3 * fld),
                     ("gn_bwd_rfft2_kernel (GroupNorm2 backward + adjoint rfft2)",
                      lambda: ops.gn_bwd_rfft2(dy_, y1_, m2_, r2_, gw, h, h, nb, mx, my), 3 * fld + spc)]
            if E // 8 <= 64:
                fused.append(("irfft2_gn_bwd_kernel (adjoint irfft2 + skip + GroupNorm1 backward + outer skip)",
                              lambda: ops.irfft2_gn_bwd(S_, dy_, x, m1_, r1_, gw, h, h, nb, mx, my, add=dy_), spc + 4 * fld))
            for name, fn, by in fused:
                t = timeit(fn)
                out.append({"kernel": "dpot::" + name, "bound": "hbm", "us_per_launch": round(t * 1e6, 2),
                            "achieved": round(by / t / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                            "frac": round(by / t / 1e9 / HBM_PEAK_GBS, 4)})
        else:
            t = timeit(lambda: ops.rfft2(x, h, h, nb, mx, my, 0))
            out.append({"kernel": "dpot::rfft2_fast_kernel (field -> kept modes, register FFTs)", "bound": "hbm",
                        "us_per_launch": round(t * 1e6, 2), "achieved": round((fld + spc) / t / 1e9, 1), "peak": HBM_PEAK_GBS,
                        "unit": "GB/s", "frac": round((fld + spc) / t / 1e9 / HBM_PEAK_GBS, 4)})
            t = timeit(lambda: ops.groupnorm_fwd(x, gw, gb_))
            out.append({"kernel": "dpot::groupnorm_fwd_cached_kernel", "bound": "hbm", "us_per_launch": round(t * 1e6, 2),
                        "achieved": round(2 * fld / t / 1e9, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                        "frac": round(2 * fld / t / 1e9 / HBM_PEAK_GBS, 4)})
        # fused per-pixel tail of the de-embed (csrc/tail.hip): NOT HBM-bound - fp32 MFMA and fp32 VALU share the FMA
        # lanes on gfx950 (profiles/r02_pmc_tail.json: VALU-active + MFMA-busy = kernel time); hbm frac reported because
        # VERDICT r1 prices these kernels against the HBM roof
        P, co, old = model.patch_size, model.out_channels * model.out_timesteps, model.out_layer[0].weight.shape[1]
        npx = B * h * h * P * P
        if ops.out_tail_supported(old, co, npx):
            up = torch.randn(npx, old, device="cuda")
            do = torch.randn(B, h * P, h * P, co, device="cuda")
            w2 = torch.randn(old, old, device="cuda") * 0.2
            b2 = torch.randn(old, device="cuda") * 0.1
            w4p, b4p = ops.out_tail_pad(torch.randn(co, old, device="cuda") * 0.2, torch.randn(co, device="cuda"), co)
            for name, fn, by in (("out_tail_fwd_kernel", lambda: ops.out_tail_fwd(up, w2, b2, w4p, b4p, B, h, h, P, co, 1),
                                  (npx * old + npx * co) * 4),
                                 ("out_tail_bwd_kernel (+ partial-row reduction)",
                                  lambda: ops.out_tail_bwd(up, do, w2, b2, w4p, B, h, h, P, co, 1),
                                  (2 * npx * old + npx * co) * 4)):
                t = timeit(fn)
                out.append({"kernel": f"dpot::{name} (act -> 1x1 conv -> act -> 1x1 conv -> pixel shuffle, one kernel)",
                            "bound": "valu+mfma (fp32 MFMA and VALU share the FMA lanes; 64 exact-erf GELUs per pixel)",
                            "us_per_launch": round(t * 1e6, 2), "achieved": round(by / t / 1e9, 1), "peak": HBM_PEAK_GBS,
                            "unit": "GB/s", "frac": round(by / t / 1e9 / HBM_PEAK_GBS, 4)})
    except Exception as e:      # the probe must never take the headline down
        log(f"[bench] secondary roofline probe failed: {e}")
    return out


def gemm_yardstick(M: int, E: int, mh: int, timeit=None):
    """MEASUREMENT-ONLY yardstick (VERDICT r5 #1a): the five channel-MLP GEMM shapes of this config as plain `torch.mm` calls on
    bf16 tensors - i.e. hipBLASLt's tuned bf16 GEMM on this very box, same timing code (hipGraph of launches, HIP events) -
    beside this build's launches of the same products.  torch / hipBLASLt are NEVER on the product path (dpot_amd/ does not
    import them for any GEMM); the rows only give `frac` a same-box denominator: what a vendor-tuned GEMM attains at the
    shape.  Forms: bf16 in -> bf16 out (hipBLASLt's cheapest store; compare with our packed-output launches) and bf16 in ->
    fp32 out (`out_dtype`, compare with our fp32-out launches)."""
    from dpot_amd import ops
    timeit = timeit or timeit_graph
    bf = torch.bfloat16
    dev = "cuda"
    x = torch.randn(M, E, device=dev)
    do = torch.randn(M, E, device=dev)
    W1 = torch.randn(mh, E, device=dev) * 0.03
    W2 = torch.randn(E, mh, device=dev) * 0.03
    b1 = torch.randn(mh, device=dev) * 0.1
    b2 = torch.randn(E, device=dev) * 0.1
    xb, dob, W1b, W2b = x.to(bf), do.to(bf), W1.to(bf), W2.to(bf)
    hb = torch.randn(M, mh, device=dev).to(bf)
    dhb = torch.randn(M, mh, device=dev).to(bf)
    fl = 2.0 * M * E * mh

    def blaslt(a, b):
        """(us bf16-out, us fp32-out | None) of a @ b through torch.mm (hipBLASLt)"""
        t16 = timeit(lambda: torch.mm(a, b), reps=20)
        try:
            torch.mm(a, b, out_dtype=torch.float32)
            t32 = timeit(lambda: torch.mm(a, b, out_dtype=torch.float32), reps=20)
        except Exception:
            t32 = None
        return t16, t32

    pk = ops.PanelPacks([(W1, mh, E, E, False), (W1, E, mh, E, True), (W2, E, mh, mh, False), (W2, mh, E, mh, True)], bf16=True)
    pk.refresh()
    xp, xpT, _ = ops.bf16_pack_both(x)
    dop, dopT, _ = ops.bf16_pack_both(do)
    _, D, hp, hpT, _ = ops.gemm_bf16p_packed(xp, pk.bufs[0], M, mh, E, bias=b1, act=1, mode=ops.EPI_ACT, save_dact=True,
                                             pack_rows=True, pack_trans=True, store=False)
    _, _, dhp, dhpT, _ = ops.gemm_bf16p_packed(dop, pk.bufs[3], M, mh, E, act=1, mode=ops.EPI_DACT, dact=D, pack_rows=True,
                                               pack_trans=True, colsum=True, store=False)
    rows = []

    def row(form, ours_s, ours_what, y16, y32, nfl=1.0):
        f = fl * nfl
        best = min(t for t in (y16, y32) if t is not None)
        rows.append({"form": form, "flops": f, "ours_us": round(ours_s * 1e6, 1), "ours_TF": round(f / ours_s / 1e12, 1),
                     "ours": ours_what, "blaslt_bf16out_us": round(y16 * 1e6, 1),
                     "blaslt_f32out_us": None if y32 is None else round(y32 * 1e6, 1),
                     "blaslt_best_TF": round(f / best / 1e12, 1),
                     "ours_over_blaslt_bf16out": round(ours_s / y16, 3),
                     "ours_over_blaslt_f32out": None if y32 is None else round(ours_s / y32, 3)})

    t = timeit(lambda: ops.gemm_bf16p_packed(xp, pk.bufs[0], M, mh, E, bias=b1, act=1, mode=ops.EPI_ACT, save_dact=True,
                                             pack_rows=True, pack_trans=True, store=False), reps=20)
    row("fc1_fwd [M,E]x[E,mh]", t, "bias+GELU, writes 3 bf16 packs (row, transposed, act')", *blaslt(xb, W1b.t()))
    t = timeit(lambda: ops.gemm_bf16p(hp, pk.bufs[2], M, E, mh, bias=b2, res=x), reps=20)
    row("fc2_fwd [M,mh]x[mh,E]", t, "bias + residual, fp32 out", *blaslt(hb, W2b.t()))
    t = timeit(lambda: ops.gemm_bf16p_packed(dop, pk.bufs[3], M, mh, E, act=1, mode=ops.EPI_DACT, dact=D, pack_rows=True,
                                             pack_trans=True, colsum=True, store=False), reps=20)
    row("fc2_dgrad [M,E]x[E,mh]", t, "x act' pack, writes 2 bf16 packs + column sums", *blaslt(dob, W2b))
    t = timeit(lambda: ops.gemm_bf16p(dhp, pk.bufs[1], M, E, mh), reps=20)
    row("fc1_dgrad [M,mh]x[mh,E]", t, "fp32 out", *blaslt(dhb, W1b))
    if ops.gemm_bf16p_pair_wanted(E, mh, mh, E, M):
        o0, o1 = torch.empty(E, mh, device=dev), torch.empty(mh, E, device=dev)
        t = timeit(lambda: ops.gemm_bf16p_pair(dopT, hpT, E, mh, dhpT, xpT, mh, E, M, out0=o0, out1=o1), reps=20)
        a16, a32 = blaslt(dob.t(), hb)
        c16, c32 = blaslt(dhb.t(), xb)
        row("wgrad pair [E,M]x[M,mh] + [mh,M]x[M,E]", t, "both weight gradients, one launch, fp32 out", a16 + c16,
            None if a32 is None or c32 is None else a32 + c32, nfl=2.0)
    return rows


def cpu_baseline(seconds: float):
    """the CPU oracle (a port of the reference's PyTorch-CPU path; parity-pinned in tests/) timed on this box's host
    cores on a bounded sample of the same workload: DPOT-Tiny train steps at B=4 (BASELINE configs[0])."""
    from oracle import dpot_ref as R
    cores = os.cpu_count() or 1
    cfg = R.DPOTConfig(**R.TINY)
    g = torch.Generator().manual_seed(1234)
    B = 4
    st = R.TrainState(params={k: v.clone() for k, v in R.recipe_state_dict(cfg, salt=1).items()})
    xx = torch.randn(B, 128, 128, 10, 4, generator=g)
    yy = torch.randn(B, 128, 128, 1, 4, generator=g)
    msk = torch.ones(B, 128, 128, 1, 4)
    # BASELINE.md section 3 / SURVEY 8(d): n = 16 threads (the reference hard-codes OMP_NUM_THREADS=16, train_temporal.py:4)
    # AND n = all physical cores of the box; `value` = the faster of the two (give the CPU its best shot), both reported
    try:
        import psutil
        phys = psutil.cpu_count(logical=False) or cores
    except Exception:                                           # pragma: no cover
        phys = cores

    def timed(threads, secs):
        torch.set_num_threads(threads)
        R.train_step(st, xx, yy, msk, cfg, lr=1e-3)            # warm-up at this thread count
        n, t0 = 0, time.perf_counter()
        while True:
            R.train_step(st, xx, yy, msk, cfg, lr=1e-3)
            n += 1
            el = time.perf_counter() - t0
            if el >= secs or n >= 200:
                break
        return {"threads": threads, "value": round(B * n / el, 2), "steps": n, "seconds": round(el, 1)}

    runs = [timed(min(16, cores), seconds * 0.5)]
    if phys != runs[0]["threads"]:
        runs.append(timed(phys, seconds * 0.5))
    best = max(runs, key=lambda r: r["value"])
    return {"value": best["value"], "unit": "samples/s", "cores": best["threads"], "kind": "port",
            "physical_cores": phys, "logical_cores": cores,
            "by_threads": {str(r["threads"]): r["value"] for r in runs},
            "sample": f"DPOT-Tiny train step (fwd+loss+bwd+clip+Adam), B={B}: "
                      + "; ".join(f"{r['steps']} steps in {r['seconds']} s at {r['threads']} threads = {r['value']} samples/s"
                                  for r in runs)
                      + f"; torch {torch.__version__} CPU, {phys} physical / {cores} logical cores; the port is ~10% "
                      f"SLOWER than the imported reference module on the same CPU (build container, 8 threads: 179 vs "
                      f"199 ms/step - VERDICT r1), so a 'reference' baseline would read ~1.1x this value"}


# the fastest (per-GPU batch, kept AR steps) point of the DPOT-L 20-step rollout that fits 288 GiB, from the sweep on one box
# (profiles/r06_l20_sweep.txt); the L20 entry itself stays at the LARGEST batch that fits, this one is reported beside it
L20_FASTEST = {"batch": 9, "keep_last": 20}


def _child(args, key, steps, warm, extra=(), env=None, timeout=300):
    import subprocess
    cmd = [sys.executable, os.path.abspath(__file__), "--gpus", "1", "--config", key, "--full", "--brief", "--steps",
           str(steps), "--warmup", str(warm), "--noise-scale", str(args.noise_scale)] + list(extra)
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=dict(os.environ, **(env or {})))
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")]
    if r.returncode != 0 or not line:
        raise RuntimeError(f"rc {r.returncode}: {r.stderr[-400:]}")
    return json.loads(line[-1])


def other_configs(args):
    """BASELINE configs[2..4] (DPOT-S / -M / -L at batch 16 / the 20-step DPOT-L rollout), each as ONE short child run of
    this script (`--config X --brief`): fresh process = fresh kernel-selection state, the same timing code as the headline.
    Kept short (the --full run must finish within minutes): steps / warm-up scaled to the step time.  Entries are COMPACT
    (numbers; a few hundred bytes each) so that the driver's 8 KB stdout tail holds all of them."""
    res = []
    for key, steps, warm in (("S", 20, 5), ("M", 20, 5), ("L", 8, 3), ("L20", 2, 1)):
        t0 = time.perf_counter()
        try:
            d = _child(args, key, steps, warm, extra=["--no-alt"] if key == "L20" else [])
            rl = d.get("roofline") or {}
            cfg = d["config"]
            ent = {"config": key, "baseline_config": cfg["baseline_config"], "value": d["value"], "unit": d["unit"],
                   "ms_per_step": d["ms_per_step"], "steps": d["steps"], "warmup": d["warmup"], "dtype": "f32, bf16 MLP operands",
                   "per_gpu_batch": cfg["per_gpu_batch"], "launch": cfg["launch"], "gemm_precision": cfg["gemm_precision"],
                   "recompute": cfg["activation_recomputation"], "peak_mem_GB": cfg["peak_mem_GB"],
                   "final_loss": cfg["final_loss"], "mixed_ceiling": (d.get("mixed_ceiling") or {}).get("value"),
                   "frac_of_mixed_ceiling": d.get("frac_of_mixed_ceiling"),
                   "x_of_baseline_md_ceiling": d.get("x_of_baseline_md_ceiling"),
                   "value_gemm_f32": (d.get("gemm_f32") or {}).get("value"),
                   "value_f32": (d.get("all_f32") or {}).get("value"),
                   "ms_per_step_f32": (d.get("all_f32") or {}).get("ms_per_step"),
                   "roofline": {k: rl.get(k) for k in ("kernel", "shape", "bound", "achieved", "peak", "unit", "frac", "traffic",
                                                       "us_per_launch", "mfma_util_pmc")},
                   "mixer": next(({k: o.get(k) for k in ("kernel", "frac", "us")}
                                  for o in rl.get("other_kernels", []) if "afno" in str(o.get("kernel"))), None),
                   "yardstick": rl.get("yardstick")}
            if key == "L20":
                try:
                    f = _child(args, key, steps, warm, extra=["--no-alt", "--batch", str(L20_FASTEST["batch"])],
                               env={"DPOT_BENCH_KEEP_LAST": str(L20_FASTEST["keep_last"])})
                    ent["fastest"] = {"B": L20_FASTEST["batch"], "keep_last": L20_FASTEST["keep_last"], "value": f["value"],
                                      "ms_per_step": f["ms_per_step"], "peak_mem_GB": f["config"]["peak_mem_GB"],
                                      "sweep": "profiles/r06_l20_sweep.txt"}
                except Exception as e:                          # pragma: no cover
                    ent["fastest"] = {"error": f"{type(e).__name__}: {e}"[:200]}
            ent["wall_s"] = round(time.perf_counter() - t0, 1)
            res.append(ent)
        except Exception as e:                                  # pragma: no cover - must never take the headline down
            log(f"[bench] other config {key} failed: {type(e).__name__}: {e}")
            res.append({"config": key, "error": f"{type(e).__name__}: {e}"[:300]})
    return res


def _kshort(k):
    """kernel name without its prose: 'dpot::afno_mlp3_kernel<RT> (AFNO mixer: ...)' -> 'dpot::afno_mlp3_kernel<RT>'"""
    if not isinstance(k, str):
        return k
    for sep in (" (", " - ", " + "):
        i = k.find(sep)
        if i > 0:
            k = k[:i]
    return k[:64]


_RL_KEYS = ("kernel", "shape", "bound", "achieved", "peak", "unit", "frac", "traffic", "us_per_launch", "flops_per_launch",
            "executed_flops_per_launch", "algorithmic_bytes_per_launch", "hbm_frac", "frac_of_sustained", "mfma_util_pmc")


def _compact_roofline(rl, keep_others=True):
    if not rl:
        return rl
    out = {k: rl[k] for k in _RL_KEYS if rl.get(k) is not None or k == "traffic"}
    out["kernel"] = _kshort(out.get("kernel"))
    if isinstance(out.get("bound"), str):
        out["bound"] = out["bound"].split(" ")[0]
    if rl.get("inference_form"):
        out["inference_form"] = {k: rl["inference_form"][k] for k in ("us_per_launch", "frac")}
    if keep_others and rl.get("other_kernels"):
        out["other_kernels"] = [{"kernel": _kshort(o.get("kernel")), "bound": str(o.get("bound", "")).split(" ")[0],
                                 "us": o.get("us_per_launch"), "achieved": o.get("achieved"), "unit": o.get("unit"),
                                 "frac": o.get("frac")} for o in rl["other_kernels"]]
    if rl.get("yardstick"):
        out["yardstick"] = rl["yardstick"]
    return out


def _compact_yardstick(rows):
    """[form, ours us, hipBLASLt bf16-out us, hipBLASLt fp32-out us] per channel-MLP GEMM form + the worst ratio"""
    if not rows:
        return None
    tab = [[r["form"].split(" ")[0], r["ours_us"], r["blaslt_bf16out_us"], r["blaslt_f32out_us"]] for r in rows]
    tot_o = sum(r["ours_us"] for r in rows)
    tot_y = sum(min(t for t in (r["blaslt_bf16out_us"], r["blaslt_f32out_us"]) if t is not None) for r in rows)
    # rows: [form, ours us, hipBLASLt bf16-out us, hipBLASLt fp32-out us] (torch.mm on bf16 tensors, same box / timing code;
    # measurement only, never on the product path - DESIGN.md section 7)
    return {"rows": tab, "ours_over_hipblaslt_best_total": round(tot_o / tot_y, 3)}


def compact_line(out: dict) -> dict:
    """the ONE JSON line the driver records: numbers only, prose lives in DESIGN.md section 7; `other_configs` LAST so the
    driver's 8 KB stdout tail always holds S / M / L / L20.  The verbose form goes to stderr / --full-json."""
    c = {}
    for k in ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline",
              "dtype", "data"):
        c[k] = out.get(k)
    cfg = dict(out.get("config", {}))
    if isinstance(cfg.get("per_rank"), dict):
        cfg["per_rank"] = {k: v for k, v in cfg["per_rank"].items() if k != "note"}
    if isinstance(cfg.get("collectives"), dict):
        cfg["collectives"] = {k: (v[:80] if isinstance(v, str) else v) for k, v in cfg["collectives"].items()}
    if isinstance(cfg.get("dp"), str):
        cfg["dp"] = cfg["dp"][:120]
    c["config"] = cfg
    c["doc"] = "DESIGN.md section 7 defines every key; verbose form: stderr '[bench-full]' / --full-json"
    for k in ("sustained", "model_flops_frac", "executed_flops_frac", "mixed_ceiling", "frac_of_mixed_ceiling",
              "baseline_md_ceiling", "x_of_baseline_md_ceiling"):
        if k in out:
            c[k] = out[k]
    if "roofline" in out:
        c["roofline"] = _compact_roofline(out["roofline"])
    for k in ("gemm_auto", "gemm_f32", "all_f32", "inference", "pipeline_inclusive"):
        if k in out:
            c[k] = {kk: vv for kk, vv in out[k].items() if kk not in ("what", "note", "gemm_precision")}
    if "cpu_baseline" in out:
        cb = out["cpu_baseline"]
        c["cpu_baseline"] = {k: cb[k] for k in ("value", "unit", "cores", "kind", "physical_cores", "by_threads") if k in cb}
        c["cpu_baseline"]["sample"] = cb.get("sample_short", cb.get("sample", ""))[:160]
        c["speedup_vs_cpu_baseline"] = out.get("speedup_vs_cpu_baseline")
    if "l20_plane" in out:
        c["l20_plane"] = out["l20_plane"]
    if "other_configs" in out:
        c["other_configs"] = out["other_configs"]
    return c


# ------------------------------------------------------------------------------------------------------
def _self_launch(n: int) -> int:
    """`python bench.py --gpus N` with no launcher around it: re-execute under torch.distributed.run, one rank per GPU,
    rendezvous on 127.0.0.1 (the container hostname may not resolve)"""
    import socket
    import subprocess
    sk = socket.socket()
    sk.bind(("127.0.0.1", 0))
    port = sk.getsockname()[1]
    sk.close()
    env = dict(os.environ)
    env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={n}", "--master-addr",
           "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    log("[bench] no launcher detected (WORLD_SIZE unset): " + " ".join(cmd))
    return subprocess.call(cmd, env=env)


def dump_outputs(path: str, loss, pred, opt, grad_scale: float) -> None:
    """--dump-outputs: what a caller of the timed step holds after its last replay - the loss, the prediction, the global
    gradient norm the clip used and the updated flat parameters - as fp32 .npy files.  An array larger than its cap is
    replaced by its flattened elements at a fixed sample of indices (seed 0, ascending; the same for every build)."""
    import numpy as np
    os.makedirs(path, exist_ok=True)

    def put(name, t, cap=None):
        t = t.detach().float()
        if cap is not None and t.numel() > cap:
            idx = np.sort(np.random.default_rng(0).choice(t.numel(), size=cap, replace=False))
            t = t.reshape(-1)[torch.from_numpy(idx).to(t.device)]
        np.save(os.path.join(path, f"{name}.npy"), t.cpu().numpy())

    put("loss", loss)
    if pred is not None:
        put("pred", pred, DUMP_MAX_PRED)
    put("grad_norm", opt.grad_norm(grad_scale))
    put("params", opt.fp.flat, DUMP_MAX_PARAMS)
    log(f"[bench] outputs of the last timed step written to {path}")


def _flush_c_stdio():
    try:
        import ctypes
        ctypes.CDLL(None).fflush(None)
    except Exception:                                          # pragma: no cover
        pass
    sys.stdout.flush()


def main():
    args = parse()
    final_line = ""
    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        raise SystemExit(_self_launch(args.gpus))
    rank = int(os.environ.get("RANK", 0))
    local_rank = int(os.environ.get("LOCAL_RANK", 0))
    world = int(os.environ.get("WORLD_SIZE", 1))
    if args.gpus != world:
        log(f"[bench] --gpus {args.gpus} but WORLD_SIZE={world}: running with the launcher's world size")
    cname, ckw, cB, T_ar, cmlp, recompute, cbase = CONFIGS[args.config]
    headline = args.config == "T"
    if args.gemm_precision is None:
        args.gemm_precision = CONFIG_GEMM[args.config]
    # DPOT_BENCH_DEBUG_GLOO=1: functional dry-run of the N>1 code path on a 1-GPU box (all ranks share cuda:0, gloo
    # collectives) - for testing only, never a performance number
    debug_gloo = os.environ.get("DPOT_BENCH_DEBUG_GLOO") == "1"
    if debug_gloo:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    # DPOT_BENCH_FORCE_DP=1 (1-GPU box): take the N>1 code path with a ONE-rank RCCL communicator - the bucket all-reduces
    # are real calls into torch's ProcessGroupNCCL / RCCL on the side stream between the graph segments.  RCCL enqueues NO
    # device work for a one-rank in-place all-reduce (rocprofv3 shows no kernel), so what is measured on hardware is the
    # communicator set-up, the host path and the stream hand-offs of the chain - not a collective's run time
    force_dp = world == 1 and os.environ.get("DPOT_BENCH_FORCE_DP") == "1"
    dp_on = world > 1 or force_dp
    if force_dp:
        os.environ.setdefault("MASTER_PORT", "29517")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
    if dp_on:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        if debug_gloo:
            dist.init_process_group("gloo")
        else:
            dist.init_process_group("nccl", device_id=torch.device("cuda", local_rank))

    from dpot_amd import DPOTNet, _lib, ops
    from dpot_amd.dp import BucketedGradReducer
    from dpot_amd.train import (FlatParams, FusedAdam, GraphedTrainStep, SegmentedTrainStep, make_dp_step, one_cycle_lr,
                                train_step)
    from dpot_amd.dp import dp_one_cycle_lr
    _lib.load()

    mlp_prec = args.mlp_precision if args.mlp_precision is not None else cmlp

    torch.manual_seed(0)                                       # identical random-init weights on every rank
    model = DPOTNet(**ckw).cuda()
    model.mlp_precision = mlp_prec                             # per-model attributes (None: the process default = f32)
    model.gemm_precision = args.gemm_precision
    model.recompute_blocks = recompute
    # selective recomputation: the last KEEP_LAST AR steps of the rollout keep their activations (their backward runs first and
    # frees them before the first recomputation) - free HBM spent on time; DPOT_BENCH_KEEP_LAST overrides
    keep_last = 0
    if recompute and T_ar > 1:
        # what fits: the rollout with every step recomputed peaks at ~7.0 GiB per sample, a kept step costs ~1.07 GiB per sample
        # (measured at batch 16: 112.4 and 17.15 GiB); leave 30 GiB of the free memory alone (batch 16 on an empty 288 GiB card: 8)
        Bq = args.batch if args.batch is not None else cB
        free_gib = torch.cuda.mem_get_info()[0] / 2 ** 30
        fit = int((free_gib - 30.0 - 7.03 * Bq) / (1.072 * Bq))
        keep_last = max(0, min(fit, T_ar))
    keep_last = int(os.environ.get("DPOT_BENCH_KEEP_LAST", keep_last))
    model.recompute_keep_last = keep_last
    fp = FlatParams(model)
    # DDP semantics for N>1: cls_head takes part (zero gradients -> weight decay only), grads averaged over ranks
    opt = FusedAdam(fp, lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0, update_tail=dp_on)
    reducer = BucketedGradReducer(fp, overlap=True) if dp_on else None     # bucket count by gradient bytes (dp.auto_n_buckets)
    if reducer is not None:
        reducer.single_rank_collective = force_dp
        reducer.broadcast_parameters(0)
    grad_scale = 1.0 / world

    B = args.batch if args.batch is not None else cB
    res = ckw["img_size"]
    g = torch.Generator().manual_seed(1234 + rank)
    xx = torch.randn(B, res, res, 10, 4, generator=g).cuda()
    yy = torch.randn(B, res, res, T_ar, 4, generator=g).cuda()
    msk = torch.ones(B, res, res, 1, 4, device="cuda")
    total_steps = args.warmup + args.steps + 8
    # N>1: accelerate steps the scheduler `world` times per optimiser step over a schedule sized by the unsharded
    # loader (train_temporal_parallel.py:150,185) - dp.dp_one_cycle_lr reproduces that rule
    lr_at = (lambda s: dp_one_cycle_lr(s, world, max(total_steps, 10) * world, 1e-3, pct_start=0.2)) if dp_on \
        else (lambda s: one_cycle_lr(s, max(total_steps, 10), 1e-3, pct_start=0.2))

    mode = "eager"
    graphed = None
    dp_info = None
    if not args.no_graph and not (dp_on and args.overlap):
        try:
            # N>1: the graph holds fwd+bwd only; the all-reduce and the optimiser run after the replay
            if dp_on and args.no_overlap:
                graphed = _GraphedFwdBwd(model, opt, xx, yy, msk, args.noise_scale)
            elif dp_on and os.environ.get("DPOT_DP_ONE_GRAPH") == "1":
                # opt-in: the WHOLE data-parallel step, bucket all-reduces included, as one hipGraph
                graphed = GraphedTrainStep(model, opt, xx, yy, msk, noise_scale=args.noise_scale,
                                           warmup=1 if T_ar > 1 else 2, reducer=reducer, capture_collectives=True)
            elif dp_on:
                # default N>1 path (round 6): train.make_dp_step - the segmented hipGraph chain (cut at the gradient-bucket
                # boundaries, bucket k all-reduced on the side stream while the compute stream replays the backward of the
                # earlier stages) AND the one-graph step (collectives captured) are both built, one trial step is run in each
                # from the same snapshot, and the one-graph step is kept only if its reduced gradient is bit-identical to the
                # chain's and across the ranks.  DPOT_DP_ONE_GRAPH=0: the chain without the trial
                graphed, dp_info = make_dp_step(model, opt, reducer, xx, yy, msk, noise_scale=args.noise_scale,
                                                warmup=1 if T_ar > 1 else 2,
                                                try_one_graph=os.environ.get("DPOT_DP_ONE_GRAPH", "auto") != "0")
            else:
                graphed = GraphedTrainStep(model, opt, xx, yy, msk, noise_scale=args.noise_scale,
                                           warmup=1 if T_ar > 1 else 2)
            mode = "hipgraph"
        except Exception as e:                                 # pragma: no cover - depends on the box
            log(f"[bench] hipGraph capture failed ({type(e).__name__}: {e}); falling back to eager launches")
            graphed = None

    step_idx = [0]
    eager_pred = [None]                                        # the eager step's prediction (a graph keeps its own)

    def one_step():
        lr = lr_at(step_idx[0])
        step_idx[0] += 1
        if graphed is None:
            loss, eager_pred[0] = train_step(model, opt, xx, yy, msk, noise_scale=args.noise_scale, lr=lr, reducer=reducer,
                                             grad_scale=grad_scale)
            return loss
        if dp_on and args.no_overlap:
            graphed.replay()
            reducer.begin_step()
            reducer.finish()                                   # bucketed RCCL all-reduce (SUM) of the flat gradient
            opt.step(lr, grad_scale)
            return graphed.loss
        return graphed.replay(lr)

    def fence():
        if dp_on:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        one_step()
    fence()
    t0 = time.perf_counter()
    host_s = 0.0                                               # host time spent INSIDE the step calls (no sync in there)
    for _ in range(args.steps):
        th = time.perf_counter()
        loss = one_step()
        host_s += time.perf_counter() - th
    fence()
    elapsed = time.perf_counter() - t0
    rank_ms = [elapsed / args.steps * 1e3]
    rank_host_us = [host_s / args.steps * 1e6]
    if dp_on:
        # value uses the MAX over ranks; the per-rank spread (and the host cost of driving the segmented chain: 3-5 graph
        # launches + the collectives of a step from one thread) is reported beside it
        t = torch.tensor([elapsed, host_s], device="cuda", dtype=torch.float64)
        allt = [torch.empty_like(t) for _ in range(world)]
        dist.all_gather(allt, t)
        rank_ms = [float(a[0]) / args.steps * 1e3 for a in allt]
        rank_host_us = [float(a[1]) / args.steps * 1e6 for a in allt]
        elapsed = max(float(a[0]) for a in allt)
    final_loss = float(loss.item())
    if rank == 0 and args.dump_outputs:
        dump_outputs(args.dump_outputs, loss, eager_pred[0] if graphed is None else getattr(graphed, "pred", None), opt,
                     grad_scale)

    if rank == 0:
        ms = elapsed / args.steps * 1e3
        value = world * B * T_ar * args.steps / elapsed          # T_ar > 1: sample-steps/s
        out = {
            "metric": (f"PDE samples/sec ({res}^2 x10 -> 1 rollout step), {cname} train step" if T_ar == 1 else
                       f"PDE sample-steps/sec ({res}^2 x10 -> 1 per step, {T_ar}-step auto-regressive rollout), {cname} "
                       f"train step"),
            "value": round(value, 2), "unit": "samples/s" if T_ar == 1 else "sample-steps/s", "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": round(ms, 4), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None,
            "dtype": ("f32" if mlp_prec in (None, "f32") else f"f32 (channel-MLP GEMM operands {mlp_prec})")
                     + ("" if args.gemm_precision == "f32" else
                        f"; fp32 GEMMs >= 3 GFLOP as the fp32-accurate bf16x6 operand split (gemm_precision {args.gemm_precision})"),
            "data": "synthetic",
            "config": {"workload": f"{cname} (embed {ckw['embed_dim']}, depth {ckw['depth']}, n_blocks {ckw['n_blocks']}, "
                                   f"modes {ckw['modes']}, patch 8, mlp_ratio {ckw['mlp_ratio']}) on synthetic ns2d-shaped "
                                   f"{res}x{res}x10x4 fields, T_ar={T_ar}: fwd + rel-L2 loss + bwd + clip + Adam"
                                   + (f"; per-GPU batch {B} with activation recomputation (BASELINE configs[4] names no batch: "
                                      f"the largest power of two that fits 288 GB - batch 32 would need ~265 GB)"
                                      if args.config == "L20" else ""),
                       "baseline_config": cbase,
                       "per_gpu_batch": B, "global_batch": B * world, "parallelism": f"dp{world}",
                       "launch": mode, "noise_scale": args.noise_scale, "final_loss": round(final_loss, 5),
                       "gemm_precision": args.gemm_precision, "mlp_precision": mlp_prec or args.gemm_precision,
                       "activation_recomputation": (f"all but the last {keep_last} of {T_ar} AR steps" if recompute and keep_last
                                                    else recompute),
                       "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)},
        }
        out["config"]["host_us_per_step"] = round(max(rank_host_us), 1)
        if dp_on:
            out["config"]["collectives"] = {
                "backend": dist.get_backend(), "world_size": dist.get_world_size(),
                "library": ("gloo (DPOT_BENCH_DEBUG_GLOO=1: functional dry run, all ranks on cuda:0 - NOT a performance "
                            "number)") if debug_gloo else f"RCCL {'.'.join(map(str, torch.cuda.nccl.version()))} over xGMI"
                           + (" (DPOT_BENCH_FORCE_DP=1: ONE-rank communicator on a 1-GPU box - real calls into RCCL, which enqueues no device work for one rank)"
                              if force_dp else "")}
            out["config"]["per_rank"] = {"ms_per_step_min": round(min(rank_ms), 4), "ms_per_step_max": round(max(rank_ms), 4),
                                         "host_us_per_step_min": round(min(rank_host_us), 1),
                                         "host_us_per_step_max": round(max(rank_host_us), 1),
                                         "note": "host_us = wall time the rank's single host thread spends inside the step "
                                                 "call (graph launches, stream waits, collective enqueues); it must stay "
                                                 "below ms_per_step or the GPU starves"}
            out["config"]["buckets_MB"] = [round((hi - lo) * 4 / 1e6, 2) for lo, hi in reducer.ranges]
            out["config"]["dp_selection"] = dp_info
            out["config"]["dp"] = ("eager, hook-driven bucket all-reduce" if graphed is None else
                                   "one graph + all-reduce after backward" if args.no_overlap else
                                   f"ONE hipGraph holding the step and its {reducer.n_buckets} bucket all-reduces (side stream "
                                   f"forked inside the capture)" if isinstance(graphed, GraphedTrainStep) else
                                   f"segmented hipGraph chain ({len(graphed.graphs)} segments), bucket all-reduce on a "
                                   f"side stream overlapped with the remaining backward; {reducer.n_buckets} buckets")
        if args.full and not dp_on and graphed is not None and args.sustain_seconds > 0 and not args.brief:
            # the K-step figure above covers < 0.1 s of GPU time; a sustained run shows what the clocks settle at
            n_sus = max(args.steps, int(args.sustain_seconds / (elapsed / args.steps)))
            torch.cuda.synchronize()
            ts = time.perf_counter()
            for _ in range(n_sus):
                one_step()
            torch.cuda.synchronize()
            es = time.perf_counter() - ts
            out["sustained"] = {"steps": n_sus, "seconds": round(es, 3), "ms_per_step": round(es / n_sus * 1e3, 4),
                                "value": round(B * T_ar * n_sus / es, 2), "unit": out["unit"]}
        # whole-step FLOP rates per GPU: ALGORITHMIC = 3 x the forward FLOPs of the model as the reference computes it
        # (3 x 3.79 GFLOP per sample at DPOT-Tiny); EXECUTED = what this build's kernels actually run after
        # the embed fold (K 5120 -> 360), the grid-channel bias table and the three-product mixer (step_flops_per_sample)
        alg, exe, alg_mlp, exe_x6 = step_flops_per_sample(ckw, B)
        per_gpu = value / world
        if mlp_prec in (None, "f32"):
            out["model_flops_frac"] = round(alg * per_gpu / (FP32_MFMA_PEAK_TFLOPS * 1e12), 4)
            out["executed_flops_frac"] = round(exe * per_gpu / (FP32_MFMA_PEAK_TFLOPS * 1e12), 4)
            out["flops_note"] = (f"per sample-step: algorithmic {alg / 1e9:.2f} GFLOP (model_flops_frac, SURVEY 8d accounting), "
                                 f"executed {exe / 1e9:.2f} GFLOP (executed_flops_frac: what the chip's matrix pipes really do); "
                                 f"both priced against the {FP32_MFMA_PEAK_TFLOPS} TFLOP/s fp32 MFMA peak")
        else:
            # the ceiling of the mode that RUNS, on the FLOPs this build executes: channel MLP on the bf16
            # pipes (2.5 PF dense), the >= 3 GFLOP generic GEMMs of gemm_precision `auto` as six bf16 products per fp32 product
            # (2.5 PF / 6), everything else on the fp32 matrix pipes (157.3 TF).  A fraction of THIS ceiling cannot exceed 1.
            x6 = exe_x6 if args.gemm_precision in ("auto", "bf16x6") else 0.0
            t_exec = (alg_mlp / (BF16_MFMA_PEAK_TFLOPS * 1e12) + x6 * 6.0 / (BF16_MFMA_PEAK_TFLOPS * 1e12)
                      + (exe - alg_mlp - x6) / (FP32_MFMA_PEAK_TFLOPS * 1e12))
            out["mixed_ceiling"] = {"value": round(1.0 / t_exec, 1), "unit": out["unit"] + " per GPU",
                                    "executed_GFLOP": round(exe / 1e9, 2), "mlp_GFLOP_bf16": round(alg_mlp / 1e9, 2),
                                    "bf16x6_GFLOP": round(x6 / 1e9, 2)}
            out["frac_of_mixed_ceiling"] = round(per_gpu * t_exec, 4)
            # BASELINE.md section 4's figure (ALGORITHMIC FLOPs of the reference formulation: K = T*E time aggregation etc., MLP
            # share at 2.5 PF, the rest at 157.3 TF) - this build executes fewer fp32 FLOPs than that formulation, so the ratio to
            # it is a speed ratio, not a fraction (it can exceed 1: DPOT-S)
            t_ceiling = alg_mlp / (BF16_MFMA_PEAK_TFLOPS * 1e12) + (alg - alg_mlp) / (FP32_MFMA_PEAK_TFLOPS * 1e12)
            out["baseline_md_ceiling"] = round(1.0 / t_ceiling, 1)
            out["x_of_baseline_md_ceiling"] = round(per_gpu * t_ceiling, 4)
        if args.full:
            try:
                mix = mixer_roofline(model, B)
                if mlp_prec == "bf16" and not headline:
                    # the dominant kernel of these configs is the bf16 panel GEMM; the mixer goes to other_kernels
                    out["roofline"] = bf16_mlp_roofline(model, B)
                    others = mix.pop("other_kernels", [])
                    out["roofline"]["other_kernels"] = [mix] + others
                else:
                    out["roofline"] = mix
            except Exception as e:                             # pragma: no cover
                log(f"[bench] roofline probe failed: {e}")
                out["roofline"] = None
        if args.full and not headline and not dp_on and graphed is not None and args.gemm_precision == "auto" \
                and not args.no_alt:
            # the bf16-channel-MLP configs run `auto`; the same step with every fp32 GEMM on native fp32 MFMA, beside it
            try:
                model.gemm_precision = "f32"
                g2 = GraphedTrainStep(model, opt, xx, yy, msk, noise_scale=args.noise_scale, warmup=1 if T_ar > 1 else 2)
                for _ in range(args.warmup):
                    g2.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    g2.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                e2 = time.perf_counter() - t1
                out["gemm_f32"] = {"gemm_precision": "f32 (native fp32 MFMA for every GEMM outside the channel MLP)",
                                   "value": round(B * T_ar * args.steps / e2, 2), "ms_per_step": round(e2 / args.steps * 1e3, 4)}
                del g2
            except Exception as e:                             # pragma: no cover
                log(f"[bench] gemm_f32 timing failed: {e}")
            finally:
                model.gemm_precision = args.gemm_precision
        if args.full and args.config in ("M", "L") and not dp_on and graphed is not None and mlp_prec == "bf16" \
                and not args.no_alt:
            # BASELINE configs[3] / [4] do not say bf16 (only configs[2] does): the SAME step with every GEMM on native fp32
            # MFMA - channel MLP included - i.e. the figure inside north_star's rtol 1e-4 (the parity gate of this mode:
            # tests/test_gpu_sizes.py::test_vs_reference_golden, fp32 leg).  Fresh model / optimiser / graph: weight packs and
            # kernel choices are per mode; the bf16 objects are released first (DPOT-L at batch 16 wants the HBM to itself)
            try:
                import gc
                graphed = None
                model = opt = fp = None
                gc.collect()
                torch.cuda.empty_cache()
                torch.manual_seed(0)
                m32 = DPOTNet(**ckw).cuda()
                m32.mlp_precision = m32.gemm_precision = "f32"
                m32.recompute_blocks = recompute
                o32 = FusedAdam(FlatParams(m32), lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=10000.0)
                g32 = GraphedTrainStep(m32, o32, xx, yy, msk, noise_scale=args.noise_scale, warmup=2)
                n32 = max(3, args.steps // 2)
                for _ in range(2):
                    g32.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(n32):
                    l32 = g32.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                e32 = time.perf_counter() - t1
                alg32 = step_flops_per_sample(ckw, B)[0]
                v32 = B * T_ar * n32 / e32
                out["all_f32"] = {"what": "the same train step with mlp_precision = f32 and gemm_precision = f32: every GEMM on "
                                          "native fp32 MFMA, inside north_star's rtol 1e-4",
                                  "value": round(v32, 2), "unit": out["unit"], "ms_per_step": round(e32 / n32 * 1e3, 4),
                                  "steps": n32, "final_loss": round(float(l32.item()), 5),
                                  "model_flops_frac": round(alg32 * v32 / (FP32_MFMA_PEAK_TFLOPS * 1e12), 4),
                                  "peak_mem_GB": round(torch.cuda.max_memory_allocated() / 2 ** 30, 2)}
                del g32, m32, o32
            except Exception as e:                             # pragma: no cover
                log(f"[bench] all_f32 timing failed: {type(e).__name__}: {e}")
        if args.full and headline and not dp_on and graphed is not None and args.gemm_precision == "f32" \
                and not args.no_alt and not args.brief:
            # not the headline: the same step with the large GEMMs on the bf16x6 kernel (fp32 emulated by operand
            # splitting on the bf16 matrix cores, same accuracy class - DESIGN.md "bf16x6"); a fresh graph is captured
            # because the kernel choice is baked in at capture time
            try:
                model.gemm_precision = "auto"
                g2 = GraphedTrainStep(model, opt, xx, yy, msk, noise_scale=args.noise_scale, warmup=2)
                for _ in range(args.warmup):
                    g2.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for _ in range(args.steps):
                    l2 = g2.replay(lr_at(step_idx[0]))
                torch.cuda.synchronize()
                e2 = time.perf_counter() - t1
                out["gemm_auto"] = {"gemm_precision": "auto (bf16x6 for GEMMs >= 3 GFLOP, native fp32 MFMA below)",
                                    "value": round(B * args.steps / e2, 2), "ms_per_step": round(e2 / args.steps * 1e3, 4),
                                    "final_loss": round(float(l2.item()), 5),
                                    "note": "reported beside the headline, which uses native fp32 MFMA everywhere"}
            except Exception as e:                             # pragma: no cover
                log(f"[bench] gemm_auto timing failed: {e}")
            finally:
                model.gemm_precision = args.gemm_precision
        if args.full and not dp_on and T_ar == 1 and not args.brief:
            # forward-only (inference) rate of the same batch, SURVEY 8(d): no_grad forward, hipGraph replay
            try:
                with torch.no_grad():
                    for _ in range(2):
                        model(xx)
                    torch.cuda.synchronize()
                    gi = torch.cuda.CUDAGraph()
                    with torch.cuda.graph(gi):
                        pred_i, _ = model(xx)
                    for _ in range(args.warmup):
                        gi.replay()
                    torch.cuda.synchronize()
                    t2 = time.perf_counter()
                    for _ in range(args.steps):
                        gi.replay()
                    torch.cuda.synchronize()
                    e3 = time.perf_counter() - t2
                out["inference"] = {"value": round(B * args.steps / e3, 2), "unit": "samples/s",
                                    "ms_per_batch": round(e3 / args.steps * 1e3, 4),
                                    "what": "DPOTNet forward only (no_grad), batch %d, hipGraph replay" % B}
            except Exception as e:                             # pragma: no cover
                log(f"[bench] inference timing failed: {e}")
        if args.full and headline and not dp_on and graphed is not None and not args.no_pipeline and not args.brief:
            # input-pipeline-inclusive rate (never `value`): raw 64x64 single-channel trajectories in host memory (the
            # ns2d_fno_1e-5 shape) -> pinned staging -> ONE H2D copy per batch on a copy stream -> device-side bilinear
            # resize to 128^2 + channel pad with ones + temporal window (csrc/data.hip) -> double-buffered batch slots;
            # the step reads slot k while slot k+1 is filled (dpot_amd/data.py)
            try:
                import numpy as np
                from dpot_amd.data import DeviceBatcher, random_window_start
                Traw = 20
                rng = np.random.default_rng(0)
                gx = np.linspace(0, 1, 64, dtype=np.float32)
                pool = [np.ascontiguousarray((np.sin(6 * gx[:, None, None] + i) * np.cos(4 * gx[None, :, None] + 0.3 * i)
                                              * np.linspace(1, 2, Traw, dtype=np.float32)[None, None, :])[..., None])
                        for i in range(4 * B)]
                db = DeviceBatcher(B, 128, 10, 1, 4, max_raw_floats_per_sample=64 * 64 * Traw)
                pick = lambda: ([pool[int(rng.integers(len(pool)))] for _ in range(B)],
                                [random_window_start(Traw, 10, 1, rng) for _ in range(B)])
                db.submit(*pick())
                n_pipe = max(args.steps, 40)
                torch.cuda.synchronize()
                tp = time.perf_counter()
                for _ in range(n_pipe):
                    db.submit(*pick())
                    bx, by, bm = db.get()
                    graphed.stage(bx, by, bm)
                    db.release()
                    one_step()
                torch.cuda.synchronize()
                ep = time.perf_counter() - tp
                out["pipeline_inclusive"] = {
                    "value": round(B * n_pipe / ep, 2), "unit": "samples/s", "ms_per_step": round(ep / n_pipe * 1e3, 4),
                    "steps": n_pipe, "h2d_MB_per_batch": round(db.h2d_bytes / (n_pipe + 1) / 1e6, 2),
                    "what": "host raw [64,64,20,1] samples -> pinned -> H2D (copy stream) -> device resize/pad/window "
                            "(double buffered) -> staged into the step's graph inputs -> train step; PCIe + host "
                            "batching inclusive, single host thread"}
            except Exception as e:                             # pragma: no cover
                log(f"[bench] pipeline-inclusive timing failed: {type(e).__name__}: {e}")
        if args.full and headline and not dp_on and not args.skip_cpu_baseline and not args.brief:
            out["cpu_baseline"] = cpu_baseline(args.cpu_seconds)
            out["speedup_vs_cpu_baseline"] = round(value / out["cpu_baseline"]["value"], 1)
        if args.full and headline and not dp_on and not args.brief and not args.no_other_configs and args.batch is None:
            # BASELINE configs[2..4] through this same script, so that the driver's record carries them:
            # the model of this process is released first - DPOT-L at batch 16 wants the HBM to itself
            del graphed, model, opt, fp
            torch.cuda.empty_cache()
            out["other_configs"] = other_configs(args)
        log("[bench-full] " + json.dumps(out))
        if args.full_json:
            with open(args.full_json, "w") as f:
                json.dump(out, f, indent=1)
        final_line = json.dumps(compact_line(out), separators=(",", ":"))
    if dp_on:
        dist.barrier()
        dist.destroy_process_group()
    # the JSON line is the LAST thing on stdout: RCCL prints its version banner through C stdio, which - stdout being a pipe -
    # sits in the C library's buffer until it is flushed; flush it (every rank) before rank 0 prints
    _flush_c_stdio()
    if rank == 0:
        if dp_on and world > 1:
            time.sleep(0.5)                                    # the other ranks' flushes land first
        print(final_line, flush=True)


class _GraphedFwdBwd:
    """hipGraph of zero_grad + rollout + loss + backward for a fixed batch (the N>1 path: collectives stay eager)."""

    def __init__(self, model, opt, xx, yy, msk, noise_scale):
        from dpot_amd.train import rollout
        self.opt = opt

        def body():
            opt.zero_grad()
            loss, _ = rollout(model, xx, yy, msk, 1, noise_scale)
            loss.backward()
            return loss.detach()

        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                body()
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: the RCCL watchdog thread of the process group may touch the HIP runtime while this thread is
        # capturing; only this thread's calls may invalidate the capture
        with torch.cuda.graph(self.graph, capture_error_mode="thread_local"):
            self.loss = body()

    def replay(self):
        self.graph.replay()


if __name__ == "__main__":
    main()
