#!/usr/bin/env python
"""Time the 3-D fine-tuning step and the three index kernels at its ends (csrc/patch3d.hip: ops.patchify3 / unpatchify3 /
fold3) against the torch compositions they replace.

    python scripts/finetune3d_time.py [--reps 20] [--out profiles/finetune3d.txt]

Windows [B, S^3, T, C]: [4, 64^3, 10, 4] (the reference's fine-tuning shape), [1, 64^3, 10, 4], [4, 32^3, 10, 4]; patch 8,
E = 512, depth 4, out_layer_dim 32, modes 32.
Yardsticks, kept here: the patch matrix from torch.stack / expand / cat and a 9-axis permute copy, its adjoint as one strided
copy, and functional._unfold3 / _fold3 - how DPOTNet3D ran before the kernels (``BeforeModel`` is that forward).
Per kernel: a hipGraph of `reps` launches between two events, median of 5 replays; microseconds, yardstick over ours, and the
algorithmic bytes (every input element read once, every output element written once) over the time as a fraction of the
copy rate MEASURED in the same run (a 1 GiB device copy: read + write).  Stages and steps: `reps` eager calls between two
events after a warm-up, median of 5, autograd included; the graphed step: replays of a GraphedTrainStep.  Peak memory:
torch.cuda.max_memory_allocated over one eager T_ar = 3 rollout + backward, minus what was allocated before it."""
from __future__ import annotations

import argparse
import gc
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from dpot_amd import DPOTNet3D, ops, train  # noqa: E402
from dpot_amd.functional import (EPI_ACT, Head3DFn, Mlp2Fn, PatchEmbed3DFn, TimeAggFn, _fold3, _unfold3,  # noqa: E402
                                 block3d)

SHAPES = [(4, 64), (1, 64), (4, 32)]
T, C, P, E, DEPTH, OLD = 10, 4, 8, 512, 4, 32


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


def time_eager(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()

    def run():
        for _ in range(reps):
            fn()
    return median5(run, reps)


# ---- the torch compositions (the parent's code) ----------------------------------------------------------------------------
def patch_matrix(x, gs, gt, P):
    B, S, _, _, T, Cin = x.shape
    h = S // P
    grid = torch.stack([gs.view(S, 1, 1, 1).expand(S, S, S, T), gs.view(1, S, 1, 1).expand(S, S, S, T),
                        gs.view(1, 1, S, 1).expand(S, S, S, T), gt.view(1, 1, 1, T).expand(S, S, S, T)], dim=-1)
    Cc = Cin + 4
    xg = torch.cat([x, grid.unsqueeze(0).expand(B, S, S, S, T, 4)], dim=-1)
    return xg.view(B, h, P, h, P, h, P, T, Cc).permute(0, 7, 1, 3, 5, 8, 2, 4, 6).reshape(B * T * h ** 3, Cc * P ** 3)


def patch_matrix_adjoint(dA, B, S, T, Cin, P):
    """what autograd makes of patch_matrix's backward: views of dA, and ONE strided copy where a kernel needs it contiguous"""
    h = S // P
    return dA.view(B, T, h, h, h, Cin + 4, P, P, P).permute(0, 2, 6, 3, 7, 4, 8, 1, 5).reshape(B, S, S, S, T, Cin + 4)[
        ..., :Cin].contiguous()


class HeadBefore(torch.autograd.Function):
    """functional.Head3DFn with the torch folds"""

    @staticmethod
    def forward(ctx, x, W0, b0e, W2, b2, W4, b4, B, h, P, act):
        ops.capture_precision(ctx)
        x, W0, W2, W4 = x.contiguous(), W0.contiguous(), W2.contiguous(), W4.contiguous()
        M, E_ = x.shape
        old = W2.shape[0]
        N0 = old * P ** 3
        H1 = torch.empty(M, N0, dtype=torch.float32, device=x.device)
        H1pre = torch.empty_like(H1)
        ops.gemm(x, W0, H1, M, N0, E_, lda=E_, ldb=N0, ldc=N0, bias=b0e.contiguous(), act=act, mode=EPI_ACT, preact=H1pre,
                 ldpre=N0)
        H1p, H1pre_p = _unfold3(H1, B, h, P, old), _unfold3(H1pre, B, h, P, old)
        del H1, H1pre
        H2, H2pre = ops.linear_fwd(H1p, W2, b2, act=act, save_pre=True)
        out, _ = ops.linear_fwd(H2, W4, b4)
        ctx.save_for_backward(x, W0, W2, W4, H1p, H1pre_p, H2, H2pre)
        ctx.dims = (B, h, P, old, act)
        return out

    @staticmethod
    @ops.with_ctx_precision
    def backward(ctx, dout):
        x, W0, W2, W4, H1p, H1pre_p, H2, H2pre = ctx.saved_tensors
        B, h, P, old, act = ctx.dims
        M, E_ = x.shape
        N0 = old * P ** 3
        dout = dout.contiguous()
        dH2pre = ops.linear_bwd_data(dout, W4, act=act, aux=H2pre)
        dW4, db4 = ops.linear_bwd_wb(dout, H2)
        dH1pre_p = ops.linear_bwd_data(dH2pre, W2, act=act, aux=H1pre_p)
        dW2, db2 = ops.linear_bwd_wb(dH2pre, H1p)
        dH1pre = _fold3(dH1pre_p, B, h, P, old)
        dW0 = torch.empty(E_, N0, dtype=torch.float32, device=x.device)
        ops.gemm(x, dH1pre, dW0, E_, N0, M, transA=True, lda=E_, ldb=N0, ldc=N0, splitk=ops.auto_splitk(E_, N0, M, tn=True))
        db0e = ops.colsum(dH1pre, M, N0)
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty(M, E_, dtype=torch.float32, device=x.device)
            ops.gemm(dH1pre, W0, dx, M, E_, N0, transB=True, lda=N0, ldb=N0, ldc=E_)
        return dx, dW0, db0e, dW2, db2, dW4, db4, None, None, None, None


class Stages:
    """the three stages of DPOTNet3D._forward (normalize=False), each callable on its own; before=True: the torch compositions"""

    def __init__(self, m, before):
        self.m, self.before = m, before

    def embed(self, x):
        m = self.m
        B, S = x.shape[0], x.shape[1]
        h = S // P
        tok, Cc = h ** 3, C + 4
        pe, ta = m.patch_embed.proj, m.time_agg_layer
        hid = pe[0].weight.shape[0]
        posT = m.pos_embed.view(E, tok).t()
        W1, W2 = pe[0].weight.view(hid, Cc * P ** 3), pe[2].weight.view(E, hid)
        if self.before:
            z = Mlp2Fn.apply(patch_matrix(x, m._gs, m._gt, P), W1, pe[0].bias, W2, pe[2].bias, m._act, posT, tok)
        else:
            z = PatchEmbed3DFn.apply(x, m._gs, m._gt, W1, pe[0].bias, W2, pe[2].bias, posT, P, m._act)
        A1 = z.view(B, T, tok, E).permute(0, 2, 1, 3).reshape(B * tok, T * E)
        return TimeAggFn.apply(A1, ta.w, ta.gamma, m._tt).view(B, tok, E)

    def blocks(self, lat):
        m = self.m
        h = round(lat.shape[1] ** (1 / 3))
        pk = m.packs.afno(m).refresh()
        for i, blk in enumerate(m.blocks):
            f = blk.filter
            lat = block3d(lat, blk.norm1.weight, blk.norm1.bias, f.w1, f.b1, f.w2, f.b2, blk.norm2.weight, blk.norm2.bias,
                          blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias, (h, h, h), m.n_blocks,
                          m.modes, m._act, (pk[2 * i], pk[2 * i + 1]))
        return lat

    def head(self, lat):
        m = self.m
        B, tok, _ = lat.shape
        h = round(tok ** (1 / 3))
        ol = m.out_layer
        fn = HeadBefore if self.before else Head3DFn
        pred = fn.apply(lat.reshape(B * tok, E), ol[0].weight.view(E, OLD * P ** 3),
                        ol[0].bias.view(OLD, 1).expand(OLD, P ** 3).reshape(-1), ol[2].weight.view(OLD, OLD), ol[2].bias,
                        ol[4].weight.view(C, OLD), ol[4].bias, B, h, P, m._act)
        return pred.view(B, h * P, h * P, h * P, 1, C)

    def __call__(self, x):
        with ops.precision_scope(self.m.gemm_precision, None):
            return self.head(self.blocks(self.embed(x)))


class BeforeModel(torch.nn.Module):
    """DPOTNet3D's parameters behind the forward of the parent commit (one tensor out, so train.rollout takes it)"""
    cls_output = False

    def __init__(self, m):
        super().__init__()
        self.m, self.run = m, Stages(m, True)

    def forward(self, x):
        return self.run(x)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finetune3d.txt"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("finetune3d_time: needs the GPU (nothing is measured without one)")
    dev, reps = "cuda", args.reps
    lines = [f"device: {torch.cuda.get_device_name(0)}   reps {reps}, median of 5   window [B,S^3,{T},{C}], patch {P}, "
             f"E {E}, depth {DEPTH}, out_layer_dim {OLD}"]
    big = torch.empty(1 << 28, device=dev)
    big2 = torch.empty_like(big)
    rate = 2.0 * big.numel() * 4 / (time_graph(lambda: big2.copy_(big), 10) * 1e-6)
    lines.append(f"measured copy rate (1 GiB read + 1 GiB write): {rate / 1e12:.2f} TB/s")
    del big, big2

    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def emit(s):
        lines.append(s)
        print(s, flush=True)
        with open(args.out, "w") as f:                     # the record as far as the run got
            f.write("\n".join(lines) + "\n")

    for B, S in SHAPES:
        torch.manual_seed(0)
        h = S // P
        tok = h ** 3
        shape = f"[{B},{S}^3,{T},{C}]"
        m = DPOTNet3D(img_size=S, patch_size=P, in_channels=C, out_channels=C, in_timesteps=T, out_timesteps=1, n_blocks=8,
                      embed_dim=E, out_layer_dim=OLD, depth=DEPTH, modes=32, mlp_ratio=1.).to(dev)
        x = torch.randn(B, S, S, S, T, C, device=dev)
        gs, gt = m._gs, m._gt
        emit(f"--- {shape}: kernels against the torch compositions")
        emit(f"{'op':30s} {'ours us':>10s} {'torch us':>10s} {'torch/ours':>10s} {'MB':>8s} {'of copy rate':>12s}")
        A = ops.patchify3(x, gs, gt, P)
        assert torch.equal(A, patch_matrix(x, gs, gt, P))
        dA = torch.randn_like(A)
        assert torch.equal(ops.unpatchify3(dA, B, S, T, C, P), patch_matrix_adjoint(dA, B, S, T, C, P))
        Hm = torch.randn(B * tok, OLD * P ** 3, device=dev)
        Hp = ops.fold3(Hm, B, h, P, OLD)
        assert torch.equal(Hp, _unfold3(Hm, B, h, P, OLD)) and torch.equal(ops.fold3(Hp, B, h, P, OLD, inverse=True), Hm)
        nx, nA, nH = 4.0 * x.numel(), 4.0 * A.numel(), 4.0 * Hm.numel()
        for what, ours, yard, nbytes in (
                ("patchify3", lambda: ops.patchify3(x, gs, gt, P), lambda: patch_matrix(x, gs, gt, P), nx + nA),
                ("unpatchify3", lambda: ops.unpatchify3(dA, B, S, T, C, P), lambda: patch_matrix_adjoint(dA, B, S, T, C, P),
                 2 * nx),
                ("fold3", lambda: ops.fold3(Hm, B, h, P, OLD), lambda: _unfold3(Hm, B, h, P, OLD), 2 * nH),
                ("fold3 inverse", lambda: ops.fold3(Hp, B, h, P, OLD, inverse=True), lambda: _fold3(Hp, B, h, P, OLD), 2 * nH)):
            to, ty = time_graph(ours, reps), time_graph(yard, reps)
            emit(f"{what:30s} {to:10.1f} {ty:10.1f} {ty / to:10.2f} {nbytes / 1e6:8.1f} {nbytes / (to * 1e-6) / rate:12.3f}")
        del A, dA, Hm, Hp

        emit(f"--- {shape}: eager forward + backward by stage (first AR step: the window carries no gradient), us")
        emit(f"{'stage':30s} {'kernels':>10s} {'torch':>10s} {'torch/kernels':>13s}")
        after, before = Stages(m, False), Stages(m, True)
        with torch.no_grad():
            lat0 = after.embed(x)
            assert torch.equal(lat0, before.embed(x))
            lat1 = after.blocks(lat0)
            out = after.head(lat1)
            assert torch.equal(out, before.head(lat1))
        glat, gout = torch.randn_like(lat0), torch.randn_like(out)
        latg = lat0.clone().requires_grad_(True)
        lat1g = lat1.clone().requires_grad_(True)

        def fb(fn, inp, g):
            def run():
                m.zero_grad(set_to_none=True)
                inp.grad = None
                fn(inp).backward(g)
            return run

        tot = {}
        for stage, inp, g in (("embed", x, glat), ("blocks", latg, glat), ("head", lat1g, gout)):
            ta_ = time_eager(fb(getattr(after, stage), inp, g), reps)
            tb_ = time_eager(fb(getattr(before, stage), inp, g), reps) if stage != "blocks" else ta_
            tot[stage] = (ta_, tb_)
            emit(f"{stage:30s} {ta_:10.1f} {tb_:10.1f} {tb_ / ta_:13.2f}")
        ta_, tb_ = time_eager(fb(after, x, gout), reps), time_eager(fb(before, x, gout), reps)
        emit(f"{'whole forward + backward':30s} {ta_:10.1f} {tb_:10.1f} {tb_ / ta_:13.2f}")
        del lat0, lat1, out, glat, gout, latg, lat1g

        emit(f"--- {shape}: train step, T_ar = 3, T_bundle = 1, noise_scale 0.01, FusedAdam with clip")
        yy = torch.randn(B, S, S, S, 3, C, device=dev)
        msk = torch.ones(B, S, S, S, 1, C, device=dev)
        opt = train.FusedAdam(train.FlatParams(m), lr=1e-4, max_norm=1.0)
        bm = BeforeModel(m)
        peak = {}
        for tag, model in (("kernels", m), ("torch", bm)):
            opt.zero_grad()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            base = torch.cuda.memory_allocated()
            loss, pred, total = train.rollout_total(model, x, yy, msk, 1, 0.01)
            total.backward()
            torch.cuda.synchronize()
            peak[tag] = (torch.cuda.max_memory_allocated() - base) / 2 ** 20
            # nothing of this autograd graph may outlive the block: its AccumulateGrad nodes belong to the current stream, and a
            # node that survives into the graphed step's capture on another stream takes the legacy stream into the capture
            del loss, pred, total
        emit(f"peak memory of one rollout + backward above the resident state: kernels {peak['kernels']:.0f} MiB, "
             f"torch {peak['torch']:.0f} MiB")
        te = time_eager(lambda: train.train_step(m, opt, x, yy, msk, noise_scale=0.01, lr=1e-4), max(3, reps // 4))
        tb = time_eager(lambda: train.train_step(bm, opt, x, yy, msk, noise_scale=0.01, lr=1e-4), max(3, reps // 4))
        gc.collect()
        gstep = train.GraphedTrainStep(m, opt, x, yy, msk, T_bundle=1, noise_scale=0.01, warmup=1)
        tg = time_eager(lambda: gstep.replay(1e-4), max(3, reps // 4))
        emit(f"eager step: kernels {te:.0f} us, torch {tb:.0f} us ({tb / te:.2f}x);  graphed step (kernels): {tg:.0f} us "
             f"({te / tg:.2f}x the eager step)")
        del gstep, opt, bm, m, x, yy, msk, after, before
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
