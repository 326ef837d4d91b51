"""The one owner of a model's weight-derived copies (``model.packs``): the AFNO packs (ops.AfnoPacks) of all three models and, for a
DPOTNet, the embed grid matrix, the small layout pieces (ops.LayoutJobs), the de-embed matrix and the panel GEMM weight packs
(ops.PanelPacks: fp32 channel MLP + de-embed, bf16, bf16x6).  Each job table is rebuilt only when the tensors it points at move
(``_where``).

Freshness rule: every forward (or once per ``DPOTNet.weights_scope()``) refreshes every set, except the one set the optimiser
last wrote itself (train.FusedAdam -> dpot_adam_step_packs) while that write is current: same FlatParams epoch, same tensor
versions of the set's sources.  Any other change of the parameters breaks it: an optimiser step or restore, load_state_dict
(tensor versions), ``FlatParams.touch()`` after a write the versions do not see.
"""
from __future__ import annotations

import contextlib

import torch

from . import _lib, ops
from .functional import (embed_derived, embed_grid_matrix, embed_implicit_tables, embed_layout_jobs, head_derived,
                         head_layout_jobs, mlp_pack_kind)


def _where(*tensors):
    """placement key of a table over these tensors: it holds their raw pointers"""
    return tuple((t.device, t.data_ptr()) for t in tensors if t is not None)


class ModelPacks:
    def __init__(self):
        self.tables = {}       # name -> (placement key, object): grid, layout, afno, wt, f32, bf16, bf16x6
        self.depth, self.held = 0, None          # weights_scope nesting, derive() result held inside it
        self.fresh = None      # (PanelPacks, FlatParams, token) of the optimiser's last pack write
        self.plan = None       # (PanelPacks, flat address, n_active, AdamPackPlan | None)

    def get(self, name: str):
        return self.tables.get(name, (None, None))[1]

    def _table(self, name: str, key, make):
        if self.get(name) is None or self.tables[name][0] != key:
            self.tables[name] = (key, make())
        return self.tables[name][1]

    # -- freshness ------------------------------------------------------------------------------------
    @staticmethod
    def _token(pp, fp):
        return fp.epoch, tuple(j[0]._version for j in pp.jobs[::2])

    def is_fresh(self, pp) -> bool:
        f = self.fresh
        return f is not None and f[0] is pp and f[2] == self._token(pp, f[1])

    def mark_fresh(self, pp, fp) -> None:
        """the optimiser has just written `pp` from the parameters of `fp` (eagerly, or in a graph replay)"""
        self.fresh = (pp, fp, self._token(pp, fp))

    def ensure_fresh(self, pp) -> None:
        if not self.is_fresh(pp):
            pp.refresh()

    def adam_plan(self, flat, n_active: int):
        """the dpot_adam_step_packs tables that let the optimiser write the plain-bf16 channel-MLP packs (made by the first
        forward in that mode), or None: no such packs / a weight that does not tile / DPOT_TUNE packs=0"""
        pp = self.get("bf16")
        if ops.tune("packs") == 0 or pp is None:
            return None
        if self.plan is None or self.plan[:3] != (pp, flat.data_ptr(), n_active):
            self.plan = (pp, flat.data_ptr(), n_active, ops.AdamPackPlan.build(flat, n_active, pp))
        return self.plan[3]

    # -- weights_scope ----------------------------------------------------------------------------------
    @contextlib.contextmanager
    def scope(self, m):
        self.depth += 1
        if self.depth == 1:
            self.held = None
            if m.pos_embed.is_cuda:
                with ops.precision_scope(m.gemm_precision, m.mlp_precision):
                    self.derive(m, defer=True)       # the first pass's EmbedFn.forward joins the side lane
        try:
            yield
        finally:
            self.depth -= 1
            if self.depth == 0:
                self.held = None
                ops.side_lane_join()                 # a scope that ran no forward

    # -- the AFNO packs of any of the three models ---------------------------------------------------------
    def afno(self, m):
        """the ops.AfnoPacks of m.blocks: Wbig = [[Wr, Wi], [-Wi, Wr]] of every AFNO layer + its fragment-block-major forms in
        persistent buffers that ``.refresh()`` re-fills in ONE launch for all layers (so a captured forward replays the refresh
        with the weights of the day)"""
        pairs = [p for blk in m.blocks for p in ((blk.filter.w1, blk.filter.b1), (blk.filter.w2, blk.filter.b2))]

        def make():
            if torch.cuda.is_current_stream_capturing():
                raise _lib.DpotHipError(f"{type(m).__name__}: run one forward before capturing (the weight-pack tables are "
                                        "built by it)")
            return ops.AfnoPacks(pairs)
        return self._table("afno", _where(*(t for p in pairs for t in p)), make)

    # -- the derived weights of one DPOTNet forward -------------------------------------------------------
    def derive(self, m, defer: bool = False):
        """-> (embed products, AFNO items, head products + (de-embed packs,), channel-MLP packs per block | None)

        Side-lane site `weights` (ops.side_lane): only the layout jobs, `embed_pack_w0` and the bias-table GEMM feed `embed_fwd`
        and go to the caller's stream; the scaled aggregation weights, the V and c products, the AFNO packs, the de-embed
        transpose and the panel packs are first read by the fold GEMM and go to the lane.  Every table is built before the fork
        (building one runs torch ops).  defer: return with the lane still forked - the caller's EmbedFn.forward joins."""
        if self.depth > 0 and self.held is not None:
            return self.held
        pe, ta, ol = m.patch_embed.proj, m.time_agg_layer, m.out_layer
        grid = None
        if ops.embed_supported(m.in_channels, m.patch_size, m.in_timesteps, pe[0].weight.shape[0], m.img_size // m.patch_size):
            grid = self._table("grid", _where(m._gx), lambda: embed_grid_matrix(
                m._gx, m._gy, m._gt, m.img_size, m.img_size, m.in_timesteps, m.in_channels, m.patch_size))
        # every small layout piece of the model (padded conv weights, pos_embed^T + bias, de-embed bias per pixel, padded
        # tail weights) in ONE launch
        lay_e = lay_h = None
        if ops.tune("fused_small") != 0:
            je = embed_layout_jobs(m.pos_embed, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias)
            jobs = je + head_layout_jobs(ol[0].bias, ol[4].weight, ol[4].bias, m.patch_size, ol[0].weight.shape[1])
            lay = self._table("layout", _where(*(j[k] for k in (0, 1) for j in jobs)), lambda: ops.LayoutJobs(jobs)).refresh()
            lay_e, lay_h = lay[:len(je)], lay[len(je):]
        afno = self.afno(m) if len(m.blocks) else None
        w0 = ol[0].weight
        wt = self._table("wt", _where(w0), lambda: w0.new_empty(m.embed_dim, m.patch_size ** 2 * w0.shape[1]))
        stale = []
        mlp_pk, head_pk = self._panels(m, wt, stale)
        eargs = (m.pos_embed, pe[0].weight, pe[0].bias, pe[2].weight, pe[2].bias, ta.w, m._time_agg_gamma(), m._tt,
                 m.in_timesteps)
        side = lay_e is not None and ops.side_lane_enabled("weights")     # the lane's products read the layout pieces
        with ops.side_lane("weights", on=side, join=False):
            emb = embed_derived(*eargs, grid=grid, layouts=lay_e, implicit_tables=not side)
            pk = afno.refresh() if afno is not None else []
            head = head_derived(w0, ol[0].bias, ol[4].weight, ol[4].bias, m.patch_size, wt_out=wt, layouts=lay_h)
            for pp in stale:
                pp.refresh()
        if side and grid is not None:
            emb = emb[:8] + embed_implicit_tables(pe[0].weight, emb[0], emb[1], grid) + emb[10:]
        if not defer:
            ops.side_lane_join()
        d = (emb, pk, head + (head_pk,), mlp_pk)
        if self.depth > 0:
            self.held = d
        return d

    def _panels(self, m, wt, stale):
        """fragment-block-major copies of the static weights of the panel GEMMs, ONE launch per set: per block W1, W1^T,
        W2, W2^T (channel-MLP forward x W^T and data gradient dy W) - fp32 for csrc/gemm_panel.hip, or bf16 / bf16x6 for
        csrc/gemm_bf16p.hip by the channel-MLP precision - and the de-embed matrix wt [E, P*P*old] both ways (fp32).
        Returns (per-block MlpPacks | None, (wt fwd, wt bwd) | None); the sets to refresh are appended to `stale`."""
        E, n_out, nb = m.embed_dim, wt.shape[1], len(m.blocks)
        ws = [b.mlp[i].weight for b in m.blocks for i in (0, 2)]            # [mh, E, 1, 1], [E, mh, 1, 1] per block
        mlp_pk = head_pk = None

        def mlp_jobs():
            mh = ws[0].shape[0]
            return [j for w1, w2 in zip(ws[::2], ws[1::2])
                    for j in ((w1, mh, E, E, False), (w1, E, mh, E, True), (w2, E, mh, mh, False), (w2, mh, E, mh, True))]

        def panel(name, key, jobs, bf16, planes=1):          # key: the set's placement beyond ws + its mode flags
            pp = self._table(name, _where(*ws) + key, lambda: ops.PanelPacks(jobs(), bf16=bf16, planes=planes))
            if not self.is_fresh(pp):
                stale.append(pp)
            return pp

        kind = mlp_pack_kind(E, ws[0].shape[0]) if nb else None
        if kind in ("bf16", "bf16x6"):
            pp = panel(kind, (kind,), mlp_jobs, True, 3 if kind == "bf16x6" else 1)
            mlp_pk = [ops.MlpPacks(pp.bufs[4 * i:4 * i + 4], kind) for i in range(nb)]
        f32_mlp = kind == "f32"
        use_head = ops.panel_enabled() and ops.gemm_panel_supported(1, n_out, E) and ops.gemm_panel_supported(1, E, n_out)
        if f32_mlp or use_head:
            head_jobs = [(wt, n_out, E, n_out, True), (wt, E, n_out, n_out, False)] if use_head else []
            pp = panel("f32", _where(wt) + (f32_mlp, use_head), lambda: (mlp_jobs() if f32_mlp else []) + head_jobs, False)
            n0 = 4 * nb if f32_mlp else 0
            if f32_mlp:
                mlp_pk = [ops.MlpPacks(pp.bufs[4 * i:4 * i + 4], "f32") for i in range(nb)]
            if use_head:
                head_pk = tuple(pp.bufs[n0:n0 + 2])
        return mlp_pk, head_pk
