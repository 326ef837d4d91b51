"""Descriptor-level yardstick of dpot_gemm_f32 (include/dpot_hip.h): a table of small descriptors that reaches every dispatch
path of csrc/gemm.hip / gemm_split.h / gemm_epi.h and the hand-off to gemm_tn_kernel, host buffers laid out exactly as each
descriptor says, and a float64 restatement of the header's epilogue.  No GPU, no library call: tests/test_cpu_gemm_desc.py
checks the table and this module, tests/test_gpu_gemm_desc.py runs the table on the kernels.

Why integers.  A and B hold values of {-4..-1, 1..4}; bias, res, aux and the prior contents of C hold integers of [-8, 8].
Every product, every partial sum (in any order: K-slab, split-K workspace, column sums, gemm_tn_kernel) and every epilogue
value then is an integer below 2^24 and so exact in fp32 - reference() asserts the bound.  Integers up to 256 are exact in
bf16: the bf16x6 planes p2, p3 are zero and plain bf16 rounds nothing.  relu and relu' are exact.  So all three precisions
must give the bits of the float64 reference and the comparison is torch.equal: one dropped, duplicated, clamped-in or
mis-indexed element fails.

Sentinels.  Every float of a buffer that the descriptor does not address - the `off` leading floats of a misaligned base, the
pad columns of ld > extent, the gaps between batches - holds IN_SENTINEL in an input (read into a sum it breaks exactness)
and NaN in an output (overwritten, it is a stray write that lands INSIDE the buffer, where tests/guard.py cannot see it).

Labels.  A case's label names the cell it is there for: "f32/t64/TN/68x132x36/vec-off:A:base+1/evec-off:preact:ld%4/...".
The `vec...` token claims why the operand loader is the 16-byte or the scalar one, the `evec...` token the same for the tile
epilogue (`reduce`: split-K, the epilogue runs in splitk_reduce_kernel).  loader_reasons() / epilogue_reasons() recompute the
reasons from the case's geometry the way dpot_gemm_f32 decides; the CPU test compares the two.
"""
import dataclasses
import math
from typing import Dict, Optional, Tuple

import torch

PREC = {"f32": 0, "bf16x6": 1, "bf16": 3}          # DPOT_GEMM_*
ACT = {None: 0, "gelu": 1, "relu": 4}              # DPOT_ACT_*
MODE = {"linear": 0, "act": 1, "dact": 2}          # DPOT_EPI_*
LAYOUTS = {"NN": (False, False), "NT": (False, True), "TN": (True, False), "TT": (True, True)}
INPUTS = ("A", "B", "bias", "aux", "res")
OUTPUTS = ("C", "preact", "colsum")
IN_SENTINEL = 12345679.0                           # large, odd, exact in fp32
LIMIT = float(1 << 24)

MN_VALUES = (1, 3, 4, 33, 68, 131, 132, 200)
K_VALUES = (1, 4, 31, 32, 36, 68, 77, 100)
SPLITK_VALUES = (2, 3, 5, 7)
SPLITK_KS = (36, 68, 100)
TERM_SETS = ("plain", "bias", "bias+preact", "act", "dact", "rowres", "acc", "acc+res+bias", "bcast")
FORMS = ("vector", "scalar", "reduce")
HANDOFF_M, HANDOFF_N = (128, 256), (128, 384)


@dataclasses.dataclass(frozen=True)
class Opnd:
    """one operand of a descriptor: `rows` x `cols` valid floats per batch, row r of batch b at off + b*stride + r*ld"""
    rows: int
    cols: int
    ld: int
    stride: int
    off: int

    def size(self, batch):
        return self.off + (batch - 1) * self.stride + self.rows * self.ld

    def index(self, batch):
        """flat positions of the valid region, [batch, rows, cols]"""
        b = torch.arange(batch).view(-1, 1, 1) * self.stride
        r = torch.arange(self.rows).view(1, -1, 1) * self.ld
        return self.off + b + r + torch.arange(self.cols).view(1, 1, -1)


@dataclasses.dataclass(frozen=True)
class Case:
    label: str
    family: str
    M: int
    N: int
    K: int
    batch: int
    transA: bool
    transB: bool
    precision: str
    tile: int
    tag: int
    splitk: int
    opnd: Dict[str, Opnd]            # present operands only
    res_div: int
    res_mod: int
    accumulate: bool
    mode: str
    act: Optional[str]
    colsum_of: int
    exact: bool                      # integer data, compared with torch.equal
    claim_loader: Tuple[str, ...]    # what the label says makes the loader scalar (empty: it vectorises)
    claim_epi: Tuple[str, ...]       # the same for the tile epilogue
    eligible: Optional[bool] = None  # hand-off family: is the descriptor meant for gemm_tn_kernel
    only: bool = False               # the claimed reasons are the only ones: the case would vectorise but for them

    @property
    def layout(self):
        return ("T" if self.transA else "N") + ("T" if self.transB else "N")

    def has(self, name):
        return name in self.opnd


# ---- the host's dispatch decisions, recomputed from the geometry (csrc/gemm.hip: vecA / vecB / p.evec) ---------------------
def loader_reasons(c):
    out = []
    for name, cont in (("A", c.M if c.transA else c.K), ("B", c.K if c.transB else c.N)):
        o = c.opnd[name]
        if o.off % 4:
            out.append(f"{name}:base+{o.off % 4}")
        if o.ld % 4:
            out.append(f"{name}:ld%4")
        if cont % 4:
            out.append(f"{name}:extent%4")
        if o.stride % 4:
            out.append(f"{name}:stride%4")
    return tuple(out)


def epilogue_reasons(c):
    out = ["N%4"] if c.N % 4 else []
    for name in ("C", "bias", "aux", "preact", "res"):
        if not c.has(name):
            continue
        o = c.opnd[name]
        if o.off % 4:
            out.append(f"{name}:base+{o.off % 4}")
        if name != "bias" and o.ld % 4:          # a bias has no leading dimension
            out.append(f"{name}:ld%4")
        if o.stride % 4:
            out.append(f"{name}:stride%4")
    return tuple(out)


def loader_is_vec(c):
    return not loader_reasons(c)


def epilogue_form(c):
    return "reduce" if c.splitk > 1 else "scalar" if epilogue_reasons(c) else "vector"


def term_set(c):
    """which of TERM_SETS the case's epilogue fields spell (None: a mix that is none of the nine)"""
    t = frozenset(n for n in ("bias", "aux", "preact", "res") if c.has(n))
    rowmap = c.res_div > 1 or c.res_mod > 0
    bcast = c.has("res") and c.batch > 1 and c.opnd["res"].stride == 0
    key = (t, c.mode, c.accumulate, rowmap, bcast)
    table = {(frozenset(), "linear", False, False, False): "plain",
             (frozenset({"bias"}), "linear", False, False, False): "bias",
             (frozenset({"bias", "preact"}), "linear", False, False, False): "bias+preact",
             (frozenset({"bias", "preact", "res"}), "act", False, False, False): "act",
             (frozenset({"aux"}), "dact", False, False, False): "dact",
             (frozenset({"res"}), "linear", False, True, False): "rowres",
             (frozenset(), "linear", True, False, False): "acc",
             (frozenset({"bias", "res"}), "linear", True, False, False): "acc+res+bias",
             (frozenset({"res"}), "linear", False, False, True): "bcast"}
    name = table.get(key)
    if name == "rowres" and (c.res_div, c.res_mod) != (3, 5):
        return None
    return name


def handoff_eligible(c):
    """the eligibility rule of dpot_gemm_tn_try (csrc/gemm_tn.hip), as include/dpot_hip.h states it"""
    if c.precision != "f32" or not c.transA or c.transB or c.splitk <= 1 or c.batch != 1:
        return False
    a, b = c.opnd["A"], c.opnd["B"]
    if c.M % 128 or c.N % 128 or c.K % 32 or a.ld % 4 or b.ld % 4 or a.off % 4 or b.off % 4 or a.stride % 4 or b.stride % 4:
        return False
    nslab = c.K // 32
    return c.splitk <= nslab and -(-nslab // c.splitk) * (c.splitk - 1) < nslab


# ---- building a case -------------------------------------------------------------------------------------------------------
TERMS_OF = {"plain": (), "bias": ("bias",), "bias+preact": ("bias", "preact"), "act": ("bias", "preact", "res"),
            "dact": ("aux",), "rowres": ("res",), "acc": (), "acc+res+bias": ("bias", "res"), "bcast": ("res",)}


def mk(family, M, N, K, *, layout="NN", prec="f32", tile=64, tag=0, splitk=1, batch=1, terms="plain", act="relu",
       colsum_of=0, dev=(), pad=0, gap=0, exact=True, note="", eligible=None, only=False):
    """a Case from its cell.  terms: one of TERM_SETS.  dev: deviations "<operand>:base+k" / ":ld%4" / ":stride%4" from the
    tight, aligned layout (only: they are the ONLY reasons for the scalar path - the shape would vectorise); pad: extra
    floats on EVERY leading dimension; gap: extra floats between batches (batch > 1)"""
    transA, transB = LAYOUTS[layout]
    present = TERMS_OF[terms]
    mode = {"act": "act", "dact": "dact"}.get(terms, "linear")
    accumulate = terms.startswith("acc")
    res_div, res_mod = (3, 5) if terms == "rowres" else (0, 0)
    if terms == "bcast":
        assert batch > 1, "the broadcast residual needs a batch"
    shapes = {"A": (K, M) if transA else (M, K), "B": (N, K) if transB else (K, N), "C": (M, N)}
    for name in present:
        shapes[name] = (1, N) if name == "bias" else (res_mod, N) if name == "res" and res_mod else (M, N)
    if colsum_of:
        assert (colsum_of == 1 and transA) or (colsum_of == 2 and not transB)
        shapes["colsum"] = (1, M if colsum_of == 1 else N)
    devs = {}
    for d in dev:
        name, what = d.split(":")
        assert name in shapes, f"{d}: operand absent"
        devs.setdefault(name, []).append(what)
    opnd = {}
    for name, (rows, cols) in shapes.items():
        what = devs.get(name, [])
        one_row = name in ("bias", "colsum")
        assert not (one_row and "ld%4" in what), f"{name} has no leading dimension"
        ld = cols if one_row else cols + pad + (1 if "ld%4" in what else 0)
        off = next((int(w[-1]) for w in what if w.startswith("base+")), 0)
        stride = 0
        if batch > 1:
            stride = rows * ld + gap + (1 if "stride%4" in what else 0)
            if terms == "bcast" and name in ("A", "res"):        # the pattern of functional.py: one A, one residual for all
                stride = 0
        else:
            assert "stride%4" not in what, "a stride deviation needs a batch"
        opnd[name] = Opnd(rows, cols, ld, stride, off)
    contA, contB = (M if transA else K), (K if transB else N)
    cont_of = {"A": contA, "B": contB}
    claim_l = tuple(d for d in dev if d.split(":")[0] in ("A", "B"))
    claim_l += tuple(f"{n}:extent%4" for n, cont in (("A", contA), ("B", contB)) if cont % 4)
    claim_e = (("N%4",) if N % 4 else ()) + tuple(d for d in dev if d.split(":")[0] in ("C", "bias", "aux", "preact", "res"))
    if pad % 4:     # an odd pad is there to bring some leading dimension TO a multiple of 4; it takes others off it
        claim_l += tuple(f"{n}:ld%4" for n in "AB" if opnd[n].ld % 4 and cont_of[n] % 4 == 0)
        claim_e += tuple(f"{n}:ld%4" for n in ("C", "aux", "preact", "res") if n in opnd and opnd[n].ld % 4 and N % 4 == 0)
    parts = [prec, f"t{tile}", layout, f"{M}x{N}x{K}"]
    if batch > 1:
        parts.append(f"b{batch}")
    if tag:
        parts.append(f"tag{tag}")
    parts.append("vec" if not claim_l else "vec-off:" + ",".join(claim_l))
    parts.append("reduce" if splitk > 1 else "evec" if not claim_e else "evec-off:" + ",".join(claim_e))
    parts.append(f"{terms}({act})" if terms in ("act", "dact") else terms)
    if splitk > 1:
        parts.append(f"splitk{splitk}")
    if colsum_of:
        parts.append("cs" + "_AB"[colsum_of])
    if pad:
        parts.append(f"pad{pad}")
    if gap:
        parts.append(f"gap{gap}")
    if not exact:
        parts.append("gauss")
    if note:
        parts.append(note)
    return Case("/".join(parts), family, M, N, K, batch, transA, transB, prec, tile, tag, splitk, opnd, res_div, res_mod,
                accumulate, mode, act if mode != "linear" else None, colsum_of, exact, claim_l, claim_e, eligible, only)


def gemm_kwargs(c):
    """the scalar keyword arguments of dpot_amd.ops.gemm for this case (the tensors are the caller's)"""
    o = c.opnd

    def f(name, field, dflt=0):
        return getattr(o[name], field) if name in o else dflt
    return dict(transA=c.transA, transB=c.transB, lda=o["A"].ld, ldb=o["B"].ld, ldc=o["C"].ld, batch=c.batch,
                strideA=o["A"].stride, strideB=o["B"].stride, strideC=o["C"].stride, strideBias=f("bias", "stride"),
                act=ACT[c.act], mode=MODE[c.mode], ldaux=f("aux", "ld"), strideAux=f("aux", "stride"),
                ldpre=f("preact", "ld"), stridePre=f("preact", "stride"), ldres=f("res", "ld"), res_div=c.res_div,
                res_mod=c.res_mod, strideRes=f("res", "stride"), accumulate=c.accumulate, splitk=c.splitk, tile=c.tile,
                tag=c.tag, colsum_of=c.colsum_of, strideColsum=f("colsum", "stride"), precision=PREC[c.precision])


def build(c, seed):
    """host buffers (flat float32, `off` leading floats included) of every present operand, laid out as the descriptor
    says; whatever the descriptor does not address holds a sentinel"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for name, o in c.opnd.items():
        is_out = name in OUTPUTS
        buf = torch.full((o.size(c.batch),), float("nan") if is_out else IN_SENTINEL, dtype=torch.float32)
        idx = o.index(c.batch)
        if is_out:
            assert c.batch == 1 or o.stride >= o.rows * o.ld, f"{c.label}: batches of the output {name} overlap"
        if not is_out or (name == "C" and c.accumulate):
            nb = 1 if (c.batch > 1 and o.stride == 0) else c.batch
            shape = (nb, o.rows, o.cols)
            if not c.exact:
                vals = torch.randn(shape, generator=g) * (0.3 if name in ("A", "B") else 1.0)
            elif name in ("A", "B"):
                vals = torch.randint(1, 5, shape, generator=g) * (torch.randint(0, 2, shape, generator=g) * 2 - 1)
            else:
                vals = torch.randint(-8, 9, shape, generator=g)
            buf[idx[:nb].reshape(-1)] = vals.reshape(-1).float()
        out[name] = buf
    return out


def _gelu(x):
    return 0.5 * x * (1.0 + torch.erf(x / math.sqrt(2.0)))


def _dgelu(x):
    return 0.5 * (1.0 + torch.erf(x / math.sqrt(2.0))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2.0 * math.pi)


def reference(c, t):
    """the header's epilogue order (include/dpot_hip.h, dpot_gemm_desc) in float64 on the buffers of build(): C, preact and
    colsum as [batch, rows, cols].  Integer cases: asserts that no intermediate reaches 2^24 in magnitude (a condition on
    the case table: below it fp32 sums are exact in any order)"""
    def get(name):
        return t[name][c.opnd[name].index(c.batch)].double()
    A, B = get("A"), get("B")
    opA = A.transpose(1, 2) if c.transA else A                  # [batch, M, K]
    opB = B.transpose(1, 2) if c.transB else B                  # [batch, K, N]
    v = torch.matmul(opA, opB)                                  # float64: exact on the integer data
    bound = torch.matmul(opA.abs(), opB.abs())                  # no partial sum, in any order, exceeds this
    ref = {}
    if c.has("bias"):
        bias = get("bias")                                      # [batch, 1, N]
        v = v + bias
        bound = bound + bias.abs()
    if c.has("preact"):
        ref["preact"] = v.clone()
    if c.mode == "act":
        v = torch.clamp(v, min=0.0) if c.act == "relu" else _gelu(v)
    elif c.mode == "dact":
        aux = get("aux")
        v = v * ((aux > 0).double() if c.act == "relu" else _dgelu(aux))
    if c.has("res"):
        rows = torch.arange(c.M)
        if c.res_div > 1:
            rows = rows // c.res_div
        if c.res_mod > 0:
            rows = rows % c.res_mod
        res = get("res")[:, rows, :]
        v = v + res
        bound = bound + res.abs()
    if c.accumulate:
        c0 = get("C")
        v = v + c0
        bound = bound + c0.abs()
    ref["C"] = v
    if c.colsum_of:
        src = A if c.colsum_of == 1 else B                      # stored [K, M] / [K, N]: sum over the K rows
        ref["colsum"] = src.sum(1, keepdim=True)
        bound = torch.maximum(bound.max(), src.abs().sum(1).max())
    if c.exact:
        assert float(bound.max()) < LIMIT, f"{c.label}: an intermediate may reach {float(bound.max()):.0f} >= 2^24"
    return ref


def check(c, before, after, ref):
    """after: the buffers of build() after the kernels ran.  Valid regions of C / preact / colsum equal the reference (bit
    for bit on integer data, helpers.assert_close at its defaults on Gaussian data) and hold no NaN; every sentinel of every
    output is still there; no input changed.  Raises AssertionError naming everything that is wrong."""
    bad = []
    for name in c.opnd:
        o = c.opnd[name]
        idx = o.index(c.batch)
        if name in OUTPUTS:
            got = after[name][idx].double()
            n_nan = int(got.isnan().sum())
            if n_nan:
                bad.append(f"{name}: {n_nan} of {got.numel()} valid elements are NaN (never written, or a NaN was read)")
            elif c.exact:
                if not torch.equal(got, ref[name]):
                    ne = got != ref[name]
                    pos = tuple(int(i) for i in torch.nonzero(ne)[0])
                    bad.append(f"{name}: {int(ne.sum())} of {got.numel()} elements differ from the float64 reference, first "
                               f"at [batch, row, col] = {pos}: got {float(got[pos])}, reference {float(ref[name][pos])}")
            else:
                from helpers import assert_close
                try:
                    assert_close(got, ref[name], name)
                except AssertionError as e:
                    bad.append(str(e))
            pad = torch.ones(after[name].numel(), dtype=torch.bool)
            pad[idx.reshape(-1)] = False
            hit = pad & ~after[name].isnan()
            if hit.any():
                bad.append(f"{name}: {int(hit.sum())} sentinel(s) overwritten (pad column, batch gap or base offset), first at "
                           f"flat position {int(torch.nonzero(hit)[0])} of {after[name].numel()}")
        if name in INPUTS:
            if not torch.equal(before[name], after[name]):
                ne = before[name] != after[name]
                bad.append(f"{name}: input changed at {int(ne.sum())} position(s), first at flat position "
                           f"{int(torch.nonzero(ne)[0])}")
    assert not bad, f"{c.label}:\n  " + "\n  ".join(bad)


# ---- the table ---------------------------------------------------------------------------------------------------------------
PRECS = ("f32", "bf16x6", "bf16")
LAY = ("NN", "NT", "TN", "TT")
ALIGNED = [(68, 132, 36), (132, 200, 68), (200, 68, 100), (4, 4, 4), (132, 68, 32), (68, 4, 68)]   # M, N, K all % 4 == 0


def _loader_cases():
    out = []
    sweep = [(1, 200, 1), (3, 132, 4), (4, 131, 31), (33, 68, 32), (68, 33, 36), (131, 4, 68), (132, 3, 77), (200, 1, 100)]
    for pi, p in enumerate(PRECS):
        for i, (M, N, K) in enumerate(sweep):                       # every M, N, K value; whatever loader the shape gives
            out.append(mk("loader", M, N, K, layout=LAY[(i + pi) % 4], prec=p, tile=(64, 128)[(i + pi) % 2], note="sweep"))
        for i, (K, lay) in enumerate([(31, "NT"), (31, "TN"), (77, "NT"), (77, "TN"), (1, "NT"), (1, "TN")]):
            M, N, _ = ALIGNED[i % 3]                                # odd K against K-contiguous and row-contiguous operands
            out.append(mk("loader", M, N, K, layout=lay, prec=p, tile=(128, 64)[(i + pi) % 2], note="oddK"))
        for i, lay in enumerate(LAY):                               # vectorising, tight and padded, single and batched
            M, N, K = ALIGNED[(i + pi) % len(ALIGNED)]
            out.append(mk("loader", M, N, K, layout=lay, prec=p, tile=(64, 128)[(i + pi) % 2], pad=4 * (i % 2),
                          batch=1 + (i // 2), gap=8 * (i // 2)))
            out.append(mk("loader", M, N, K, layout=lay, prec=p, tile=(128, 64)[(i + pi) % 2], pad=4 * ((i + 1) % 2)))
        # K = 4: the 16-byte loader of a K-contiguous operand clamps every k to min(k, kmax - 4) = 0
        out.append(mk("loader", 4, 4, 4, layout="NT", prec=p, tile=(64, 128)[pi % 2], note="K4"))
        out.append(mk("loader", 68, 132, 4, layout="NN", prec=p, tile=(128, 64)[pi % 2], note="K4"))
        i = 0
        for name in "AB":                                           # each reason for the scalar loader, on its own
            for what in ("base+1", "base+2", "base+3", "ld%4", "stride%4"):
                M, N, K = ALIGNED[(i + pi) % len(ALIGNED)]
                out.append(mk("loader", M, N, K, layout=LAY[(i + pi) % 4], prec=p, tile=(64, 128)[i % 2],
                              dev=(f"{name}:{what}",), batch=2 if what == "stride%4" else 1, only=True))
                i += 1
        for t, dev in ((64, ()), (128, ("A:base+1",))):             # the tag == 1 instantiation (layout NN only)
            out.append(mk("loader", 68, 132, 36, layout="NN", prec=p, tile=t if pi % 2 == 0 else 192 - t, tag=1, dev=dev))
    return out


def _epilogue_cases():
    out = []
    vec_shapes = [(33, 132, 36), (131, 68, 32), (200, 4, 68), (68, 200, 100)]
    sca_shapes = [(68, 33, 36), (132, 131, 32), (4, 3, 4), (200, 1, 77)]
    n = 0
    for pi, p in enumerate(PRECS):
        for ti, terms in enumerate(TERM_SETS):
            b = 3 if terms == "bcast" else (2 if (ti + pi) % 3 == 0 else 1)
            lay = LAY[(ti + pi) % 4]
            M, N, K = vec_shapes[(ti + pi) % 4]
            out.append(mk("epilogue", M, N, K, layout=lay, prec=p, tile=(64, 128)[n % 2], terms=terms, batch=b,
                          pad=4 * (n % 2), gap=8 * (n % 2) if b > 1 else 0))
            # the scalar tile epilogue: by N % 4, or by ldc % 4 at a shape that would vectorise
            if (ti + pi) % 2 == 0:
                M, N, K = sca_shapes[(ti + pi) % 4]
                out.append(mk("epilogue", M, N, K, layout=lay, prec=p, tile=(128, 64)[n % 2], terms=terms, batch=b))
            else:
                M, N, K = vec_shapes[(ti + pi + 1) % 4]
                out.append(mk("epilogue", M, N, K, layout=lay, prec=p, tile=(128, 64)[n % 2], terms=terms, batch=b,
                              dev=("C:ld%4",), pad=4 * ((n + 1) % 2)))
            M, N, K = [(33, 132, 68), (131, 68, 100), (200, 3, 68), (68, 131, 100)][(ti + pi) % 4]
            out.append(mk("epilogue", M, N, K, layout=lay, prec=p, tile=(64, 128)[n % 2], terms=terms, batch=b,
                          splitk=(2, 3)[n % 2], pad=4 * (n % 2)))
            n += 1
    for pi, p in enumerate(PRECS):      # N % 4 on its own: N = 33 in rows of 36 floats, every leading dimension a multiple of 4
        out.append(mk("epilogue", 68, 33, 36, layout=LAY[pi], prec=p, tile=(64, 128)[pi % 2], terms="act", pad=3, only=True))
    # each other reason for the scalar tile epilogue on its own, at shapes that would vectorise
    reasons = [("C", w) for w in ("base+1", "base+2", "base+3", "ld%4", "stride%4")]
    reasons += [("bias", w) for w in ("base+1", "base+2", "base+3", "stride%4")]
    for name in ("aux", "preact", "res"):
        reasons += [(name, w) for w in ("base+1", "base+2", "base+3", "ld%4", "stride%4")]
    for i, (name, what) in enumerate(reasons):
        M, N, K = ALIGNED[i % len(ALIGNED)]
        out.append(mk("epilogue", M, N, K, layout=LAY[i % 4], prec=PRECS[i % 3], tile=(64, 128)[(i // 3) % 2],
                      terms="dact" if name == "aux" else "act", dev=(f"{name}:{what}",),
                      batch=2 if what == "stride%4" else 1, only=True))
    return out


def _splitk_cases():
    out = []
    shapes = [(33, 68), (131, 4), (200, 132), (68, 131), (4, 200), (132, 33)]
    for pi, p in enumerate(PRECS):
        n = 0
        for s in SPLITK_VALUES:
            for K in SPLITK_KS:
                cs = (n + pi) % 3
                lay = LAY[(n + pi) % 4] if cs == 0 else ("TN", "TT")[n % 2] if cs == 1 else ("NN", "TN")[n % 2]
                M, N = shapes[(n + pi) % len(shapes)]
                out.append(mk("splitk", M, N, K, layout=lay, prec=p, tile=(64, 128)[n % 2], splitk=s, colsum_of=cs,
                              batch=(1, 3)[(n // 2) % 2], gap=4 * (n % 2) if (n // 2) % 2 else 0))
                n += 1
    return out


def _colsum_cases():
    out = []
    shapes = [(131, 68, 77), (200, 132, 100), (68, 200, 36), (132, 131, 68)]
    for pi, p in enumerate(PRECS):
        n = 0
        for of in (1, 2):
            for s in (1, 3):
                for t in (64, 128):
                    M, N, K = shapes[(n + pi) % 4]
                    lay = (("TN", "TT") if of == 1 else ("NN", "TN"))[n % 2]
                    b = (1, 3)[(n + pi) % 2]
                    out.append(mk("colsum", M, N, K, layout=lay, prec=p, tile=t, splitk=s, colsum_of=of, batch=b,
                                  dev=("colsum:base+1",) if n % 4 == 1 else (), gap=4 if b > 1 and n % 3 == 0 else 0,
                                  terms=("plain", "bias", "acc")[n % 3]))
                    n += 1
    return out


# (K, splitk) -> slabs per split: 1,1 | 1,1,1 | 2,1 | 2,2 | 3,3 | 3,3,1 | 4,4 | 5,4
HANDOFF_SPLITS = [(64, 2), (96, 3), (96, 2), (128, 2), (192, 2), (224, 3), (256, 2), (288, 2)]


def _handoff_cases():
    out = []
    mn = [(M, N) for M in HANDOFF_M for N in HANDOFF_N]
    for i, (K, s) in enumerate(HANDOFF_SPLITS):
        for cs in (0, 1, 2):
            M, N = mn[(i + cs) % 4]
            for pad in (0, 8):                                      # pad: the operands are column windows of wider matrices
                out.append(mk("handoff", M, N, K, layout="TN", splitk=s, colsum_of=cs, pad=pad, eligible=True,
                              note=f"tn:{'+'.join(map(str, _slabs(K, s)))}slabs"))
        # ineligible neighbours: the generic kernel must give the same bits
        cs = i % 3
        M, N = mn[i % 4]
        pad = 8 * (i % 2)
        kw = dict(layout="TN", colsum_of=cs, pad=pad, eligible=False)
        nslab = K // 32
        out.append(mk("handoff", M, N, K + 4, splitk=s, note="near:K+4", **kw))
        out.append(mk("handoff", M + 4, N, K, splitk=s, note="near:M+4", **kw))
        out.append(mk("handoff", M, N, K, splitk=s, dev=("A:base+1",), note="near:A+1float", **kw))
        out.append(mk("handoff", M, N, K, splitk=s, dev=("A:ld%4",), note="near:lda%4", **kw))
        out.append(mk("handoff", M, N, K, splitk=nslab + 1, note="near:splitk>slabs", **kw))
        empty = next((q for q in range(2, nslab + 1) if -(-nslab // q) * (q - 1) >= nslab), None)
        if empty:                                                   # no such split count exists for 2 or 3 slabs
            out.append(mk("handoff", M, N, K, splitk=empty, note="near:empty-split", **kw))
    return out


def _slabs(K, s):
    nslab = K // 32
    sps = -(-nslab // s)
    return [min(sps, nslab - i * sps) for i in range(s)]


def _gauss_cases():
    # gelu and gelu' in both epilogue forms and the split-K reduce; f32 and bf16x6 (plain bf16 rounds its operands to 8 bits:
    # ~4e-3 relative, it is not meant to meet the 1e-4 of helpers.assert_close on real-valued data)
    out = []
    for pi, p in enumerate(("f32", "bf16x6")):
        for ti, terms in enumerate(("act", "dact")):
            lay = LAY[(2 * pi + ti) % 4]
            out.append(mk("gauss", 131, 68, 100, layout=lay, prec=p, tile=(64, 128)[ti], terms=terms, act="gelu", exact=False))
            out.append(mk("gauss", 68, 131, 77, layout=lay, prec=p, tile=(128, 64)[ti], terms=terms, act="gelu", exact=False))
            out.append(mk("gauss", 200, 33, 100, layout=lay, prec=p, tile=(64, 128)[pi], terms=terms, act="gelu", exact=False,
                          splitk=3))
    return out


CASES = _loader_cases() + _epilogue_cases() + _splitk_cases() + _colsum_cases() + _handoff_cases() + _gauss_cases()
FAMILIES = ("loader", "epilogue", "splitk", "colsum", "handoff", "gauss")


def items():
    """the table cut into the items of tests/test_gpu_gemm_desc.py: families split by precision (the hand-off family, native
    fp32 only, by its column sums) - id -> cases; every case is in exactly one item"""
    out = {}
    for c in CASES:
        key = f"{c.family}-cs{c.colsum_of}" if c.family == "handoff" else f"{c.family}-{c.precision}"
        out.setdefault(key, []).append(c)
    return out


_SEEDS = {c.label: 7000 + i for i, c in enumerate(CASES)}


def seed_of(c):
    """a fixed seed per case (its position in the table)"""
    return _SEEDS[c.label]
