"""Integer operands, float64 reference and pack helpers for the launch-plan sweep of the bf16 panel GEMM
(csrc/gemm_bf16p.hip: dpot_gemm_bf16p, dpot_gemm_bf16p_pair; planes == 1 only).  No GPU, no library call:
tests/test_cpu_bf16p.py checks this module, tests/test_gpu_bf16p.py runs the table of bf16p_cases.py with it.

Why integers.  A and W hold integers of {-vmax..-1, 1..vmax} (vmax <= 4: exact in bf16, and never zero, so every product
counts); bias, residual and aux hold integers of [-8, 8].  Every product, every k-slab partial, every split-K partial in the
workspace, every reduce and every epilogue value then is an integer, and reference() asserts that the sum of the ABSOLUTE
terms of every accumulation it relies on - each output element over k, each column sum over the rows - stays below 2^24:
below that fp32 sums are exact in any order.  relu and relu' are exact.  So the kernels must give the bits of the float64
reference and every comparison is torch.equal: one dropped k-slab of a ragged split, one row clamped onto its neighbour,
one tile written for another fails.  The bf16 packs of an output are its round-to-nearest-even bf16 rounding, which
torch's .bfloat16() is as well.
"""
from typing import Dict, Optional

import torch

LIMIT = float(1 << 24)
ACT_RELU = 4                     # DPOT_ACT_RELU
EPI_LINEAR, EPI_ACT, EPI_DACT = 0, 1, 2


# ---- operands ----------------------------------------------------------------------------------------------------------
def operand(rows, cols, vmax, seed):
    """[rows, cols] float32 integers of {-vmax..-1, 1..vmax}"""
    g = torch.Generator().manual_seed(seed)
    mag = torch.randint(1, vmax + 1, (rows, cols), generator=g, dtype=torch.int8)
    sign = torch.randint(0, 2, (rows, cols), generator=g, dtype=torch.int8) * 2 - 1
    return (mag * sign).float()


def term(rows, cols, seed):
    """[rows, cols] float32 integers of [-8, 8] (bias: rows = 1; residual, aux)"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-8, 9, (rows, cols), generator=g, dtype=torch.int8).float()


def build(M, N, K, vmax, seed, want=("bias", "res", "aux")):
    """the operands of one problem: A [M, K], W [N, K] (nn.Linear layout: C = A W^T) and the epilogue terms in `want`"""
    t = {"A": operand(M, K, vmax, seed), "W": operand(N, K, vmax, seed + 1)}
    if "bias" in want:
        t["bias"] = term(1, N, seed + 2).view(N)
    if "res" in want:
        t["res"] = term(M, N, seed + 3)
    if "aux" in want:
        t["aux"] = term(M, N, seed + 4)
    return t


# ---- the reference -----------------------------------------------------------------------------------------------------
def reference(t: Dict[str, torch.Tensor], mode: int = EPI_LINEAR, bias: bool = False, res: bool = False,
              dact: Optional[torch.Tensor] = None, colsum: bool = False, what: str = "") -> Dict[str, torch.Tensor]:
    """float64 restatement of the epilogue (include/dpot_hip.h: bias, pre-activation save, relu / relu'(aux), residual):
    {"pre", "C"} and, with colsum, {"colsum"} (the column sums of C over its M rows).  dact: a {0, 1} matrix that stands
    for the saved act' pack of an EPI_DACT launch (instead of aux).  Asserts the exactness bound."""
    A, W = t["A"].double(), t["W"].double()
    M, K = A.shape
    v = A @ W.t()
    # sum over k of |a| |w| <= K max|a| max|w| for every element: no partial sum, in any order or split, exceeds this
    top = K * float(A.abs().max()) * float(W.abs().max())
    if bias:
        v = v + t["bias"].double()
        top += float(t["bias"].abs().max())
    out = {"pre": v.clone()}
    if mode == EPI_ACT:
        v = torch.clamp(v, min=0.0)
    elif mode == EPI_DACT:
        v = v * (dact.double() if dact is not None else (t["aux"] > 0).double())
    if res:
        v = v + t["res"].double()
        top += float(t["res"].abs().max())
    out["C"] = v
    if colsum:
        out["colsum"] = v.sum(0)
        top *= M                                     # |C| <= top element-wise: the absolute terms of a column sum
    assert top < LIMIT, f"{what}: the absolute terms of an accumulation may reach {top:.0f} >= 2^24"
    out["bound"] = top
    return out


def dact_of(pre64):
    """relu'(pre) as the EPI_ACT launch saves it: {0, 1}"""
    return (pre64 > 0).float()


# ---- packs (include/dpot_hip.h: [ceil(rows/32)][K/16][64 chunks][8 bf16], chunk l = (row l & 31, k 8 (l >> 5) .. + 7)) -----
def pack_rows(x):
    """[R, K] (R % 32 == 0, K % 16 == 0) -> the flat row-form pack, bf16"""
    R, K = x.shape
    assert R % 32 == 0 and K % 16 == 0
    t = x.bfloat16().view(R // 32, 32, K // 16, 2, 8)                     # [rt, row, kb, half, 8]
    return t.permute(0, 2, 3, 1, 4).reshape(-1)


def unpack_rows(pk, R, K):
    """the inverse of pack_rows: flat pack -> [R, K] float32"""
    t = pk.view(R // 32, K // 16, 2, 32, 8).float()                        # [rt, kb, half, row, 8]
    return t.permute(0, 3, 1, 2, 4).reshape(R, K)


def pack_frag(x):
    """[M, N] (both % 32 == 0) -> the act' pack in FRAGMENT order [M/32][N/32][2 halves][64 lanes][8 bf16]
    (csrc/gemm_bf16p_common.h epi_fragment_direct): lane l = (column l & 31, kh = l >> 5), element j of half s is row
    (j & 3) + 4 kh + 8 (j >> 2) + 16 s of the 32 x 32 fragment"""
    M, N = x.shape
    assert M % 32 == 0 and N % 32 == 0
    t = x.bfloat16().view(M // 32, 2, 2, 2, 4, N // 32, 32)                # [mt, s, j >> 2, kh, j & 3, nt, col]
    return t.permute(0, 5, 1, 3, 6, 2, 4).reshape(-1)                      # [mt, nt, s, kh, col, j >> 2, j & 3]


def unpack_frag(pk, M, N):
    """the inverse of pack_frag: flat pack -> [M, N] float32"""
    t = pk.view(M // 32, N // 32, 2, 2, 32, 2, 4).float()                  # [mt, nt, s, kh, col, j >> 2, j & 3]
    return t.permute(0, 2, 5, 3, 6, 1, 4).reshape(M, N)                    # row bits [s][j >> 2][kh][j & 3]


# ---- comparison ---------------------------------------------------------------------------------------------------------
def first_difference(got, ref, tile_rows=128, tile_cols=256):
    """None if got == ref bit for bit (and holds no NaN), else a sentence naming the first differing (row, col), the values
    and the workgroup tile it lies in.  got / ref: [M, N] tensors of one dtype on one device"""
    if got.shape != ref.shape:
        return f"shape {tuple(got.shape)} instead of {tuple(ref.shape)}"
    if torch.equal(got, ref):
        return None
    ne = (got != ref) | got.isnan()
    flat = int(torch.nonzero(ne.reshape(-1))[0])
    ncol = ref.shape[-1] if ref.dim() > 1 else ref.numel()
    r, c = divmod(flat, ncol)
    g = got.reshape(-1)[flat].item()
    w = ref.reshape(-1)[flat].item()
    return (f"{int(ne.sum())} of {ref.numel()} elements differ, first at (row, col) = ({r}, {c}): got {g}, reference {w}; "
            f"tile (tm, tn) = ({r // tile_rows}, {c // tile_cols}) of {tile_rows} x {tile_cols}")
