"""Case table of the GroupNorm kernel tests (csrc/norm.hip).

One module, two readers: tests/test_cpu_groupnorm.py asserts with the library's own selection (dpot_groupnorm_kernel_kind)
that every case still reaches the route it is here for and that the table reaches every route that exists
(dpot_groupnorm_kernel_kinds); tests/test_gpu_groupnorm.py runs the kernels on the very same tuples, inputs and float64
references.

A case is (B, T, E, G, form, off, kind_fwd, kind_bwd, note):
    form   "fb"       groupnorm_fwd + groupnorm_bwd with the workspace (chunked=True)
           "fb_noc"   the same without (chunked=False): the one-workgroup-per-slab kernels on a slab that would be chunked
           "stats"    groupnorm_stats (forward with y == NULL); kind_fwd is its kind, kind_bwd unused (-1)
           "packs"    groupnorm_bwd_packs; kind_bwd is its kind, kind_fwd that of the forward that feeds it
    off    misalignment: ((operand, floats), ...) - the operand is a view that many floats into a 16-byte aligned buffer;
           operands x, dy, add, gamma, beta and "out" (y in the forward, dx in the backward)
    kinds  SCALAR / VEC4 (generic kernels), CACHED4 / CACHED8 (register-cached), CHUNKED, REFUSED

The kinds are written down per section by hand; gn_select below restates the selection rules of csrc/norm.hip in plain
Python and the CPU test holds table, restatement and library to one another:
    cached     E/G = 4 * 2^k <= 256 (one channel quad per lane, TJ = E/G/4 lanes, TT = 1024 / TJ token lanes) and
               T <= 4 TT (4 items) or T <= 8 TT (8 items)
    chunked    a workspace, E/G % 4 == 0, E/G <= 1024, not cached, B*G < 192, T >= 64; chunks = min(ceil(512 / (B*G)), T // 16,
               64) >= 2, TC = ceil(T / chunks), chunks = ceil(T / TC)
    float4     E/G % 4 == 0 and every pointer 16-byte aligned; else scalar
    packs      T % 32 == 0, E % 32 == 0 and either E/G == 128 in a cached slab (rows 1) or a chunked slab with E/G % 32 == 0,
               E/G <= 256, TC % 32 == 0 (rows = chunks); every pointer aligned
"""
import functools
from collections import namedtuple

import torch

SCALAR, VEC4, CACHED4, CACHED8, CHUNKED, REFUSED = 0, 1, 4, 8, 16, -1
THREADS = 1024
EPS = 1e-5

Case = namedtuple("Case", "B T E G form off kind_fwd kind_bwd note")


def case_id(c):
    off = "".join(f"-{k}+{v}" for k, v in c.off)
    return f"{c.form}-B{c.B}-T{c.T}-E{c.E}-G{c.G}{off}"


# ---- the selection, restated ------------------------------------------------------------------------------------------
def gn_cached_items(T, E, G):
    cg = E // G
    if cg % 4:
        return 0
    tj = cg // 4
    if tj < 1 or tj > 64 or tj & (tj - 1):
        return 0
    tt = THREADS // tj
    return 4 if T <= 4 * tt else 8 if T <= 8 * tt else 0


def gn_chunking(B, T, E, G):
    """(TC, chunks), (0, 0) when the shape is never chunked"""
    cg = E // G
    if cg % 4 or cg > THREADS or gn_cached_items(T, E, G):
        return 0, 0
    slabs = B * G
    if slabs >= 192 or T < 64:
        return 0, 0
    chunks = min((512 + slabs - 1) // slabs, T // 16, 64)
    if chunks < 2:
        return 0, 0
    tc = (T + chunks - 1) // chunks
    return tc, (T + tc - 1) // tc


def gn_packs_rows(B, T, E, G):
    if min(B, T, E, G) <= 0 or E % G or T % 32 or E % 32:
        return 0
    cg = E // G
    if cg == 128 and gn_cached_items(T, E, G):
        return 1
    tc, chunks = gn_chunking(B, T, E, G)
    return chunks if chunks and cg % 32 == 0 and cg <= 256 and tc % 32 == 0 else 0


def gn_select(B, T, E, G, direction, has_workspace=True, aligned=True):
    if min(B, T, E, G) <= 0 or E % G or B > 65535:
        return REFUSED
    if direction == "bwd_packs":
        if not aligned or gn_packs_rows(B, T, E, G) == 0:
            return REFUSED
        if E // G == 128 and gn_cached_items(T, E, G):
            return gn_cached_items(T, E, G)
        return CHUNKED if has_workspace else REFUSED
    if direction not in ("fwd", "bwd", "stats"):
        return REFUSED
    vec = (E // G) % 4 == 0 and aligned
    if vec and has_workspace and gn_chunking(B, T, E, G)[1]:
        return CHUNKED
    if direction == "stats":
        return REFUSED
    items = gn_cached_items(T, E, G) if vec else 0
    return items if items else VEC4 if vec else SCALAR


FWD_OPERANDS = ("x", "gamma", "beta", "out")           # the pointers whose alignment the forward looks at
BWD_OPERANDS = ("x", "dy", "add", "gamma", "out")      # ... the backward


def aligned_for(c, direction):
    names = FWD_OPERANDS if direction in ("fwd", "stats") else BWD_OPERANDS
    return not any(k in names and v % 4 for k, v in c.off)


def expected_kinds(c):
    """(kind of the forward, kind of the backward) from the restated selection"""
    ws = c.form != "fb_noc"
    if c.form == "stats":
        return gn_select(c.B, c.T, c.E, c.G, "stats", True, aligned_for(c, "stats")), REFUSED
    kf = gn_select(c.B, c.T, c.E, c.G, "fwd", ws, aligned_for(c, "fwd"))
    kb = gn_select(c.B, c.T, c.E, c.G, "bwd_packs" if c.form == "packs" else "bwd", ws, aligned_for(c, "bwd"))
    return kf, kb


# ---- the table --------------------------------------------------------------------------------------------------------
def _fb(kind, B, T, E, G, note, form="fb"):
    return Case(B, T, E, G, form, (), kind, kind, note)


CASES = []
# ---- register-cached, 4 items --------------------------------------------------------------------------------------------
CASES += [_fb(CACHED4, 2, 40, 64, 8, "T below the 512 token lanes: every item but the first is a clamped load"),
          _fb(CACHED4, 2, 600, 64, 8, "the second item partly filled (88 of 512 lanes), items 3 and 4 empty"),
          _fb(CACHED4, 2, 96, 1024, 8, "128 channels per group, 3 of 4 items"),
          _fb(CACHED4, 3, 256, 512, 8, "exactly full: 4 items x 64 token lanes"),
          _fb(CACHED4, 1, 2048, 64, 8, "exactly full at 2 channel lanes: the last shape of 4 items")]
# ---- register-cached, 8 items --------------------------------------------------------------------------------------------
CASES += [_fb(CACHED8, 1, 2049, 64, 8, "one token past 4 items: item 5 holds a single token"),
          _fb(CACHED8, 1, 2100, 32, 4, "G = 4"),
          _fb(CACHED8, 1, 4200, 32, 8, "E/G = 4: one channel lane, 1024 token lanes"),
          _fb(CACHED8, 1, 256, 1024, 8, "exactly full: 8 items x 32 token lanes")]
# ---- generic float4 ------------------------------------------------------------------------------------------------------
CASES += [_fb(VEC4, 24, 40, 1536, 8, "192 slabs (DPOT-L from batch 24 on): T above the 32 token lanes, channel loop of two trips"),
          _fb(VEC4, 24, 520, 96, 8, "three channel quads on two lanes, T above the 512 token lanes"),
          _fb(VEC4, 1, 100, 4128, 4, "E/G = 1032 > 1024: never chunked; five ragged trips of the channel loop"),
          _fb(VEC4, 24, 64, 96, 8, "B*G = 192: the slabs fill the chip as they are"),
          _fb(VEC4, 1, 63, 96, 8, "T = 63: one token short of the chunked kernels"),
          _fb(VEC4, 1, 4097, 64, 8, "one token past the 8-item cached kernels, without a workspace", form="fb_noc"),
          _fb(VEC4, 1, 8200, 32, 8, "E/G = 4 past the cached kernels: one channel lane, nine token trips", form="fb_noc")]
# ---- generic scalar ------------------------------------------------------------------------------------------------------
CASES += [_fb(SCALAR, 3, 9, 8, 8, "E/G = 1, T below the lanes"),
          _fb(SCALAR, 1, 1030, 8, 8, "E/G = 1, T above the 1024 token lanes"),
          _fb(SCALAR, 2, 70, 48, 8, "E/G = 6: four channel lanes for six channels"),
          _fb(SCALAR, 2, 33, 1048, 8, "E/G = 131: three ragged trips of the channel loop over 64 lanes")]
# ---- chunked, and the same slabs on the one-workgroup kernels (chunked=False) ----------------------------------------------
_CHUNKED = [(1, 64, 96, 8, "four chunks of 16 tokens: the smallest chunked shape"),
            (2, 65, 96, 8, "chunks of 17, 17, 17 and 14 tokens"),
            (23, 64, 96, 8, "B*G = 184: three chunks of 22, 22 and 20"),
            (3, 130, 12, 1, "G = 1, three channel quads"),
            (2, 300, 48, 4, "G = 4"),
            (2, 200, 96, 8, "twelve chunks of 17, the last of 13"),
            (1, 64, 2048, 2, "E/G = 1024, the bound: 4 token lanes, every thread a column of the apply prologue"),
            (1, 1000, 1536, 8, "59 chunks of 17, the last of 14"),
            (1, 2048, 512, 4, "64 chunks, the cap"),
            (1, 6400, 256, 1, "chunks of 6400 float4: past what the statistics kernel prefetches (6 x 1024)"),
            (4, 1024, 1536, 8, "DPOT-L at 256^2, batch 4")]
for _B, _T, _E, _G, _note in _CHUNKED:
    _items = gn_cached_items(_T, _E, _G)
    assert _items == 0
    CASES += [_fb(CHUNKED, _B, _T, _E, _G, _note),
              _fb(VEC4, _B, _T, _E, _G, "the one-workgroup kernel on: " + _note, form="fb_noc"),
              Case(_B, _T, _E, _G, "stats", (), CHUNKED, REFUSED, "statistics only: " + _note)]
# ---- misaligned bases: the generic scalar kernels on float4 shapes -----------------------------------------------------
#   x, gamma, out are read by both directions, beta by the forward alone, dy and add by the backward alone
for _B, _T, _E, _G, _aligned in [(2, 200, 96, 8, CHUNKED), (2, 96, 1024, 8, CACHED4)]:
    for _name in ("x", "dy", "add", "gamma", "beta", "out"):
        _kf = SCALAR if _name in FWD_OPERANDS else _aligned
        _kb = SCALAR if _name in BWD_OPERANDS else _aligned
        CASES += [Case(_B, _T, _E, _G, "fb", ((_name, 1),), _kf, _kb, f"the base of {_name} one float off a 16-byte boundary")]
CASES += [Case(2, 96, 1024, 8, "fb", (("x", 3), ("out", 2)), SCALAR, SCALAR, "x three floats and the output two floats off"),
          Case(2, 200, 96, 8, "fb", (("x", 4), ("dy", 8), ("out", 4)), CHUNKED, CHUNKED, "offsets of whole float4s stay aligned")]
# ---- pack-writing backward ---------------------------------------------------------------------------------------------
CASES += [Case(2, 96, 1024, 8, "packs", (), CACHED4, CACHED4, "three row tiles of four items"),
          Case(1, 256, 1024, 8, "packs", (), CACHED8, CACHED8, "eight row tiles: every item"),
          Case(1, 32, 1024, 8, "packs", (), CACHED4, CACHED4, "one row tile"),
          Case(1, 2016, 256, 8, "packs", (), CHUNKED, CHUNKED, "E/G = 32, the lower channel bound: 63 chunks of one sub-tile"),
          Case(3, 1344, 128, 4, "packs", (), CHUNKED, CHUNKED, "G = 4, 42 chunks"),
          Case(1, 2016, 768, 8, "packs", (), CHUNKED, CHUNKED, "E/G = 96"),
          Case(1, 2016, 1024, 8, "packs", (), CHUNKED, CHUNKED, "E/G = 128 on a slab too long for the cached kernels"),
          Case(1, 2016, 1024, 4, "packs", (), CHUNKED, CHUNKED, "E/G = 256, the upper channel bound: the whole staging tile"),
          Case(4, 1024, 1536, 8, "packs", (), CHUNKED, CHUNKED, "DPOT-L: 16 chunks of two sub-tiles, E/G = 192")]

FB = [c for c in CASES if c.form in ("fb", "fb_noc")]
STATS = [c for c in CASES if c.form == "stats"]
PACKS = [c for c in CASES if c.form == "packs"]

# boundary pairs: neighbouring shapes on different routes (each side is a case above)
PAIRS = [((1, 2049, 64, 8), (1, 2048, 64, 8)),      # 8 | 4 items
         ((23, 64, 96, 8), (24, 64, 96, 8)),        # chunked | generic: 184 | 192 slabs
         ((1, 64, 96, 8), (1, 63, 96, 8))]          # chunked | generic: T = 64 | 63

# refusals: (B, T, E, G)
STATS_REFUSED = [(2, 96, 1024, 8),                  # a cached slab
                 (24, 64, 96, 8),                   # 192 slabs
                 (1, 63, 96, 8),                    # T < 64
                 (2, 70, 48, 8)]                    # E/G % 4 != 0
PACKS_REFUSED = [(1, 256, 2048, 8),                 # chunks of 16 tokens: no whole row tile
                 (2, 512, 768, 8),
                 (2, 600, 64, 8),                   # cached, but not 128 channels per group (and T % 32 != 0)
                 (24, 64, 1536, 8)]                 # 192 slabs: neither cached nor chunked

# the hard statistics inputs on one case of every forward route: (B, T, E, G, chunked, kind of the forward)
HARD_RECIPES = ("large_mean", "outlier_first", "tiny_variance", "offset_border")
HARD_SHAPES = [(2, 2048, 768, 8, True, CHUNKED),
               (2, 2048, 768, 8, False, VEC4),
               (3, 256, 512, 8, True, CACHED4),
               (1, 4200, 32, 8, True, CACHED8),
               (2, 256, 48, 8, True, SCALAR)]

# groupnorm_param_grads: B x E, each with one to four jobs
PARAM_GRAD_B = (1, 4, 5, 8, 9, 13)
PARAM_GRAD_E = (8, 96, 512)


# ---- inputs and float64 references --------------------------------------------------------------------------------------
def _gen(B, T, E, G, salt=0):
    return torch.Generator().manual_seed(((B * 131 + T) * 131 + E) * 131 + G + 7919 * salt)


def _ramps(T, E, G):
    """a per-token ramp [T, 1] and a per-channel ramp inside every group [1, E], both over [-1, 1]"""
    cg = E // G
    tr = torch.linspace(-1.0, 1.0, T).view(T, 1) if T > 1 else torch.zeros(1, 1)
    cr = (torch.linspace(-1.0, 1.0, cg) if cg > 1 else torch.zeros(1)).repeat(G).view(1, E)
    return tr, cr


@functools.lru_cache(maxsize=4)
def inputs(B, T, E, G):
    """float32 CPU tensors x, gamma, beta, dy, add.  x and dy are noise over a nonzero group mean plus a ramp over the tokens
    and one over the channels of each group: the last token and the last channel of a slab sit away from its mean, so a
    kernel that drops either moves the statistics by far more than the tolerance (the mutation check of the CPU test)"""
    g = _gen(B, T, E, G)
    tr, cr = _ramps(T, E, G)
    x = torch.randn(B, T, E, generator=g) * 1.3 + 0.7 + 0.5 * tr + 0.4 * cr
    dy = torch.randn(B, T, E, generator=g) + 0.5 + 1.0 * tr + 0.3 * cr
    add = torch.randn(B, T, E, generator=g)
    gamma = torch.randn(E, generator=g) * 0.3 + 1.0
    beta = torch.randn(E, generator=g) * 0.2
    return {"x": x.float(), "gamma": gamma.float(), "beta": beta.float(), "dy": dy.float(), "add": add.float()}


def hard_input(recipe, B, T, E, G):
    """the inputs of test_gpu_ops.py::test_groupnorm_chunked_statistics_hard_cases, for any shape: mean >> sigma; an outlier as
    the very first element of a slab and one in its middle; nearly constant data; a border (the first tokens of every sample)
    100 sigma away from the rest"""
    x = torch.randn(B, T, E, generator=_gen(B, T, E, G, salt=1 + HARD_RECIPES.index(recipe)))
    if recipe == "large_mean":
        x = x * 0.05 + 300.0
    elif recipe == "outlier_first":
        x[:, 0, 0] = 1.0e4
        x[:, T // 2, E // G] = -3.0e3
    elif recipe == "offset_border":
        x = x * 0.01
        x[:, :min(32, T // 2), :] += 1.0
    else:
        assert recipe == "tiny_variance"
        x = x * 1e-4 + 2.0
    return x.float()


def stats_ref(x, G, drop_token=False, drop_channel=False):
    """float64 (mean, biased variance) [B, G] of every (sample, group) slab, written out as sums; drop_token / drop_channel
    leave the slab's last token / the group's last channel out of them (the mutants of the CPU test)"""
    B, T, E = x.shape
    s = x.double().view(B, T, G, E // G)
    if drop_token:
        s = s[:, :-1]
    if drop_channel:
        s = s[:, :, :, :-1]
    n = s.shape[1] * s.shape[3]
    mean = s.sum(dim=(1, 3)) / n
    var = ((s - mean.view(B, 1, G, 1)) ** 2).sum(dim=(1, 3)) / n
    return mean, var


def forward_ref(t, G, **drop):
    """{y, mean, rstd} in float64 from the slab statistics of stats_ref"""
    x = t["x"]
    B, T, E = x.shape
    mean, var = stats_ref(x, G, **drop)
    rstd = 1.0 / torch.sqrt(var + EPS)
    xh = (x.double().view(B, T, G, E // G) - mean.view(B, 1, G, 1)) * rstd.view(B, 1, G, 1)
    y = xh.reshape(B, T, E) * t["gamma"].double() + t["beta"].double()
    return {"y": y, "mean": mean, "rstd": rstd, "xhat": xh.reshape(B, T, E)}


def backward_ref(t, G, drop_token=False, drop_channel=False):
    """{dx (without add), part [2, B, E], dgamma, dbeta} in float64.  Unmutated: dx, dgamma from autograd through
    torch.nn.functional.group_norm, part from the per-sample sums.  Mutated: the closed form with the last token / channel
    left out of every sum a kernel forms (the per-channel sums and the two group means)"""
    x, dy, gamma = t["x"].double(), t["dy"].double(), t["gamma"].double()
    B, T, E = x.shape
    cg = E // G
    f = forward_ref(t, G)
    xh = f["xhat"]
    keep = torch.ones(T, E, dtype=torch.float64)
    if drop_token:
        keep[-1, :] = 0
    if drop_channel:
        keep.view(T, G, cg)[:, :, -1] = 0
    part = torch.stack([(dy * xh * keep).sum(1), (dy * keep).sum(1)])
    if not (drop_token or drop_channel):
        xr, gr = x.clone().requires_grad_(True), gamma.clone().requires_grad_(True)
        yr = torch.nn.functional.group_norm(xr.transpose(1, 2), G, gr, t["beta"].double(), EPS).transpose(1, 2)
        yr.backward(dy)
        return {"dx": xr.grad, "part": part, "dgamma": gr.grad, "dbeta": dy.sum(dim=(0, 1))}
    n = T * cg
    m1 = (part[1] * gamma).view(B, G, cg).sum(2) / n
    m2 = (part[0] * gamma).view(B, G, cg).sum(2) / n
    rs = f["rstd"].view(B, 1, G, 1)
    dx = rs * ((gamma * dy).view(B, T, G, cg) - m1.view(B, 1, G, 1) - xh.view(B, T, G, cg) * m2.view(B, 1, G, 1))
    return {"dx": dx.reshape(B, T, E), "part": part, "dgamma": part[0].sum(0), "dbeta": part[1].sum(0)}


@functools.lru_cache(maxsize=2)
def reference(B, T, E, G):
    """the float64 reference of a shape, computed once and shared by the cases on it (callers must not modify it)"""
    t = inputs(B, T, E, G)
    ref = forward_ref(t, G)
    ref.update(backward_ref(t, G))
    return ref


# what the GPU test holds each output to: helpers.assert_close keywords (empty: its defaults, the 1e-4 north-star tolerance);
# mean / rstd as tests/test_gpu_ops.py::test_groupnorm_chunked_statistics_hard_cases, the column sums of the packs as
# test_groupnorm_bwd_writes_the_gradient_packs
TOL = {"y": {}, "dx": {}, "part": {}, "dgamma": {}, "dbeta": {},
       "mean": dict(rtol=1e-6, atol_scale=1e-6), "rstd": dict(rtol=2e-5, atol_scale=2e-5),
       "colsum": dict(rtol=1e-5, atol_scale=1e-5)}
