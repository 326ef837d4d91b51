"""Host side of the batched weight-gradient launches (csrc/gemm_tn.hip): the one-round split / group rule (what DPOT_TUNE
fused_small=3 launches; the default batch keeps the per-block split factors) through its C queries - no GPU needed.  For every launch the rule plans: at most 256 workgroups (one round of the chip) where the rule promises it,
no empty token range, and the ranges cover the tokens exactly once."""
import ctypes as C

import pytest


@pytest.fixture(scope="module")
def lib():
    from dpot_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def _ranges(lib, T, splits):
    out = []
    for i in range(splits):
        t0, n = C.c_int(-1), C.c_int(-1)
        assert lib.dpot_tn_split_range(T, splits, i, C.byref(t0), C.byref(n)) == 0
        out.append((t0.value, n.value))
    return out


def _check_cover(lib, T, splits, what):
    r = _ranges(lib, T, splits)
    assert all(n > 0 and n % 32 == 0 for _, n in r), (what, r)               # every range non-empty, whole slabs
    pos = 0
    for t0, n in r:                                                           # in order, adjacent: each token exactly once
        assert t0 == pos, (what, r)
        pos += n
    assert pos == T, (what, r)


def _afno_plan(lib, Mm, nb, bs, n):
    s12, s = C.c_int(0), C.c_int(0)
    per = lib.dpot_afno_wgrad_batch_plan(Mm, nb, bs, n, C.byref(s12), C.byref(s))
    return per, s12.value, s.value


# (depth, nb) at 128 channels per AFNO block; Mm = 32 samples x 16 x 9 modes, 8192 tokens (DPOT-Tiny's batch-32 step), and a
# short, ragged token count; depth 40: more sets than the problem table holds (32)
@pytest.mark.parametrize("depth,nb", [(4, 4), (6, 8), (12, 8), (40, 4), (40, 1)])
@pytest.mark.parametrize("Mm,T", [(4608, 8192), (32 * 29, 32 * 37)])
def test_split_and_group_rule(lib, depth, nb, Mm, T):
    cap = lib.dpot_wgrad_batch_max_blocks()
    assert cap >= 12                                                          # DPOT-M's depth fits one problem table
    E = mh = nb * 128
    # AFNO: blocks per launch and the two split factors
    per, s12, s = _afno_plan(lib, Mm, nb, 128, depth)
    assert 1 <= per <= min(depth, cap) and 1 <= s12 <= s
    assert 2 * per * nb * (2 * s12 + s) <= 256
    _check_cover(lib, Mm, s12, f"afno P1/P2 depth {depth} nb {nb}")
    _check_cover(lib, Mm, s, f"afno sum product depth {depth} nb {nb}")
    # channel MLP: launches of at most `cap` blocks, max(1, 256 / tiles) ranges
    sk = lib.dpot_mlp_wgrad_batch_splitk(T, E, mh, depth)
    assert sk >= 1
    launches = -(-depth // cap)
    per_m = -(-depth // launches)
    assert 2 * per_m <= 2 * cap
    tiles = 2 * per_m * (E // 128) * (mh // 128)
    assert tiles * sk <= max(256, tiles)                                      # one round unless the tiles alone exceed it
    _check_cover(lib, T, sk, f"mlp depth {depth} nb {nb}")


def test_rule_at_the_headline_shapes(lib):
    """DPOT-Tiny (depth 4, nb 4): two blocks per AFNO launch at (5, 6) - 256 workgroups - and 128 channel-MLP tiles x 2;
    nb = 8 (DPOT-S / -M): one block already is 16 problems, no batch; 96 channels per block (DPOT-L): not covered"""
    assert _afno_plan(lib, 4608, 4, 128, 4) == (2, 5, 6)
    assert lib.dpot_mlp_wgrad_batch_splitk(8192, 512, 512, 4) == 2
    assert _afno_plan(lib, 4608, 8, 128, 6)[0] == 1 and _afno_plan(lib, 4608, 8, 128, 12)[0] == 1
    assert _afno_plan(lib, 4608, 16, 96, 24)[0] == 0
    assert lib.dpot_mlp_wgrad_batch_splitk(8192, 500, 512, 4) == 0
