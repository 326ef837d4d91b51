"""CPU side of the streaming-kernel tests: the numpy Philox restatement against the Random123 known answers, the premise of
every shape in tests/streaming_cases.py (the library's own planners say it reaches the path it is there for), and the
channel limit of the noise entry points, which fails before any HIP call."""
import numpy as np
import pytest

import philox_ref
import streaming_cases as SC


@pytest.fixture(scope="module")
def built_lib():
    from dpot_amd import build
    return build.build(verbose=False)


@pytest.fixture(scope="module")
def lib(built_lib):
    from dpot_amd import _lib
    return _lib.load()


def cdiv(a, b):
    return -(-a // b)


def pow2_ge(c):
    p = 1
    while p < c:
        p *= 2
    return p


# ---- Philox4x32-10 ------------------------------------------------------------------------------------------------------
# Random123 kat_vectors, "philox4x32 10": counter, key -> output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("counter,key,want", KAT)
def test_philox_known_answers(counter, key, want):
    got = philox_ref.philox4x32_10(np.array(counter, dtype=np.uint32), key)
    assert [f"{int(v):08x}" for v in got] == [f"{v:08x}" for v in want]


def test_philox_is_vectorised_over_counters():
    ctr = np.array([k[0] for k in KAT[:1]] * 3 + [(1, 0, 0, 0)], dtype=np.uint32)
    got = philox_ref.philox4x32_10(ctr, (0, 0))
    assert got.shape == (4, 4) and (got[:3] == np.array(KAT[0][2], dtype=np.uint32)).all() and (got[3] != got[0]).any()


def test_normal4_counter_key_layout_and_mapping():
    """counter = {index lo, index hi, offset lo, offset hi}, key = {seed lo, seed hi}; uniforms in float32, Box-Muller in
    float64: the third known answer read as (seed, offset, index)"""
    (c0, c1, c2, c3), (k0, k1), out = KAT[2]
    z = philox_ref.normal4(k0 | (k1 << 32), c2 | (c3 << 32), np.array([c0 | (c1 << 32)], dtype=np.uint64))[0]
    s = np.float32(2.0 ** -32)
    u = [np.float32(np.float32(out[0]) * s + np.float32(2.0 ** -33)), np.float32(out[1]) * s,
         np.float32(np.float32(out[2]) * s + np.float32(2.0 ** -33)), np.float32(out[3]) * s]
    u = [float(v) for v in u]
    want = [np.sqrt(-2 * np.log(u[0])) * np.cos(2 * np.pi * u[1]), np.sqrt(-2 * np.log(u[0])) * np.sin(2 * np.pi * u[1]),
            np.sqrt(-2 * np.log(u[2])) * np.cos(2 * np.pi * u[3]), np.sqrt(-2 * np.log(u[2])) * np.sin(2 * np.pi * u[3])]
    assert np.allclose(z, want, rtol=1e-14, atol=0)
    # the extreme words: u0 = 1 (float(2^32 - 1) rounds up to 2^32) gives radius 0, not a NaN; word 0 gives a finite radius
    u0, u1, _, _ = philox_ref.uniforms(np.array([[0xffffffff, 0xffffffff, 0, 0]], dtype=np.uint32))
    assert u0[0] == 1.0 and u1[0] == 1.0
    u0, _, _, _ = philox_ref.uniforms(np.array([[0, 0, 0, 0]], dtype=np.uint32))
    assert u0[0] == np.float32(2.0 ** -33) and np.isfinite(np.sqrt(-2 * np.log(np.float64(u0[0]))))


def test_field_noise_index_rule_and_moments():
    e = philox_ref.field_noise(77, 3, 3, 4096)
    assert e.shape == (3, 4096)
    # element i of sample b = component i % 4 of counter b * n/4 + i // 4
    one = philox_ref.normal4(77, 3, np.array([2 * 1024 + 5], dtype=np.uint64))[0]
    assert (e[2, 20:24] == one).all()
    n = e.size
    assert abs(e.mean()) <= 5 / np.sqrt(n) and abs(e.var() - 1.0) <= 5 * np.sqrt(2.0 / n)
    assert not (philox_ref.field_noise(77, 4, 3, 4096) == e).any()           # the offset is part of the counter


# ---- premises: every shape reaches the path it is there for -------------------------------------------------------------
@pytest.mark.parametrize("case", SC.REL_L2, ids=lambda c: c.name)
def test_rel_l2_case_premise(lib, case):
    B, S, C, Tt = case.B, case.S, case.C, case.Tt
    assert case.shape[0] == B and case.shape[-1] == C and case.shape[-2] == Tt and int(np.prod(case.shape)) == B * S * C
    assert S % Tt == 0
    nch = lib.dpot_rel_l2_chunks(S, C)
    assert nch == case.chunks
    rows, TS = cdiv(S, nch), 1024 // pow2_ge(C)
    if case.name == "c4_pair_tail":
        # the float4 path: TS = 256 row lanes, two points in flight per trip; chunk 0 = rows [0, 515), chunk 1 = [515, 1029)
        assert (nch, rows, TS) == (2, 515, 256)
        assert rows - 2 * TS == 3 and S - rows - 2 * TS == 2              # one pair trip, then a 3- and a 2-point tail
        assert rows % Tt != 0                                             # chunk 1 starts inside a grid point's Tt steps
    if case.name == "c4_cap32":
        assert cdiv(S * C, 4096) > 32 and (nch - 1) * rows < S            # capped, and every chunk has rows
    if case.name == "c4_misaligned":
        assert case.off % 4 != 0
    if case.name == "c1024":
        assert TS == 1 and rows == 5 and nch - cdiv(S, rows) == 6         # six chunks wholly past S
    if case.C not in (3, 4):
        assert pow2_ge(C) != 4
    if case.name == "c40":
        assert pow2_ge(C) - C == 24 and rows % Tt != 0
    if case.name in ("c3", "c5"):
        assert pow2_ge(C) > C                                             # idle tc >= C lanes


@pytest.mark.parametrize("case", SC.NOISE_ALL, ids=lambda c: c.name)
def test_noise_case_premise(lib, case):
    B, S, C = SC.field_dims(case.shape)
    assert (B, S, C) == (case.B, case.S, case.C) and C <= SC.NOISE_MAX_C
    assert lib.dpot_noise_chunks(S, C) == case.chunks


def test_noise_path_premises(lib):
    by = {c.name: c for c in SC.NOISE_FWD}
    c = by["c4_deep_tail"]                       # 256 threads, four float4 in flight: a trip needs s + 768 < S
    assert c.S > 768 + 255 and c.S % 1024 != 0 and c.S - 1024 < 1024
    c = by["c4_two_chunks"]
    assert cdiv(c.S, c.chunks) == 1025             # per chunk: one 4-deep trip of 1024 points and a one-point tail
    c = by["c2_odd"]                             # the float4 eps path needs S*C % 4 == 0; sample bases are 8 bytes off
    assert (c.S * c.C) % 4 == 2
    for name in ("c8", "c12"):                   # float4 eps path with a wrapping (c0 + k) % C
        assert by[name].C % 4 == 0 and by[name].C > 4
    assert 256 // pow2_ge(by["c256"].C) == 1 and 256 // pow2_ge(by["c40"].C) == 4
    # backward: chunks are multiples of 4 on the flattened (s, c) axis
    c = SC.NOISE_BWD[0]
    per = cdiv(c.S * c.C // 4, c.chunks) * 4
    assert per == 4100 and per % c.C != 0
    # generator: S*C % 4 == 0 everywhere; the C == 4 loop strides 512 float4 per workgroup with the second at q + 256
    for c in SC.NOISE_RNG:
        assert (c.S * c.C) % 4 == 0
    c = SC.NOISE_RNG[0]
    n4 = c.S * c.C // 4
    # the last workgroup's thread t holds float4 q = 1536 + t and its partner q + 256: only t = 255 has q + 256 == n4
    assert c.C == 4 and n4 % 512 == 511 and cdiv(n4, 512) <= cdiv(2048, c.B)
    c = SC.NOISE_RNG[1]                          # the second workgroup: 8 threads with a float4, none with a partner
    assert c.C == 4 and (c.S * c.C // 4) % 512 == 8
    assert SC.NOISE_RNG[2].C % 4 != 0 and SC.NOISE_RNG[3].C % 4 != 0


@pytest.mark.parametrize("case", SC.COLSUM, ids=lambda c: f"{c.M}x{c.N}")
def test_colsum_case_premise(lib, case):
    width = 16 if case.N <= 16 else 32 if case.N <= 32 else 64
    assert width == case.width
    parts = min(lib.dpot_colsum_parts(case.M), cdiv(1024, cdiv(case.N, width)))
    assert parts == case.parts


def test_colsum_instantiations_covered(lib):
    assert {c.width for c in SC.COLSUM} == {16, 32, 64}
    assert any(c.parts == 1 for c in SC.COLSUM) and any(c.parts > 1 for c in SC.COLSUM)
    M, N, parts, segs = SC.COLSUM_SCATTER
    assert min(lib.dpot_colsum_parts(M), cdiv(1024, cdiv(N, 32))) == parts
    covered = sorted(j for s, n in segs for j in range(s, s + n))
    assert len(covered) == len(set(covered)) < N and max(covered) == N - 1           # a gap, no overlap, the last column used


def test_small_op_premises():
    assert min(SC.TOKEN_MEAN_T) < 4 and {28, 29}.issubset(SC.TOKEN_MEAN_T) and all(e > 64 for e in SC.TOKEN_MEAN_E)
    assert any(e > 256 for _, e in SC.TIMEAGG) and any(e % 256 for _, e in SC.TIMEAGG)
    for B, X, Y, T, C, P in SC.PATCHIFY:
        assert X != Y and X % P == 0 and Y % P == 0
    B, X, Y, T, C, P = SC.PATCHIFY[0]
    assert (C + 3) * P * P == 320 and P * T * C == 48
    B, X, Y, T, C, P = SC.PATCHIFY[1]
    assert P * T * C == 280


# ---- the channel limit of the noise kernels -------------------------------------------------------------------------------
def test_noise_entry_points_refuse_more_than_256_channels(lib):
    """chan_sumsq_part_kernel gives every channel a lane of a 256-thread block; above 256 channels its row loop would not
    advance.  The requirement fails before any HIP call, so dummy (non-null, 16-byte aligned) addresses are enough."""
    a = [0x10000 * (k + 1) for k in range(7)]
    B, S, C = 1, 4, SC.NOISE_MAX_C + 1
    calls = {
        "noise_inject": lambda: lib.dpot_noise_inject(a[0], a[1], a[2], a[3], 0.05, B, S, C, None),
        "noise_inject_rng": lambda: lib.dpot_noise_inject_rng(a[0], a[2], a[3], a[4], 0.05, B, S, C, None),
        "noise_inject_bwd": lambda: lib.dpot_noise_inject_bwd(a[0], a[1], None, a[2], a[3], a[5], a[6], 0.05, B, S, C, None),
    }
    for name, call in calls.items():
        assert call() != 0, name
        msg = lib.dpot_last_error().decode()
        assert msg.startswith(name + ":") and "channels" in msg and "257" in msg and "limit of 256" in msg, msg


def test_noise_dims_docstring_names_the_limit():
    from dpot_amd import ops
    assert "C' > 256" in ops.noise_dims.__doc__ and "1024" not in ops.noise_dims.__doc__
