"""CPU tests of the 3-D Fourier resize's host side (ops.spectral_resize3_terms, ops.Resize3Plan.host_matrices) against the
float64 rfftn restatement (tests/resize3_ref.py), its tie to the reference-pinned 2-D definition (tests/resize_ref.py), the
ABI of the new entry points, and the refusals that need no GPU."""
import os
import re
import subprocess

import numpy as np
import pytest
import torch

from resize3_ref import resize3_ref, resize3_torch
from resize_ref import hash_field, resize_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# every parity pattern, both directions, the two-term pairs on each axis, more than one 16- and 32-row tile
SIZES = [((8, 8, 8), (5, 5, 5)), ((5, 6, 7), (8, 8, 8)), ((16, 16, 16), (8, 8, 8)), ((8, 8, 8), (16, 16, 16)),
         ((8, 8, 8), (8, 8, 8)), ((10, 12, 6), (16, 14, 9)), ((6, 10, 12), (9, 16, 7)), ((33, 20, 18), (34, 17, 24))]
IDS = ["x".join(map(str, n)) + "-" + "x".join(map(str, m)) for n, m in SIZES]


def field(n, B=2, TC=3, salt=1):
    return hash_field((B,) + tuple(n) + (TC,), salt).astype(np.float64)


def apply_terms(terms, x, n):
    out = 0.0
    for sign, ax, ay, az in terms:
        out = out + sign * np.einsum("ux,vy,wz,bxyzp->buvwp", ax, ay, az, x, optimize=True)
    return out / float(np.prod(n))


@pytest.mark.parametrize("n,m", SIZES, ids=IDS)
def test_surviving_terms_equal_the_rfftn_restatement(n, m):
    """the derivation: Re(Dx (x) Dy (x) Dz) = Rx Ry Rz - Rx Iy Iz - Ix Ry Iz - Ix Iy Rz with the rank-one Ix, Iy, a term only
    where its imaginary factors exist - in float64 against rfftn / irfftn, and the count of terms per parity pattern"""
    from dpot_amd import ops
    terms = ops.spectral_resize3_terms(*n, *m)
    ex = n[0] != m[0] and min(n[0], m[0]) % 2 == 0
    ey = n[1] != m[1] and min(n[1], m[1]) % 2 == 0
    assert len(terms) == {(False, False): 1, (True, False): 2, (False, True): 2, (True, True): 4}[(ex, ey)]
    x = field(n)
    want = resize3_ref(x, m)
    got = apply_terms(terms, x, n)
    err = np.abs(got - want).max()
    print(f"terms {n} -> {m}: {len(terms)} terms, max |err| {err:.2e} at scale {np.abs(want).max():.2e}")
    assert err <= 1e-12 * max(1.0, np.abs(want).max())


def apply_host_matrices(h, x, n, m):
    """what the launches of csrc/resize3.hip compute, in float64 from the plan's fp32 matrices: P on every (b, x) plane, the
    X contraction, and (where Im Dx exists) -ux (x) Q(sum_x vx in); returns the result and sum |operator| |x| for the bound"""
    nx, ny, nz = n
    mx, my, mz = m
    d = {k: (None if v is None else v.astype(np.float64)) for k, v in h.items()}
    rx, ry = d["rxT"][:nx, :mx], d["ryT"][:ny, :my]
    rz = d["rzT"][:nz, :mz]

    def plane(f, az, bz, u, absolute=False):
        a = (lambda t: np.abs(t)) if absolute else (lambda t: t)
        o = np.einsum("yv,zw,b...yzp->b...vwp", a(ry), a(az), f, optimize=True)
        if d["uy2"] is not None:
            w = np.einsum("y,b...yzp->b...zp", a(d["vy"][:ny]), f)
            o = o + np.einsum("v,zw,b...zp->b...vwp", a(u[:my]), a(bz), w, optimize=True)
        return o

    def run(f, absolute):
        a = (lambda t: np.abs(t)) if absolute else (lambda t: t)
        iz = None if d["izT"] is None else d["izT"][:nz, :mz]
        nuy, uy = (d["uy2"][1], d["uy2"][0]) if d["uy2"] is not None else (None, None)
        out = np.einsum("xu,bxvwp->buvwp", a(rx), plane(f, rz, iz, nuy, absolute), optimize=True)
        if d["nux"] is not None:
            s = np.einsum("x,bxyzp->byzp", a(d["vx"][:nx]), f)
            out = out + np.einsum("u,bvwp->buvwp", a(d["nux"][:mx]), plane(s, iz, rz, uy, absolute))
        return out

    return run(x, False), run(np.abs(x), True)


@pytest.mark.parametrize("n,m", SIZES, ids=IDS)
def test_plan_host_matrices_assemble_the_operator_and_have_the_promised_shapes(n, m):
    from dpot_amd import ops
    h = ops.Resize3Plan.host_matrices(*n, *m)
    nxp, nyp, nzp, mxp, myp, mzp = ops.Resize3Plan.pads(*n, *m)
    assert (nxp % 16, nyp % 16, nzp % 16, mxp % 32, myp % 32, mzp % 16) == (0,) * 6
    assert all(0 <= p - s < q for p, s, q in zip((nxp, nyp, nzp, mxp, myp, mzp), n + m, (16, 16, 16, 32, 32, 16)))
    ex = n[0] != m[0] and min(n[0], m[0]) % 2 == 0
    ey = n[1] != m[1] and min(n[1], m[1]) % 2 == 0
    shapes = {"rxT": (nxp, mxp), "ryT": (nyp, myp), "rzT": (nzp, mzp), "izT": (nzp, mzp) if ex or ey else None,
              "nux": (mxp,) if ex else None, "vx": (nxp,) if ex else None, "uy2": (2, myp) if ey else None,
              "vy": (nyp,) if ey else None}
    assert set(h) == set(shapes)
    for k, shp in shapes.items():
        if shp is None:
            assert h[k] is None, k
            continue
        assert h[k].dtype == np.float32 and h[k].shape == shp and h[k].flags.c_contiguous, k
    # the padding is zero: a kernel that reads a padded row or column adds nothing
    for k, (r, c) in {"rxT": (n[0], m[0]), "ryT": (n[1], m[1]), "rzT": (n[2], m[2])}.items():
        assert not h[k][r:].any() and not h[k][:, c:].any(), k
    if ey:
        assert np.array_equal(h["uy2"][1], -h["uy2"][0]) and not h["uy2"][:, m[1]:].any() and not h["vy"][n[1]:].any()
    if ex:
        assert not h["nux"][m[0]:].any() and not h["vx"][n[0]:].any()
    x = field(n)
    got, mag = apply_host_matrices(h, x, n, m)
    want = resize3_ref(x, m)
    # each of the three factors of a product is rounded once to fp32: (1 + 2^-24)^3 - 1 < 4 * 2^-24 of sum |op| |x|
    bound = 4.0 * 2.0 ** -24 * mag + 1e-13
    worst = float((np.abs(got - want) / bound).max())
    print(f"host matrices {n} -> {m}: worst |err| / bound {worst:.3f}")
    assert worst <= 1.0


@pytest.mark.parametrize("nz,mz", [(8, 5), (7, 8), (8, 16), (8, 8), (6, 9), (12, 7)])
@pytest.mark.parametrize("nxy,mxy", [((8, 8), (5, 5)), ((10, 12), (16, 14)), ((6, 10), (9, 16))])
def test_a_field_constant_along_one_axis_resizes_as_the_2d_definition(nxy, mxy, nz, mz):
    """The tie to the reference-pinned 2-D restatement (tests/resize_ref.py).
    Constant along X: only k_x = 0 is excited, the (Y, Z) planes are a full-spectrum and a half-spectrum axis as the 2-D
    field's (X, Y) are, so every X slice is resize_ref of the plane - for every size pair.
    Constant along Z: only k_z = 0 is excited and every Z slice is Re(Dx (x) Dy) in / (n_x n_y) with BOTH axes full-spectrum
    (resize_ref.axis_operator(..., half=False)).  That equals resize_ref itself exactly where Y has no unpaired frequency
    (min(n_y, m_y) odd, or n_y == m_y): the 2-D definition keeps +-h of its half-spectrum axis as a pair, the row rule of a
    full-spectrum axis keeps -h alone, and the two differ by Im Dx (x) sin(h ...) on a two-term pair."""
    from resize_ref import axis_operator
    (n1, n2), (m1, m2) = nxy, mxy
    x2 = hash_field((2, n1, n2, 3), 5).astype(np.float64)
    # constant along Z
    x3 = np.repeat(x2[:, :, :, None, :], nz, axis=3)
    got = resize3_ref(x3, (m1, m2, mz))
    assert got.shape == (2, m1, m2, mz, 3)
    full = np.einsum("ux,vy,bxyp->buvp", axis_operator(n1, m1, False), axis_operator(n2, m2, False),
                     x2.astype(np.complex128), optimize=True).real / (n1 * n2)
    assert np.abs(got - full[:, :, :, None, :]).max() <= 1e-12
    if n2 == m2 or min(n2, m2) % 2:
        assert np.abs(got - resize_ref(x2, (m1, m2))[:, :, :, None, :]).max() <= 1e-12
    # constant along X (n_x = nz -> m_x = mz): the planes (Y, Z) = the 2-D field's (X, Y)
    x3 = np.repeat(x2[:, None], nz, axis=1)
    got = resize3_ref(x3, (mz, m1, m2))
    assert np.abs(got - resize_ref(x2, (m1, m2))[:, None]).max() <= 1e-12


def test_up_then_down_is_the_identity_on_band_limited_fields_and_equal_sizes_keep_everything():
    from dpot_amd import ops
    x = field((6, 7, 8), B=1, TC=2, salt=3)
    same = resize3_ref(x, (6, 7, 8))
    assert np.abs(same - x).max() <= 1e-13                                 # every frequency is kept
    assert np.abs(apply_terms(ops.spectral_resize3_terms(6, 7, 8, 6, 7, 8), x, (6, 7, 8)) - x).max() <= 1e-13
    low = resize3_ref(x, (5, 5, 5))                                        # odd sizes: no unpaired frequency, band-limited
    up = resize3_ref(low, (9, 12, 16))
    back = resize3_ref(up, (5, 5, 5))
    assert np.abs(back - low).max() <= 1e-12
    t = apply_terms(ops.spectral_resize3_terms(9, 12, 16, 5, 5, 5), up, (9, 12, 16))
    assert np.abs(t - low).max() <= 1e-12


def test_the_float32_torch_composition_is_the_restatement():
    x = hash_field((2, 10, 12, 6, 3), 9)
    got = resize3_torch(torch.from_numpy(x).double(), (16, 14, 9)).numpy()
    assert np.abs(got - resize3_ref(x, (16, 14, 9))).max() <= 1e-12


def test_product_path_refuses_cpu_tensors_and_bad_sizes():
    import dpot_amd
    from dpot_amd import _lib, infer, ops
    for name in ("spectral_resize3", "resize3_plan", "Resize3Plan", "Resized3D"):
        assert name in dpot_amd.__all__ and hasattr(dpot_amd, name), name
    assert dpot_amd.Resized3D is infer.Resized3D
    with pytest.raises(_lib.DpotHipError, match="no CPU path"):
        ops.spectral_resize3(torch.zeros(1, 8, 8, 8, 1, 1), 6)
    with pytest.raises(_lib.DpotHipError, match=">= 2"):
        ops.resize3_plan(8, 8, 1, 8, 8, 8, "cpu")
    cap = _lib.load().dpot_spectral_resize3_max_size()
    with pytest.raises(_lib.DpotHipError, match=str(cap + 1)):
        ops.resize3_plan(8, 8, 8, 8, cap + 1, 8, "cpu")
    with pytest.raises(ValueError, match="model_res"):
        infer.Resized3D(torch.nn.Identity(), (8, 8))
    w = infer.Resized3D(torch.nn.Identity(), 8)
    assert w.model_res == (8, 8, 8) and list(w.parameters()) == []
    with pytest.raises(ValueError, match="6-D"):
        w(torch.zeros(1, 8, 8, 1, 1))
    with pytest.raises(_lib.DpotHipError, match="no CPU path"):
        w(torch.zeros(1, 6, 6, 6, 1, 1))


def test_header_ctypes_table_and_exported_symbols_agree():
    from dpot_amd import _lib, build
    with open(os.path.join(ROOT, "include", "dpot_hip.h")) as f:
        header = f.read()
    declared = sorted(set(re.findall(r"^(?:int|int64_t)\s+(dpot_spectral_resize3\w*)\(", header, flags=re.M)))
    assert declared == ["dpot_spectral_resize3", "dpot_spectral_resize3_max_size", "dpot_spectral_resize3_pad",
                        "dpot_spectral_resize3_ws_elems"]
    assert sorted(n for n in _lib.SIGNATURES if n.startswith("dpot_spectral_resize3")) == declared
    assert "resize3.hip" in build.SOURCES
    lib = _lib.load()
    assert lib.dpot_version() >= 279
    exported = subprocess.check_output(["nm", "-D", "--defined-only", build.LIB], text=True)
    for name in declared:
        assert f" T {name}\n" in exported, name
        proto = re.search(r"^(?:int|int64_t)\s+" + name + r"\(([^;]*)\);", header, flags=re.M | re.S).group(1)
        n_args = 0 if proto.strip() == "void" else len(proto.split(","))
        assert n_args == len(_lib.SIGNATURES[name][1]), name
    assert lib.dpot_spectral_resize3_max_size() >= 128
    assert [lib.dpot_spectral_resize3_pad(41, r) for r in (0, 1)] == [48, 64]
    # the workspace is the smaller intermediate: planes first when shrinking, the X pass first when growing; two-term X pairs
    # add one input plane and one output plane per sample
    ws = lib.dpot_spectral_resize3_ws_elems
    assert ws(1, 128, 128, 128, 64, 64, 64, 4) == 4 * (128 * 64 * 64 + 128 * 128 + 64 * 64)
    assert ws(1, 64, 64, 64, 128, 128, 128, 40) == 40 * (128 * 64 * 64 + 64 * 64 + 128 * 128)
    assert ws(2, 5, 6, 7, 8, 8, 8, 3) == 2 * 3 * min(5 * 8 * 8, 8 * 6 * 7)
    assert ws(1, 8, 8, 1, 8, 8, 8, 1) == 0 and b"spectral_resize3" in lib.dpot_last_error()
    assert ws(1, 8, 8, 8, 8, 8, lib.dpot_spectral_resize3_max_size() + 1, 1) == 0
    rc = lib.dpot_spectral_resize3(*([None] * 11), 1, 8, 8, 8, 8, 8, 8, 1, None)
    assert rc != 0 and b"spectral_resize3" in lib.dpot_last_error()
