"""GPU tests of csrc/patch3d.hip - ops.patchify3 / unpatchify3 / fold3 - against the torch index expressions they replace (kept
here as the yardstick: DPOTNet3D built its patch matrix this way before the kernels, functional._unfold3 / _fold3 are the
statement of fold3).  Pure fp32 data movement: every comparison is torch.equal.  Buffers are guarded and NaN-poisoned
(tests/guard.py), so an unwritten element or a stray write shows."""
import functools

import numpy as np
import pytest
import torch

import guard
from guard import guarded  # noqa: F401  (fixture)

pytestmark = pytest.mark.gpu

# (B, S, P, T, C)
SHAPES = [(2, 8, 2, 3, 2),          # MINI3D
          (2, 12, 3, 3, 2),         # odd patch: runs of 9 / 27 / 18 floats, scalar paths
          (1, 16, 8, 10, 4),        # the reference patch and window, h = 2: the 16-byte paths
          (3, 6, 1, 2, 1),          # P = 1: every patch one voxel
          (1, 10, 5, 1, 3)]         # T = 1, odd everything
IDS = ["x".join(map(str, s)) for s in SHAPES]
OLDS = [32, 5]


def tables(S, T):
    """coordinate tables of get_grid_4d, as DPOTNet3D registers them"""
    return (torch.tensor(np.linspace(0, 1, S), dtype=torch.float32), torch.tensor(np.linspace(0, 1, T), dtype=torch.float32))


def patch_matrix(x, gs, gt, P):
    """the patch matrix as DPOTNet3D._forward built it in torch: four coordinate channels x, y, z, t appended, then rows
    ((b, t), hx, hy, hz), columns (c, i, j, k)"""
    B, S, _, _, T, Cin = x.shape
    h = S // P
    grid = torch.stack([gs.view(S, 1, 1, 1).expand(S, S, S, T), gs.view(1, S, 1, 1).expand(S, S, S, T),
                        gs.view(1, 1, S, 1).expand(S, S, S, T), gt.view(1, 1, 1, T).expand(S, S, S, T)], dim=-1)
    Cc = Cin + 4
    xg = torch.cat([x, grid.unsqueeze(0).expand(B, S, S, S, T, 4)], dim=-1)
    return xg.view(B, h, P, h, P, h, P, T, Cc).permute(0, 7, 1, 3, 5, 8, 2, 4, 6).reshape(B * T * h ** 3, Cc * P ** 3)


@functools.lru_cache(maxsize=None)
def case(i):
    """CPU inputs and expectations of SHAPES[i], computed once and shared (never modified)"""
    B, S, P, T, C = SHAPES[i]
    gen = torch.Generator().manual_seed(4100 + i)
    x = torch.randn(B, S, S, S, T, C, generator=gen).requires_grad_(True)
    gs, gt = tables(S, T)
    A = patch_matrix(x, gs, gt, P)
    dA = torch.randn(A.shape, generator=gen)
    dx, = torch.autograd.grad(A, x, dA)
    return dict(x=x.detach(), gs=gs, gt=gt, A=A.detach(), dA=dA, dx=dx)


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_patchify3_equals_the_torch_expression(i, guarded):
    from dpot_amd import ops
    B, S, P, T, C = SHAPES[i]
    c = case(i)
    got = ops.patchify3(guard.wrap(c["x"], "cuda"), guard.wrap(c["gs"], "cuda"), guard.wrap(c["gt"], "cuda"), P)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B * T * (S // P) ** 3, (C + 4) * P ** 3)
    assert torch.equal(got.cpu(), c["A"])


@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_unpatchify3_equals_the_autograd_gradient(i, guarded):
    from dpot_amd import ops
    B, S, P, T, C = SHAPES[i]
    c = case(i)
    got = ops.unpatchify3(guard.wrap(c["dA"], "cuda"), B, S, T, C, P)
    torch.cuda.synchronize()
    assert tuple(got.shape) == (B, S, S, S, T, C)
    assert torch.equal(got.cpu(), c["dx"])


def test_unaligned_bases_take_the_scalar_path(guarded):
    """P = 8 with bases off the 16-byte grid: the float4 paths need a proof of alignment, these calls give none"""
    from dpot_amd import _lib, ops
    i = 2
    B, S, P, T, C = SHAPES[i]
    c = case(i)
    x = guard.wrap(torch.cat([torch.zeros(1), c["x"].reshape(-1)]), "cuda")[1:].view(c["x"].shape)
    assert x.data_ptr() % 16 == 4 and x.is_contiguous()
    got = ops.patchify3(x, guard.wrap(c["gs"], "cuda"), guard.wrap(c["gt"], "cuda"), P)
    dA = guard.wrap(torch.cat([torch.zeros(3), c["dA"].reshape(-1)]), "cuda")[3:].view(c["dA"].shape)
    got_dx = ops.unpatchify3(dA, B, S, T, C, P)
    # the C entry point writing to an unaligned destination
    out = guard.full_nan((c["A"].numel() + 1,))
    lib = _lib.load()
    xa = guard.wrap(c["x"], "cuda")
    assert lib.dpot_patchify3(xa.data_ptr(), guard.wrap(c["gs"], "cuda").data_ptr(), guard.wrap(c["gt"], "cuda").data_ptr(),
                              out[1:].data_ptr(), B, S, T, C, P, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(got.cpu(), c["A"])
    assert torch.equal(got_dx.cpu(), c["dx"])
    assert torch.equal(out[1:].cpu().view(c["A"].shape), c["A"]) and bool(out[0].isnan())


@pytest.mark.parametrize("old", OLDS)
@pytest.mark.parametrize("i", range(len(SHAPES)), ids=IDS)
def test_fold3_both_directions(i, old, guarded):
    from dpot_amd import ops
    from dpot_amd.functional import _fold3, _unfold3
    B, S, P, _, _ = SHAPES[i]
    h = S // P
    gen = torch.Generator().manual_seed(4200 + 10 * i + old)
    t = torch.randn(B * h ** 3, old * P ** 3, generator=gen)
    u = torch.randn(B * S ** 3, old, generator=gen)
    fwd = ops.fold3(guard.wrap(t, "cuda"), B, h, P, old)
    inv = ops.fold3(guard.wrap(u, "cuda"), B, h, P, old, inverse=True)
    back = ops.fold3(fwd, B, h, P, old, inverse=True)
    torch.cuda.synchronize()
    assert tuple(fwd.shape) == (B * S ** 3, old) and tuple(inv.shape) == (B * h ** 3, old * P ** 3)
    assert torch.equal(fwd.cpu(), _unfold3(t, B, h, P, old))
    assert torch.equal(inv.cpu(), _fold3(u, B, h, P, old))
    assert torch.equal(back.cpu(), t)                                   # inverse after forward: the identity


def test_bad_arguments_return_an_error_and_launch_nothing(guarded):
    from dpot_amd import _lib, ops
    lib = _lib.load()
    s = torch.cuda.current_stream().cuda_stream
    d = guard.wrap(torch.zeros(64), "cuda")
    p = d.data_ptr()
    assert lib.dpot_patchify3(p, p, p, p, 1, 5, 1, 1, 2, s) == -1             # S % P != 0
    assert lib.dpot_patchify3(p, p, p, None, 1, 4, 1, 1, 2, s) == -1          # null pointer
    assert lib.dpot_unpatchify3(p, p, 1, 4, 0, 1, 2, s) == -1                 # T = 0
    assert lib.dpot_fold3(p, p, 1, 2, 0, 4, 0, s) == -1                       # P = 0
    assert lib.dpot_patchify3(p, p, p, p, 1, 64, 64, 64, 64, s) == -1         # a slab beyond the LDS
    with pytest.raises(_lib.DpotHipError):
        ops.fold3(d.view(8, 8), 1, 2, 2, 3)                                   # shape does not match B, h, P, old
    torch.cuda.synchronize()
    assert not d.any()


def test_kernels_replay_bit_for_bit_inside_a_graph():
    from dpot_amd import ops
    i = 2
    B, S, P, T, C = SHAPES[i]
    c = case(i)
    x, gs, gt, dA = (c[k].cuda() for k in ("x", "gs", "gt", "dA"))
    old, h = 32, S // P
    t = torch.randn(B * h ** 3, old * P ** 3, device="cuda")

    def body():
        A = ops.patchify3(x, gs, gt, P)
        f = ops.fold3(t, B, h, P, old)
        return A, ops.unpatchify3(dA, B, S, T, C, P), f, ops.fold3(f, B, h, P, old, inverse=True)

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eager = [o.clone() for o in body()]
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        outs = body()
    for o in outs:
        o.fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    for o, e in zip(outs, eager):
        assert torch.equal(o, e)
    assert torch.equal(outs[0].cpu(), c["A"]) and torch.equal(outs[3], t)


def test_indices_past_2_to_31(guarded):
    """B*T*h^3 * (C+4)*P^3 = 2^31 + 2^24 patch-matrix elements: the last sample's rows sit past a 32-bit index on the
    rows side of all three kernels.  Checked on the last sample alone (the torch expression of the whole would take minutes)."""
    from dpot_amd import ops
    B, S, P, T, C = 129, 64, 8, 8, 4
    h = S // P
    gs, gt = tables(S, T)
    x = torch.randn(B, S, S, S, T, C, device="cuda")
    A = ops.patchify3(x, gs.cuda(), gt.cuda(), P)
    assert A.numel() > 2 ** 31
    rows = T * h ** 3
    want = patch_matrix(x[-1:].cpu(), gs, gt, P)
    assert torch.equal(A[-rows:].cpu(), want)
    assert torch.equal(A[:rows].cpu(), patch_matrix(x[:1].cpu(), gs, gt, P))
    dx = ops.unpatchify3(A, B, S, T, C, P)                             # the adjoint of a gather of x returns x
    torch.cuda.synchronize()
    assert torch.equal(dx[-1], x[-1]) and torch.equal(dx[0], x[0])
    del dx, x
    # fold3 on the same buffer read as [B*T * h^3, old * P^3], old = C + 4: its rows side past a 32-bit index as well
    from dpot_amd.functional import _unfold3
    f = ops.fold3(A, B * T, h, P, C + 4)
    torch.cuda.synchronize()
    assert torch.equal(f[-S ** 3:], _unfold3(A[-h ** 3:], 1, h, P, C + 4))
    assert torch.equal(f[:S ** 3], _unfold3(A[:h ** 3], 1, h, P, C + 4))
