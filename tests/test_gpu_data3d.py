"""GPU tests of the 3-D device-side input pipeline (csrc/data3d.hip, dpot_amd/data.py): trilinear resize + channel pad +
temporal window + strided sub-sampling against the golden vectors of the reference's TemporalDataset3D (g19) and the CPU
restatement (tests/data3d_ref.py), the caller-supplied output buffers, the double-buffered DeviceBatcher3D, and one batch
taken through a training step of a tiny DPOTNet3D.

Tolerance of kernel against reference: rtol 1e-6 and 1e-6 of the tensor's magnitude, the 2-D test's.  A float32 restatement
of the kernel's arithmetic in another association order than ATen's stays within 0.21 of it, torch's own float32 result
is within 0.52 of its float64 one; a wrong weight or index is orders of magnitude outside."""
import numpy as np
import pytest
import torch

import data3d_ref as D3
import guard
from guard import guarded  # noqa: F401  (fixture)
from helpers import RTOL, assert_close, load

pytestmark = pytest.mark.gpu

TOL = dict(rtol=1e-6, atol_scale=1e-6)


def _ref(raw, res, nc, t0, t_in, t_ar, down=(1, 1, 1)):
    """(x, y) of one raw sample [H,W,L,T,C] by the restatement"""
    return D3.downsample3(*D3.window(D3.pad_data3(raw, res, nc), t0, t_in, t_ar), down)


def test_kernel_matches_golden_training_cases(guarded):
    from dpot_amd.data import resize_pad_window3
    fx = load("g19_data3d")
    for k in range(4):
        H, W, L, T, Cc, res, nc, t_in, t_ar, t0 = (int(v) for v in fx[f"c{k}.meta"])
        raw = guard.wrap(D3.recipe_sample3((H, W, L, T, Cc), salt=100 + k), "cuda")
        xx, yy = resize_pad_window3([raw], [t0], res, t_in, t_ar, nc)
        assert_close(xx[0], fx[f"c{k}.x"], f"case {k} x", **TOL)
        assert_close(yy[0], fx[f"c{k}.y"], f"case {k} y", **TOL)


def test_kernel_matches_golden_test_mode_cases(guarded):
    """t_test past the trajectory, pred_channels below C (the mask's business: the window is unchanged), downsample
    (2, 1, 3) at res 8, a target coarser than the data"""
    from dpot_amd.data import eval_window, resize_pad_window3
    fx = load("g19_data3d")
    for k in range(4):
        H, W, L, T, Cc, res, nc, t_in, t_test, d0, d1, d2, pc = (int(v) for v in fx[f"t{k}.meta"])
        raw = guard.wrap(D3.recipe_sample3((H, W, L, T, Cc), salt=200 + k), "cuda")
        t0, t_ar = eval_window(T, t_in, t_test)
        xx, yy = resize_pad_window3([raw], [t0], res, t_in, t_ar, nc, downsample=(d0, d1, d2))
        assert_close(xx[0], fx[f"t{k}.x"], f"test case {k} x", **TOL)
        assert_close(yy[0], fx[f"t{k}.y"], f"test case {k} y", **TOL)


def test_one_launch_mixed_batch(guarded):
    """six samples of four shapes and different t0 in ONE launch at res 40, t_in + t_ar = 3, n_channels 4 (one sample with
    C = 4).  40^3 voxels are 1000 tiles of 64; six samples get 2048 // 6 = 341 workgroups each, so every workgroup's tile
    loop takes two or three trips and the last trip is a partial one (1000 = 2 * 341 + 318).  A last tile of fewer than 64
    voxels: the res 6 and the down-sampled golden cases (216 and 96 voxels)"""
    from dpot_amd.data import resize_pad_window3
    res, t_in, t_ar, nc = 40, 2, 1, 4
    shapes = [(10, 12, 9, 5, 3), (40, 40, 40, 3, 4), (7, 7, 7, 6, 1), (50, 16, 24, 4, 2)]
    pick, starts = [0, 1, 2, 3, 0, 2], [0, 0, 3, 1, 2, 1]
    raws = [D3.recipe_sample3(shapes[p], salt=30 + i) for i, p in enumerate(pick)]
    xx, yy = resize_pad_window3([guard.wrap(r, "cuda") for r in raws], starts, res, t_in, t_ar, nc)
    assert tuple(xx.shape) == (6, res, res, res, t_in, nc) and tuple(yy.shape) == (6, res, res, res, t_ar, nc)
    for i, r in enumerate(raws):
        xr, yr = _ref(r, res, nc, starts[i], t_in, t_ar)
        assert_close(xx[i], xr, f"sample {i} x", **TOL)
        assert_close(yy[i], yr, f"sample {i} y", **TOL)


def test_t_ar_zero_and_window_past_the_trajectory(guarded):
    from dpot_amd.data import resize_pad_window3
    raw = D3.recipe_sample3((5, 6, 4, 6, 2), salt=41)
    dev = guard.wrap(raw, "cuda")
    xx, yy = resize_pad_window3([dev], [2], 6, 4, 0, 5)
    assert yy is None
    assert_close(xx[0], _ref(raw, 6, 5, 2, 4, 0)[0], "t_ar = 0 x", **TOL)
    with pytest.raises(ValueError, match="window"):
        resize_pad_window3([dev], [3], 6, 4, 0, 5)                       # frames 3 .. 6 of 6
    with pytest.raises(ValueError, match="window"):
        resize_pad_window3([dev], [0], 6, 4, 3, 5)


def test_rejects_wrong_output_buffers_and_fills_a_correct_one(guarded):
    from dpot_amd import _lib
    from dpot_amd.data import resize_pad_window3
    raw = [guard.wrap(D3.recipe_sample3((5, 6, 4, 6, 2), salt=42), "cuda")]
    args = (raw, [0], 8, 3, 2, 5)
    down = (2, 1, 3)                                                      # outputs [1, 4, 8, 3, t, 5]
    ok_x = guard.full_nan((1, 4, 8, 3, 3, 5))
    with pytest.raises(_lib.DpotHipError, match="out_xx"):                # the un-sub-sampled shape
        resize_pad_window3(*args, out_xx=torch.empty(1, 8, 8, 8, 3, 5, device="cuda"), downsample=down)
    with pytest.raises(_lib.DpotHipError, match="out_yy"):                # t_in frames where t_ar belong
        resize_pad_window3(*args, out_xx=ok_x, out_yy=torch.empty(1, 4, 8, 3, 3, 5, device="cuda"), downsample=down)
    with pytest.raises(_lib.DpotHipError, match="out_xx"):                # not contiguous
        resize_pad_window3(*args, out_xx=torch.empty(1, 4, 8, 3, 3, 10, device="cuda")[..., ::2], downsample=down)
    with pytest.raises(_lib.DpotHipError, match="out_yy"):                # wrong device
        resize_pad_window3(*args, out_xx=ok_x, out_yy=torch.empty(1, 4, 8, 3, 2, 5), downsample=down)
    with pytest.raises(_lib.DpotHipError, match="out_xx"):                # wrong dtype
        resize_pad_window3(*args, out_xx=torch.empty(1, 4, 8, 3, 3, 5, device="cuda", dtype=torch.float64), downsample=down)
    assert bool(torch.isnan(ok_x).all())                                  # no rejected call has touched it
    xx, yy = resize_pad_window3(*args, out_xx=ok_x, downsample=down)
    assert xx is ok_x and tuple(yy.shape) == (1, 4, 8, 3, 2, 5)
    assert torch.isfinite(xx).all() and torch.isfinite(yy).all()          # both were NaN before the launch: fully written


def test_device_batcher3d_double_buffer_is_exact():
    from dpot_amd.data import DeviceBatcher3D, staged_floats
    B, res, t_in, t_ar, nc = 4, 8, 3, 2, 3
    shapes = [(6, 5, 7, 9, 1), (8, 8, 8, 7, 3), (5, 6, 4, 8, 2), (6, 5, 7, 9)]          # the last one: a [H,W,L,T] dataset
    db = DeviceBatcher3D(B, res, t_in, t_ar, nc, max_raw_floats_per_sample=8 * 8 * 8 * (t_in + t_ar) * 3)
    rng = np.random.default_rng(1)
    batches = []
    for it in range(5):                                   # more batches than slots: slots are recycled
        raws = [D3.recipe_sample3(s if len(s) == 5 else s + (1,), salt=20 * it + i) for i, s in enumerate(shapes)]
        raws = [r if len(s) == 5 else r[..., 0] for r, s in zip(raws, shapes)]
        starts = [int(rng.integers(0, 3)) for _ in shapes]
        batches.append((raws, starts, [it, 7, 2 * it, 1]))
    db.submit(*batches[0])
    for it in range(5):
        if it + 1 < 5:
            db.submit(*batches[it + 1])                                   # next batch in flight while this one is read
        xx, yy, msk = db.get()
        got_x, got_y, cls = xx.clone(), yy.clone(), db.last_cls.clone()   # "the step": reads the slot on this stream
        assert db.last_slot == it % 2
        db.release()
        raws, starts, ids = batches[it]
        for i, r in enumerate(raws):
            xr, yr = _ref(r if r.dim() == 5 else r.unsqueeze(-1), res, nc, starts[i], t_in, t_ar)
            assert_close(got_x[i], xr, f"batch {it} sample {i} x", **TOL)
            assert_close(got_y[i], yr, f"batch {it} sample {i} y", **TOL)
        assert cls.dtype == torch.int64 and cls.cpu().tolist() == [[d] for d in ids]
        assert tuple(msk.shape) == (B, res, res, res, 1, nc) and bool((msk == 1).all())
    # only the window's frames cross the bus
    assert db.h2d_bytes == 5 * 4 * sum(staged_floats(s, t_in, t_ar) for s in shapes)
    assert db.h2d_bytes < sum(int(np.prod(r.shape)) * 4 for raws, _, _ in batches for r in raws)
    with pytest.raises(ValueError, match="window"):
        db.submit(batches[0][0], [0, 3, 0, 0])                            # frames 3 .. 7 of sample 1's 7
    with pytest.raises(ValueError, match="max_raw_floats_per_sample"):
        db.submit([np.zeros((9, 9, 9, 5, 3), np.float32)] * 4, [0] * 4)
    assert db.pending == [] and db.k == 5                                 # a rejected batch changes nothing


def test_device_batcher3d_test_mode_with_downsampling_golden():
    from dpot_amd.data import DeviceBatcher3D, eval_window, staged_floats
    fx = load("g19_data3d")
    for k in (0, 2):                                      # t_test past the trajectory; downsample (2, 1, 3)
        H, W, L, T, Cc, res, nc, t_in, t_test, d0, d1, d2, pc = (int(v) for v in fx[f"t{k}.meta"])
        raw = D3.recipe_sample3((H, W, L, T, Cc), salt=200 + k)
        t0, t_ar = eval_window(T, t_in, t_test)
        db = DeviceBatcher3D(2, res, t_in, t_ar, nc, max_raw_floats_per_sample=staged_floats(raw.shape, t_in, t_ar),
                             downsample=(d0, d1, d2))
        db.submit([raw.numpy(), raw], [t0, t0], dataset_ids=[3, 5])       # a numpy array and a CPU tensor
        bx, by, msk = db.get()
        gx, gy, cls = bx.clone(), by.clone(), db.last_cls.clone()
        db.release()
        torch.cuda.synchronize()
        assert cls.cpu().tolist() == [[3], [5]]
        assert tuple(msk.shape) == (2, res, res, res, 1, nc)              # the mask is not sub-sampled
        assert_close(gx[1], fx[f"t{k}.x"], f"batcher test case {k} x", **TOL)
        assert_close(gy[0], fx[f"t{k}.y"], f"batcher test case {k} y", **TOL)


def test_batch_through_a_training_step():
    """a DeviceBatcher3D batch at res 16 through train.train_step of a tiny DPOTNet3D against a hand-built batch of the
    restatement through the same step of an identically initialised model"""
    from dpot_amd import DPOTNet3D
    from dpot_amd.data import DeviceBatcher3D, staged_floats
    from dpot_amd.train import FlatParams, FusedAdam, train_step
    B, res, t_in, t_ar, nc = 2, 16, 3, 2, 3
    shapes, starts = [(10, 12, 9, 7, 2), (16, 16, 16, 5, 3)], [1, 0]
    raws = [D3.recipe_sample3(s, salt=60 + i) for i, s in enumerate(shapes)]
    db = DeviceBatcher3D(B, res, t_in, t_ar, nc, max_raw_floats_per_sample=max(staged_floats(s, t_in, t_ar) for s in shapes))
    db.submit(raws, starts)
    ref = [_ref(r, res, nc, t0, t_in, t_ar) for r, t0 in zip(raws, starts)]
    hand = (torch.stack([x for x, _ in ref]).cuda(), torch.stack([y for _, y in ref]).cuda(),
            torch.ones(B, res, res, res, 1, nc, device="cuda"))
    losses = []
    for batch in (None, hand):
        torch.manual_seed(0)
        m = DPOTNet3D(img_size=res, patch_size=4, in_channels=nc, out_channels=nc, in_timesteps=t_in, out_timesteps=1,
                      embed_dim=32, depth=1, n_blocks=4, mlp_ratio=2, out_layer_dim=16, modes=3).cuda()
        opt = FusedAdam(FlatParams(m), lr=1e-3)
        xx, yy, msk = db.get() if batch is None else batch
        loss, pred = train_step(m, opt, xx, yy, msk, lr=1e-3)
        if batch is None:
            db.release()
            assert_close(xx, hand[0], "batcher x", **TOL)
            assert_close(yy, hand[1], "batcher y", **TOL)
        assert torch.isfinite(pred).all()
        losses.append(loss.item())
    print(f"loss through the batcher {losses[0]:.9g}, hand-built {losses[1]:.9g}")
    assert np.isfinite(losses).all() and losses[1] > 0
    assert abs(losses[0] - losses[1]) <= RTOL * abs(losses[1])
