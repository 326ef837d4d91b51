"""CPU tests of the UNet baseline: the model's layout and refusals against the reference's recorded layout
(tests/golden/g24_unet.npz), and the float64 restatement (tests/unet_ref.py) against the reference's float64 records."""
import inspect

import pytest
import torch

import unet_ref as UR
from helpers import load


def _model(in_shape=(32, 32), **kw):
    from dpot_amd import UNet
    return UNet(2, **dict(UR.CFG, in_shape=in_shape, **kw))


def test_state_dict_layout_and_strict_load():
    fx = load("g24_unet")
    m = _model()
    sd = m.state_dict()
    assert len(sd) == 118
    assert [(k, tuple(v.shape), v.dtype) for k, v in sd.items()] == UR.fixture_layout(fx)
    assert sum(p.numel() for p in m.parameters()) == 30844
    ref = UR.fixture_sd(fx)
    m.load_state_dict(ref, strict=True)
    for k, v in m.state_dict().items():
        assert torch.equal(v, ref[k]), k
    assert m.encoder1.enc1conv1.weight.shape == (2, 8, 3, 3) and m.upconv4.weight.shape == (32, 16, 2, 2)
    assert m.encoder1.enc1norm1.num_batches_tracked.dtype == torch.int64


def test_constructor_signature_is_the_references():
    from dpot_amd import UNet
    fx = load("g24_unet")
    sig = inspect.signature(UNet.__init__)
    assert [f"{k}={v.default!r}" for k, v in sig.parameters.items() if k != "self"] == [str(s) for s in fx["signature"]]


def test_refusals():
    from dpot_amd import UNet, ops
    from dpot_amd.train import rollout_total
    for n_dim in (1, 3):
        with pytest.raises(ValueError, match="n_dim"):
            UNet(n_dim, in_shape=(32,) * n_dim)
    with pytest.raises(ValueError, match="out_shape"):
        UNet(2, in_shape=(32, 32), out_shape=(16, 16))
    UNet(2, in_shape=(32, 32), out_shape=(32, 32), width=2)                      # the same shape is no Interpolate branch
    max_w, max_c = ops.unet_limits()
    with pytest.raises(ValueError, match=str(max_w + 16)):
        UNet(2, in_shape=(16, max_w + 16), width=2)
    with pytest.raises(ValueError, match=str(max_c + 1)):
        ops.unet_check_sizes(16, (4, max_c + 1))
    m = _model()
    x = torch.zeros(1, 20, 24, UR.CFG["in_timesteps"], UR.CFG["in_channels"])
    with pytest.raises(ValueError, match="20x24"):
        m(x)                                                                     # in_shape (32, 32) pads nothing
    xx = torch.zeros(2, 32, 32, UR.CFG["in_timesteps"], UR.CFG["in_channels"])
    yy = torch.zeros(2, 32, 32, 1, UR.CFG["out_channels"])
    with pytest.raises(ValueError, match="cls_weight"):
        rollout_total(m, xx, yy, None, cls=torch.zeros(2, dtype=torch.int64), cls_weight=0.5)
    assert m.cls_output and not m.cls_trainable


@pytest.mark.parametrize("tag", list(UR.WINDOWS))
def test_restatement_equals_the_references_float64_records(tag):
    fx = load("g24_unet")
    B, in_shape = UR.WINDOWS[tag]
    x, y = UR.window_inputs(tag)
    ref = UR.Model(UR.fixture_sd(fx), in_shape, UR.CFG["out_timesteps"], UR.CFG["out_channels"], UR.CFG["act"])
    pred = ref.forward(x.double(), train=True)
    want = torch.from_numpy(fx[f"{tag}.pred64"])
    assert pred.shape == want.shape
    assert (pred - want).abs().max() <= 1e-12 * want.abs().max()
    _, dpred = UR.rel_l2(pred, y.double())
    g = ref.backward(dpred)
    layout = UR.param_layout(fx)
    pieces = UR.unpack(torch.from_numpy(fx[f"{tag}.g64"]), [s for _, s in layout])
    for (name, shape), rec in zip(layout, pieces):
        got = UR.sub(g[name]).reshape(-1)
        assert tuple(g[name].shape) == shape, name
        assert (got - rec).abs().max() <= 1e-12 * rec.abs().max(), (name, float((got - rec).abs().max()), float(rec.abs().max()))


def test_restatement_buffers_equal_the_references_first_step():
    """the running statistics one training-mode forward leaves (momentum 0.1, unbiased variance, counter) against the
    reference's float32 buffers after its first step"""
    fx = load("g24_unet")
    ref = UR.Model(UR.fixture_sd(fx), (32, 32), UR.CFG["out_timesteps"], UR.CFG["out_channels"], UR.CFG["act"])
    ref.forward(UR.window_inputs("a")[0].double(), train=True)
    layout = UR.buffer_layout(fx)
    pieces = UR.unpack(torch.from_numpy(fx["step.buf1"]), [s for _, s in layout])
    assert list(ref.buffers) == [n for n, _ in layout]
    for (name, shape), rec in zip(layout, pieces):
        got = ref.buffers[name].double().reshape(-1)
        assert (got - rec.double()).abs().max() <= 1e-5 * max(1.0, float(rec.abs().max())), name


def test_pooling_tie_rule_is_torchs():
    """a field with planted ties (ReLU's zeros): the restatement's maxima and where their gradient goes equal
    torch.nn.functional.max_pool2d and its autograd"""
    y = UR.ints((2, 6, 8, 3), 77, 0, 2).double()                                 # three values: most windows tie
    best, arg = UR.pool_first_max(y)
    yc = y.permute(0, 3, 1, 2).clone().requires_grad_(True)
    want = torch.nn.functional.max_pool2d(yc, 2, 2)
    assert torch.equal(best, want.detach().permute(0, 2, 3, 1))
    g = UR.hash_input(tuple(best.shape), 78).double()
    want.backward(g.permute(0, 3, 1, 2))
    assert torch.equal(UR.unpool(g, arg, y.shape), yc.grad.permute(0, 2, 3, 1))
    win = y.reshape(2, 3, 2, 4, 2, 3)
    assert int(((win == win.amax(dim=(2, 4), keepdim=True)).sum(dim=(2, 4)) > 1).sum()) > 20          # ties are there
