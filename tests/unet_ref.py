"""float64 restatement of the UNet baseline's operators and of the model, written from the formulas (no torch.nn.functional
convolution, normalisation or pooling; torch is the array library): 3x3 convolution as explicit tap sums, batch statistics,
normalise + activation, 2x2 max pooling with torch's tie rule (the FIRST maximum of a window in (row, column) order), the
k = s = 2 transposed convolution, the whole forward and the hand-derived backward.  tests/test_cpu_unet.py holds it to the
float64 records of tests/golden/g24_unet.npz at 1e-12; the GPU tests compare the kernels with it at every other shape.
Fields are channels-last [B, H, W, C]."""
import math
from collections import OrderedDict

import torch

from oracle import dpot_ref as R

F64 = torch.float64
EPS, MOMENTUM = 1e-5, 0.1
ACT_IDS = {"gelu": 1, "tanh": 2, "sigmoid": 3, "relu": 4, "leaky_relu": 5, "softplus": 6, "ELU": 7, "silu": 8}

# (B, H, W, Cin, Cout): what each is there for is said in tests/test_gpu_unet_ops.py
OP_SHAPES = [(1, 1, 1, 1, 1), (2, 1, 1, 5, 3), (1, 2, 3, 3, 2), (2, 5, 7, 6, 10), (3, 6, 6, 4, 8), (1, 16, 16, 8, 2),
             (1, 33, 17, 4, 36), (1, 8, 8, 128, 16), (2, 4, 4, 32, 64)]


# the fixture model (tests/golden/g24_unet.npz, scripts/make_golden_unet.py): width 2, 30 844 parameters
CFG = dict(in_channels=2, out_channels=2, in_timesteps=3, out_timesteps=1, width=2, act="gelu", n_cls=3)
WINDOWS = OrderedDict(a=(4, (32, 32)), b=(2, (20, 24)))          # tag -> (batch, in_shape)
STEP = dict(lr=1e-3, betas=(0.9, 0.9), weight_decay=1e-6, max_norm=5.0)
BIG, STRIDE = 2048, 3          # a recorded tensor of more than BIG elements is kept as every STRIDE-th element


def hash_input(shape, salt):
    return R.recipe_input(tuple(shape), salt)


def window_inputs(tag):
    """(x [B, X, Y, T, C], y [B, X, Y, 1, C_out]) of a fixture window"""
    B, (X, Y) = WINDOWS[tag]
    salt = 900 + 10 * list(WINDOWS).index(tag)
    return (hash_input((B, X, Y, CFG["in_timesteps"], CFG["in_channels"]), salt),
            hash_input((B, X, Y, CFG["out_timesteps"], CFG["out_channels"]), salt + 1))


def sub(t):
    """what the fixture records of a tensor"""
    return t.reshape(-1)[::STRIDE].clone() if t.numel() > BIG else t


def pack(tensors):
    """the recorded forms of `tensors`, flattened one after the other"""
    return torch.cat([sub(t).reshape(-1) for t in tensors])


def unpack(flat, shapes, subsample=True):
    """the pieces of a packed record, by the tensors' shapes: each flat, subsampled as `sub` does"""
    out, at = [], 0
    for shape in shapes:
        n = math.prod(shape)
        if subsample and n > BIG:
            n = (n + STRIDE - 1) // STRIDE
        out.append(flat[at:at + n])
        at += n
    assert at == len(flat), (at, len(flat))
    return out


def nerr(a, b):
    import numpy as np
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300))


def ints(shape, salt, lo=-3, hi=3):
    """float32 integers in [lo, hi] from the hash recipe"""
    u = hash_input(shape, salt).double() / 3.0 + 0.5
    return (torch.floor((hi - lo + 1) * u).clamp(0, hi - lo) + lo).float()


# ---- activations -------------------------------------------------------------------------------------------------------------
def act(name, x):
    if name == "gelu":
        return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))
    if name == "relu":
        return torch.where(x < 0, torch.zeros_like(x), x)
    if name == "leaky_relu":
        return torch.where(x > 0, x, 0.1 * x)
    if name == "tanh":
        return torch.tanh(x)
    if name == "sigmoid":
        return 1 / (1 + torch.exp(-x))
    if name == "silu":
        return x / (1 + torch.exp(-x))
    raise KeyError(name)


def dact(name, x):
    if name == "gelu":
        return 0.5 * (1 + torch.erf(x / math.sqrt(2))) + x * torch.exp(-0.5 * x * x) / math.sqrt(2 * math.pi)
    if name == "relu":
        return (x > 0).to(x.dtype)
    if name == "leaky_relu":
        return torch.where(x > 0, torch.ones_like(x), torch.full_like(x, 0.1))
    if name == "tanh":
        return 1 - torch.tanh(x) ** 2
    if name == "sigmoid":
        s = 1 / (1 + torch.exp(-x))
        return s * (1 - s)
    if name == "silu":
        s = 1 / (1 + torch.exp(-x))
        return s * (1 + x * (1 - s))
    raise KeyError(name)


# ---- convolution -------------------------------------------------------------------------------------------------------------
def _padded(x):
    B, H, W, C = x.shape
    xp = x.new_zeros(B, H + 2, W + 2, C)
    xp[:, 1:H + 1, 1:W + 1] = x
    return xp


def conv3x3(x, w):
    """out[b, h, w, co] = sum over (dy, dx) and ci of x[b, h + dy - 1, w + dx - 1, ci] w[co, ci, dy, dx], zero outside"""
    B, H, W, _ = x.shape
    xp = _padded(x)
    out = x.new_zeros(B, H, W, w.shape[0])
    for dy in range(3):
        for dx in range(3):
            out += xp[:, dy:dy + H, dx:dx + W] @ w[:, :, dy, dx].T
    return out


def conv3x3_bwd_data(dz, w):
    """dx[b, h, w, ci] = sum over (dy, dx) and co of dz[b, h - dy + 1, w - dx + 1, co] w[co, ci, dy, dx]"""
    B, H, W, _ = dz.shape
    gp = _padded(dz)
    out = dz.new_zeros(B, H, W, w.shape[1])
    for dy in range(3):
        for dx in range(3):
            out += gp[:, 2 - dy:2 - dy + H, 2 - dx:2 - dx + W] @ w[:, :, dy, dx]
    return out


def conv3x3_wgrad(x, dz):
    """dw[co, ci, dy, dx] = sum over the pixels of dz[p, co] x[p + (dy - 1, dx - 1), ci]"""
    B, H, W, Cin = x.shape
    xp = _padded(x)
    dw = x.new_zeros(dz.shape[-1], Cin, 3, 3)
    for dy in range(3):
        for dx in range(3):
            dw[:, :, dy, dx] = dz.reshape(-1, dz.shape[-1]).T @ xp[:, dy:dy + H, dx:dx + W].reshape(-1, Cin)
    return dw


# ---- BatchNorm ---------------------------------------------------------------------------------------------------------------
def bn_stats(z, eps=EPS):
    """(mean, biased variance, invstd) per channel over every pixel of the batch"""
    f = z.reshape(-1, z.shape[-1])
    mean = f.mean(0)
    var = ((f - mean) ** 2).mean(0)
    return mean, var, 1 / torch.sqrt(var + eps)


def bn_running(z, rm, rv, nbt, momentum=MOMENTUM):
    """the buffers after one training-mode call: momentum, the UNBIASED variance, the counter + 1"""
    mean, var, _ = bn_stats(z)
    n = z.numel() // z.shape[-1]
    return (1 - momentum) * rm + momentum * mean, (1 - momentum) * rv + momentum * var * n / (n - 1), nbt + 1


def pool_first_max(y):
    """(the 2x2 / stride-2 maximum [B, H/2, W/2, C], the index 2 r + c of the FIRST maximum of each window)"""
    B, H, W, C = y.shape
    win = y.reshape(B, H // 2, 2, W // 2, 2, C).permute(0, 1, 3, 5, 2, 4).reshape(B, H // 2, W // 2, C, 4)
    best, arg = win[..., 0].clone(), torch.zeros(win.shape[:-1], dtype=torch.int64)
    for q in range(1, 4):
        take = win[..., q] > best                              # a tie keeps the earlier one
        best, arg = torch.where(take, win[..., q], best), torch.where(take, torch.full_like(arg, q), arg)
    return best, arg


def unpool(dpool, arg, shape):
    """the pooled field's gradient routed to the recorded position of each window"""
    B, H, W, C = shape
    hot = torch.zeros(B, H // 2, W // 2, C, 4, dtype=dpool.dtype)
    hot.scatter_(-1, arg.unsqueeze(-1), dpool.unsqueeze(-1))
    return hot.reshape(B, H // 2, W // 2, C, 2, 2).permute(0, 1, 4, 2, 5, 3).reshape(B, H, W, C)


def bn_act(z, mean, invstd, gamma, beta, name, pool=False):
    y = act(name, gamma * ((z - mean) * invstd) + beta)
    return (y, pool_first_max(y)[0]) if pool else y


def bn_act_bwd(dy, dpool, z, mean, invstd, gamma, beta, name):
    """-> (dz, dgamma, dbeta) of training-mode BatchNorm + act (+ pooling): g = (dy + routed dpool) act'(pre),
    dz = gamma invstd (g - mean(g) - xhat mean(g xhat))"""
    xhat = (z - mean) * invstd
    pre = gamma * xhat + beta
    up = torch.zeros_like(z) if dy is None else dy.clone()
    if dpool is not None:
        up = up + unpool(dpool, pool_first_max(act(name, pre))[1], z.shape)
    g = up * dact(name, pre)
    gf, xf = g.reshape(-1, g.shape[-1]), xhat.reshape(-1, g.shape[-1])
    dbeta, dgamma = gf.sum(0), (gf * xf).sum(0)
    n = gf.shape[0]
    return gamma * invstd * (g - dbeta / n - xhat * (dgamma / n)), dgamma, dbeta


# ---- transposed convolution k = s = 2 ------------------------------------------------------------------------------------------
def upconv2(x, w, b):
    """out[b, 2 h + i, 2 w + j, co] = sum_ci x[b, h, w, ci] w[ci, co, i, j] + b[co]"""
    B, h, wd, Cin = x.shape
    Co = w.shape[1]
    z = (x.reshape(-1, Cin) @ w.reshape(Cin, Co * 4)).reshape(B, h, wd, Co, 2, 2)
    return z.permute(0, 1, 4, 2, 5, 3).reshape(B, 2 * h, 2 * wd, Co) + b


def upconv2_bwd(dy, x, w):
    B, h, wd, Cin = x.shape
    Co = w.shape[1]
    dz = dy.reshape(B, h, 2, wd, 2, Co).permute(0, 1, 3, 5, 2, 4).reshape(-1, Co * 4)
    dx = (dz @ w.reshape(Cin, Co * 4).T).reshape(x.shape)
    dw = (x.reshape(-1, Cin).T @ dz).reshape(w.shape)
    return dx, dw, dy.reshape(-1, Co).sum(0)


# ---- the loss: utils/criterion.py SimpleLpLoss(size_average=False), p = 2, no mask -------------------------------------------------
def rel_l2(pred, y):
    """sum over the samples of the mean over the channels of ||pred - y||_2 / (||y||_2 + 1e-8) taken over (X, Y, T);
    -> (loss, dpred)"""
    B, C = pred.shape[0], pred.shape[-1]
    d = (pred - y).reshape(B, -1, C)
    dn, yn = torch.sqrt((d ** 2).sum(1)), torch.sqrt((y.reshape(B, -1, C) ** 2).sum(1)) + 1e-8
    loss = (dn / yn).mean(1).sum()
    return loss, (d / (dn * yn * C).unsqueeze(1)).reshape(pred.shape)


# ---- the model -------------------------------------------------------------------------------------------------------------------
BLOCKS = ("encoder1", "encoder2", "encoder3", "encoder4", "bottleneck", "decoder4", "decoder3", "decoder2", "decoder1")
SHORT = {"encoder1": "enc1", "encoder2": "enc2", "encoder3": "enc3", "encoder4": "enc4", "bottleneck": "bottleneck",
         "decoder4": "dec4", "decoder3": "dec3", "decoder2": "dec2", "decoder1": "dec1"}


def assemble(x, in_shape):
    """[B, X, Y, T, C] -> the padded network input [B, Xp, Yp, 2 + T C]: grid first (float32 linspace, as the reference), zeros
    at the high end of both axes up to the next multiple of 16 of in_shape"""
    B, X, Y, T, C = x.shape
    pad = [int(math.ceil(s / 16) * 16 - s) for s in in_shape]
    gx = torch.linspace(0, 1, X, dtype=torch.float32).to(x.dtype).view(1, X, 1, 1).expand(B, X, Y, 1)
    gy = torch.linspace(0, 1, Y, dtype=torch.float32).to(x.dtype).view(1, 1, Y, 1).expand(B, X, Y, 1)
    f = torch.cat([gx, gy, x.reshape(B, X, Y, T * C)], dim=-1)
    out = f.new_zeros(B, X + pad[0], Y + pad[1], f.shape[-1])
    out[:, :X, :Y] = f
    return out


class Model:
    """the UNet forward in `dtype` from a reference state dict, keeping what the backward needs; train=True normalises with the
    batch statistics and records the buffers a step leaves (self.buffers), train=False uses the running ones"""

    def __init__(self, sd, in_shape, out_timesteps, out_channels, name="gelu", dtype=F64):
        self.sd = OrderedDict((k, torch.as_tensor(v).to(dtype) if torch.as_tensor(v).is_floating_point() else torch.as_tensor(v))
                              for k, v in sd.items())
        self.in_shape, self.To, self.Co, self.name = tuple(in_shape), out_timesteps, out_channels, name

    def _layer(self, x, blk, i, train, pool=False):
        p = f"{blk}.{SHORT[blk]}"
        w, gamma, beta = self.sd[f"{p}conv{i}.weight"], self.sd[f"{p}norm{i}.weight"], self.sd[f"{p}norm{i}.bias"]
        z = conv3x3(x, w)
        rm, rv, nbt = (self.sd[f"{p}norm{i}.{k}"] for k in ("running_mean", "running_var", "num_batches_tracked"))
        if train:
            mean, _, invstd = bn_stats(z)
            for k, v in zip(("running_mean", "running_var", "num_batches_tracked"), bn_running(z, rm, rv, nbt)):
                self.buffers[f"{p}norm{i}.{k}"] = v
        else:
            mean, invstd = rm, 1 / torch.sqrt(rv + EPS)
        self.tape.append((f"{p}conv{i}", f"{p}norm{i}", x, z, mean, invstd, pool))
        return bn_act(z, mean, invstd, gamma, beta, self.name, pool)

    def _block(self, x, blk, train, pool=False):
        return self._layer(self._layer(x, blk, 1, train), blk, 2, train, pool)

    def forward(self, x, train=True):
        self.tape, self.buffers, self.ups = [], OrderedDict(), []
        B, X, Y, T, C = x.shape
        self.x_shape = x.shape
        h = assemble(x.to(next(iter(self.sd.values())).dtype), self.in_shape)
        skips = []
        for blk in BLOCKS[:4]:
            y, h = self._block(h, blk, train, pool=True)
            skips.append(y)
        h = self._block(h, "bottleneck", train)
        for k, blk in zip((4, 3, 2, 1), BLOCKS[5:]):
            w, b = self.sd[f"upconv{k}.weight"], self.sd[f"upconv{k}.bias"]
            self.ups.append((f"upconv{k}", h, len(self.tape)))
            h = self._block(torch.cat([upconv2(h, w, b), skips[k - 1]], dim=-1), blk, train)
        self.last = h
        rows = h[:, :X, :Y].reshape(-1, h.shape[-1])
        cw = self.sd["conv.weight"].reshape(self.To * self.Co, -1)
        return (rows @ cw.T + self.sd["conv.bias"]).reshape(B, X, Y, self.To, self.Co)

    def backward(self, dpred):
        """the gradient of every parameter, by name, from the gradient of the prediction of the last train-mode forward"""
        g = OrderedDict()
        B, X, Y, T, C = self.x_shape
        d2 = dpred.reshape(B * X * Y, -1)
        cw = self.sd["conv.weight"]
        g["conv.weight"] = (d2.T @ self.last[:, :X, :Y].reshape(B * X * Y, -1)).reshape(cw.shape)
        g["conv.bias"] = d2.sum(0)
        dh = torch.zeros_like(self.last)
        dh[:, :X, :Y] = (d2 @ cw.reshape(cw.shape[0], -1)).reshape(B, X, Y, -1)
        ups = {at: (name, xin) for name, xin, at in self.ups}
        skip_grads = {}                      # tape index of an encoder's last layer -> the gradient of its y through the skip
        pool_grad = None                     # gradient of the pooled field of the layer about to be visited
        enc_last = [2 * k + 1 for k in range(4)]
        for idx in reversed(range(len(self.tape))):
            conv, norm, x, z, mean, invstd, pool = self.tape[idx]
            dy, dpool = dh, None
            if pool:
                dy, dpool = skip_grads[idx], pool_grad
            dz, g[norm + ".weight"], g[norm + ".bias"] = bn_act_bwd(dy, dpool, z, mean, invstd, self.sd[norm + ".weight"],
                                                                    self.sd[norm + ".bias"], self.name)
            g[conv + ".weight"] = conv3x3_wgrad(x, dz)
            dx = conv3x3_bwd_data(dz, self.sd[conv + ".weight"])
            if idx in ups:                   # x was cat(upconv(h), skip): split, send the skip's half to its encoder
                name, xin = ups[idx]
                Cu = self.sd[name + ".weight"].shape[1]
                level = int(name[-1])
                skip_grads[enc_last[level - 1]] = dx[..., Cu:]
                dh, g[name + ".weight"], g[name + ".bias"] = upconv2_bwd(dx[..., :Cu], xin, self.sd[name + ".weight"])
            elif idx >= 2 and idx % 2 == 0 and idx <= 8:      # the first layer of encoder2..4 / the bottleneck: x was a pooled field
                pool_grad, dh = dx, None
            else:
                dh = dx
        return g


# ---- the fixture's records ---------------------------------------------------------------------------------------------------
def fixture_layout(fx):
    """[(name, shape, torch dtype)] of the recorded state dict"""
    names = [str(n) for n in fx["sd.names"]]
    shapes = [tuple(int(s) for s in row if s) for row in fx["sd.shapes"]]
    dtypes = [getattr(torch, str(d).split(".")[-1]) for d in fx["sd.dtypes"]]
    return list(zip(names, shapes, dtypes))


def fixture_sd(fx):
    layout = fixture_layout(fx)
    pieces = unpack(torch.from_numpy(fx["sd.flat"]), [s for _, s, _ in layout], subsample=False)
    return OrderedDict((n, p.reshape(s).to(d).clone()) for (n, s, d), p in zip(layout, pieces))


def is_buffer(name):
    return name.rsplit(".", 1)[-1] in ("running_mean", "running_var", "num_batches_tracked")


def param_layout(fx):
    return [(n, s) for n, s, _ in fixture_layout(fx) if not is_buffer(n)]


def buffer_layout(fx):
    return [(n, s) for n, s, _ in fixture_layout(fx) if is_buffer(n)]
