"""float64 restatement of the 3-D Fourier resize: the three-axis form of the reference's resize (utils/utilities.py:277-305),
written with numpy.fft as the reference writes the 2-D one with torch.fft.

    rfftn over (X, Y, Z), norm='backward'
    a zero spectrum [m_x, m_y, m_z//2 + 1]
    on each full-spectrum axis (X, Y) the reference's row rule: the first min((n+1)//2, (m+1)//2) and the last
        min(n//2, m//2) frequencies - four corner blocks; on the half-spectrum axis Z the first min(n_z//2 + 1, m_z//2 + 1)
    irfftn(s = out_size), times (m_x / n_x)(m_y / n_y)(m_z / n_z)

It shares no code with dpot_amd.ops; `resize3_torch32` is the same composition in float32 torch.fft, channels first, the
figure the kernel's error is set beside."""
import numpy as np


def _size3(out_size):
    return (out_size,) * 3 if isinstance(out_size, int) else tuple(int(s) for s in out_size)


def _blocks(n, m):
    """the (source slice, destination slice) pairs of one full-spectrum axis"""
    t, b = min((n + 1) // 2, (m + 1) // 2), min(n // 2, m // 2)
    out = [(slice(0, t), slice(0, t))]
    if b:
        out.append((slice(n - b, n), slice(m - b, m)))
    return out


def resize3_ref(x, out_size):
    """x [B, n_x, n_y, n_z, ...planes] (any float dtype) -> float64 [B, m_x, m_y, m_z, ...planes]"""
    x = np.asarray(x, dtype=np.float64)
    mx, my, mz = _size3(out_size)
    B, nx, ny, nz = x.shape[:4]
    spec = np.fft.rfftn(x, axes=(1, 2, 3), norm="backward")
    new = np.zeros((B, mx, my, mz // 2 + 1) + x.shape[4:], dtype=np.complex128)
    kz = min(nz // 2 + 1, mz // 2 + 1)
    for sx, dx in _blocks(nx, mx):
        for sy, dy in _blocks(ny, my):
            new[:, dx, dy, :kz] = spec[:, sx, sy, :kz]
    out = np.fft.irfftn(new, s=(mx, my, mz), axes=(1, 2, 3), norm="backward")
    return out * ((mx / nx) * (my / ny) * (mz / nz))


def resize3_torch(x, out_size):
    """the same composition with torch.fft in x's own dtype and on its own device: channels-first rfftn, the corner
    assignments, irfftn.  x [B, n_x, n_y, n_z, ...planes] torch tensor -> the same layout at the new size"""
    import torch
    mx, my, mz = _size3(out_size)
    B, nx, ny, nz = x.shape[:4]
    cf = x.reshape(B, nx, ny, nz, -1).permute(0, 4, 1, 2, 3)
    spec = torch.fft.rfftn(cf, dim=(2, 3, 4), norm="backward")
    new = torch.zeros((B, cf.shape[1], mx, my, mz // 2 + 1), dtype=spec.dtype, device=x.device)
    kz = min(nz // 2 + 1, mz // 2 + 1)
    for sx, dx in _blocks(nx, mx):
        for sy, dy in _blocks(ny, my):
            new[:, :, dx, dy, :kz] = spec[:, :, sx, sy, :kz]
    out = torch.fft.irfftn(new, s=(mx, my, mz), dim=(2, 3, 4), norm="backward") * ((mx / nx) * (my / ny) * (mz / nz))
    return out.permute(0, 2, 3, 4, 1).reshape((B, mx, my, mz) + tuple(x.shape[4:])).contiguous()
