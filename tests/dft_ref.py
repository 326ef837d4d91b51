"""References of the 2-D DFT kernel tests, written from the definition with torch.fft on the host.

The kernels (include/dpot_hip.h) transform x[B, h, w, E] over (h, w) with norm="ortho", keep the modes kx < mx, ky < my of the
half spectrum and weight its columns: weight 2 on the interior columns 0 < ky, ky != w / 2 for even w, where col_weights asks for
it.  Forward, col_weights = 1 multiplies the spectrum by the weights; inverse, col_weights = 1 IS irfft2 of the zero-padded
spectrum (a one-sided spectrum counts its interior columns twice) and col_weights = 0 is irfft2 of the spectrum with those
columns halved.  Every function takes the dtype to compute in: float64 is the reference, float32 the yardstick the kernels'
norm-wise error is held against.
"""
import torch

CPLX = {torch.float64: torch.complex128, torch.float32: torch.complex64}


def interior_columns(w, my):
    """bool [my]: the columns of the half spectrum that stand for two columns of the full one"""
    ky = torch.arange(my)
    interior = ky > 0
    if w % 2 == 0:
        interior &= ky != w // 2
    return interior


def rfft2_ref(x, mx, my, dtype=torch.float64):
    """x [B,h,w,E] -> the kept modes of rfft2, complex [B,mx,my,E] (col_weights = 0)"""
    return torch.fft.rfft2(x.to(dtype), dim=(1, 2), norm="ortho")[:, :mx, :my]


def weighted(spec, w):
    """col_weights = 1 of the forward transform: the interior columns of spec [B,mx,my,E] doubled (exact in any dtype)"""
    out = spec.clone()
    out[:, :, interior_columns(w, spec.shape[2])] *= 2
    return out


def irfft2_ref(spec, h, w, col_weights, dtype=torch.float64):
    """spec complex [B,mx,my,E] (any values: no Hermitian symmetry asked) -> [B,h,w,E]"""
    B, mx, my, E = spec.shape
    full = torch.zeros(B, h, w // 2 + 1, E, dtype=CPLX[dtype])
    full[:, :mx, :my] = spec.to(CPLX[dtype])
    if not col_weights:
        full[:, :, :my][:, :, interior_columns(w, my)] *= 0.5
    return torch.fft.irfft2(full, s=(h, w), dim=(1, 2), norm="ortho")


def to_planar(spec, nb):
    """complex [B,mx,my,E] -> the kernels' rows [B*mx*my, 2E] fp32: per channel block [re(bs) | im(bs)]"""
    B, mx, my, E = spec.shape
    bs = E // nb
    planes = torch.stack([spec.real.reshape(B, mx, my, nb, bs), spec.imag.reshape(B, mx, my, nb, bs)], dim=-2)
    return planes.reshape(B * mx * my, 2 * E).float().contiguous()


def from_planar(rows, B, mx, my, nb):
    """the kernels' rows [B*mx*my, 2E] -> complex128 [B,mx,my,E]"""
    E = rows.shape[1] // 2
    p = rows.detach().cpu().double().view(B, mx, my, nb, 2, E // nb)
    return torch.complex(p[..., 0, :].reshape(B, mx, my, E), p[..., 1, :].reshape(B, mx, my, E))


def rel_err(got, ref):
    """|| got - ref || / || ref || over the whole tensor, in float64 (complex or real)"""
    ref = ref.to(torch.complex128 if ref.is_complex() else torch.float64)
    got = got.detach().cpu().to(ref.dtype)
    return (torch.linalg.vector_norm(got - ref) / torch.linalg.vector_norm(ref)).item()
