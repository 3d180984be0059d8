"""Float64 oracle of the spatially varying blur of include/osmosis_psffield.h (torch on the CPU; the reference has no such operator).

The DEFINITION is per pixel: the output at p is the interpolated kernel sum_n hat_n(p) K_n applied at p over reflection padding
(`forward_pixelwise`).  Because the blur is linear in its kernel this equals sum_n hat_n (.) conv(pad(x), K_n) (`forward_sum`, the
form the kernel computes), and the transpose is sum_n A_n (hat_n (.) v) (`adjoint_gather`: the gather form of the header, pre-image by
pre-image; `adjoint_vjp`: autograd of `forward_sum`).  tests/test_psffield_cpu.py holds these against each other.

The hats come from the fp32 tables of `ops.gain_tables_host` read as float64 (a = 1 - fx, b = 1 - fy exact): the oracle sees the same
inputs as the kernel."""
import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24


def hats(H, W, gh, gw):
    """(haty float64 [gh,H], hatx float64 [gw,W]) from the fp32 tables."""
    from osmosis_diffusion_code_amd import ops
    iy0, fy, ix0, fx = ops.gain_tables_host(H, W, gh, gw)

    def axis(i0, f, g):
        h = np.zeros((g, len(i0)))
        pos = np.arange(len(i0))
        h[i0, pos] += 1.0 - f.astype(np.float64)
        h[i0 + 1, pos] += f.astype(np.float64)
        return torch.from_numpy(h)
    return axis(iy0, fy, gh), axis(ix0, fx, gw)


def hat_field(H, W, gh, gw):
    """hat_n(p), float64 [gh,gw,H,W]."""
    hy, hx = hats(H, W, gh, gw)
    return hy[:, None, :, None] * hx[None, :, None, :]


def conv_reflect(x, k):
    kh, kw = k.shape
    P = x.shape[1]
    return F.conv2d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), k.expand(P, 1, kh, kw).contiguous(), groups=P)


def forward_pixelwise(x, K):
    """The definition: x [B,P,H,W], K [gh,gw,kh,kw], float64."""
    B, P, H, W = x.shape
    gh, gw, kh, kw = K.shape
    hat = hat_field(H, W, gh, gw).reshape(gh * gw, H * W)
    Kp = K.reshape(gh * gw, kh * kw).t() @ hat                                          # the kernel of every pixel [kh kw, H W]
    patches = F.unfold(F.pad(x.reshape(B * P, 1, H, W), (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), (kh, kw))
    return (patches * Kp[None]).sum(dim=1).reshape(B, P, H, W)


def forward_sum(x, K):
    gh, gw = K.shape[:2]
    hat = hat_field(x.shape[2], x.shape[3], gh, gw)
    out = torch.zeros_like(x)
    for jy in range(gh):
        for jx in range(gw):
            out = out + hat[jy, jx] * conv_reflect(x, K[jy, jx])
    return out


def adjoint_vjp(v, K):
    x = torch.zeros_like(v).requires_grad_(True)
    g, = torch.autograd.grad(forward_sum(x, K), x, v)
    return g


def _pre_images(n, d):
    """The three index maps of pre_n(r, d) of include/osmosis_psf.h: [(index [n], valid [n])] for the direct image, the low and the
    high mirror."""
    r = np.arange(n)
    maps = [(r - d, np.ones(n, bool)), (-r - d, r >= 1), (2 * (n - 1) - r - d, r <= n - 2)]
    return [(np.clip(i, 0, n - 1), ok & (i >= 0) & (i < n)) for i, ok in maps]


def psf_adjoint_gather(u, k):
    """A (the adjoint map of osmosis_psf.h) of the kernel k [kh,kw] on u [B,P,H,W], pre-image by pre-image."""
    H, W = u.shape[-2:]
    kh, kw = k.shape
    g = torch.zeros_like(u)
    for ty in range(kh):
        for tx in range(kw):
            wt = float(k[ty, tx])
            if wt == 0.0:
                continue
            for iy, oky in _pre_images(H, ty - kh // 2):
                for ix, okx in _pre_images(W, tx - kw // 2):
                    m = torch.from_numpy(oky[:, None] & okx[None, :]).to(u.dtype)
                    g = g + wt * m * u[:, :, iy][:, :, :, ix]
    return g


def adjoint_gather(v, K):
    gh, gw = K.shape[:2]
    hat = hat_field(v.shape[2], v.shape[3], gh, gw)
    g = torch.zeros_like(v)
    for jy in range(gh):
        for jx in range(gw):
            g = g + psf_adjoint_gather(hat[jy, jx] * v, K[jy, jx])
    return g


def kernels_of_taps(dy, dx, w, Ry, Rx):
    """float64 [gh,gw,2 Ry + 1,2 Rx + 1] of a tap list with node weights w fp32 [gh,gw,T]."""
    w = np.asarray(w)
    K = np.zeros(w.shape[:2] + (2 * Ry + 1, 2 * Rx + 1))
    K[:, :, np.asarray(dy) + Ry, np.asarray(dx) + Rx] = w.astype(np.float64)
    return torch.from_numpy(K)


def bounds(x, v, K, T):
    """The header's first-order bounds per element: forward (T + 8) u sum_n hat_n sum |w||x|, adjoint (T + 14 + gh gw) u sum_n |A_n|
    (hat_n |v|); x, v float64."""
    gh, gw = K.shape[:2]
    return (T + 8) * U24 * forward_sum(x.abs(), K.abs()), (T + 14 + gh * gw) * U24 * adjoint_vjp(v.abs(), K.abs())
