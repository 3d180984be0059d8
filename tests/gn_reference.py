"""fp64 reference of the GroupNorm family on NHWC views, and guarded buffers for view tests (a helper, not a test).

Everything takes and returns torch float64 CPU tensors in the kernels' own layout: activations [B][HW][C] (a group's
channels contiguous inside a pixel row), gamma / beta [C], FiLM [B][2C] = scale | shift, statistics [B][G][2].

    xh = (x - mean_g) * rstd_g          mean / biased variance over the HW x (C / G) slice of group g
    z  = (xh * gamma + beta) * (1 + scale) + shift
    y  = silu(z) or z
    dxh = dy * silu'(z) * (1 + scale) * gamma,   m1 = sum(dxh) / n,   m2 = sum(dxh * xh) / n   (per image and group)
    dx = rstd * (dxh - m1 - xh * m2) (+ addend) (+ addend2)

tests/test_gn_reference_cpu.py checks all of it against torch.autograd on F.group_norm in double."""
import numpy as np
import torch

F64 = torch.float64


def _grouped(t, G):
    B, HW, C = t.shape
    return t.reshape(B, HW, G, C // G)


def _per_channel(s, C):
    """[B][G] -> [B][1][C]"""
    B, G = s.shape
    return s.repeat_interleave(C // G, dim=1).reshape(B, 1, C)


def stats(x, G, eps=1e-5):
    """(mean, rstd), each [B][G].  eps is taken as the float32 the kernels receive."""
    xg = _grouped(x.to(F64), G)
    mean = xg.mean(dim=(1, 3))
    var = ((xg - mean[:, None, :, None]) ** 2).mean(dim=(1, 3))
    return mean, 1.0 / torch.sqrt(var + float(np.float32(eps)))


def pack_stats(a, b):
    """two [B][G] -> flat [B * G * 2], the layout of `stats` / `gstats`"""
    return torch.stack([a, b], dim=2).reshape(-1)


def _scale_shift(film, B, C):
    if film is None:
        return torch.zeros(B, 1, C, dtype=F64), torch.zeros(B, 1, C, dtype=F64)
    film = film.to(F64)
    return film[:, None, :C], film[:, None, C:2 * C]


def _xh_z(x, G, gamma, beta, film, eps):
    x = x.to(F64)
    B, HW, C = x.shape
    mean, rstd = stats(x, G, eps)
    xh = (x - _per_channel(mean, C)) * _per_channel(rstd, C)
    sc, sh = _scale_shift(film, B, C)
    z = (xh * gamma.to(F64) + beta.to(F64)) * (1.0 + sc) + sh
    return xh, z, mean, rstd


def forward(x, G, gamma, beta, film=None, silu=True, eps=1e-5):
    """act(FiLM(GN(x))), [B][HW][C]"""
    _, z, _, _ = _xh_z(x, G, gamma, beta, film, eps)
    return z * torch.sigmoid(z) if silu else z


def backward(x, dy, G, gamma, beta, film=None, silu=True, eps=1e-5, addend=None, addend2=None):
    """(dx (+ addend + addend2) [B][HW][C], m1 [B][G], m2 [B][G])"""
    B, HW, C = x.shape
    xh, z, _, rstd = _xh_z(x, G, gamma, beta, film, eps)
    dz = dy.to(F64)
    if silu:
        s = torch.sigmoid(z)
        dz = dz * (s * (1.0 + z * (1.0 - s)))
    sc, _ = _scale_shift(film, B, C)
    dxh = dz * (1.0 + sc) * gamma.to(F64)
    m1 = _grouped(dxh, G).mean(dim=(1, 3))
    m2 = _grouped(dxh * xh, G).mean(dim=(1, 3))
    dx = _per_channel(rstd, C) * (dxh - _per_channel(m1, C) - xh * _per_channel(m2, C))
    for a in (addend, addend2):
        if a is not None:
            dx = dx + a.to(F64)
    return dx, m1, m2


def table(x, G, gamma, beta, film=None, eps=1e-5):
    """the gn_prep table [B][4][C]: mean | rstd | gamma (1 + scale) | beta (1 + scale) + shift"""
    B, HW, C = x.shape
    mean, rstd = stats(x, G, eps)
    sc, sh = _scale_shift(film, B, C)
    ga = (gamma.to(F64) * (1.0 + sc)).reshape(B, C)
    be = (beta.to(F64) * (1.0 + sc) + sh).reshape(B, C)
    return torch.stack([_per_channel(mean, C).reshape(B, C), _per_channel(rstd, C).reshape(B, C), ga, be], dim=1)


def cols_combine(colsum, B, nchunk, HW, C, G, mode=0, eps=1e-5):
    """fp64 combine of column sums [B][nchunk][2][C] -> (mean, rstd) (mode 0) or (s1 / n, s2 / n) (mode 1), each [B][G]"""
    cs = colsum.to(F64).reshape(B, nchunk, 2, G, C // G).sum(dim=(1, 4))        # [B][2][G]
    n = float(HW) * (C // G)
    a, b = cs[:, 0] / n, cs[:, 1] / n
    if mode == 1:
        return a, b
    var = torch.clamp(b - a * a, min=0.0)
    return a, 1.0 / torch.sqrt(var + float(np.float32(eps)))


# ------------------------------------------------------------------------------------------------ guarded buffers
SENTINEL = -777.25      # exact in half and float


class Guarded:
    """A [rows + 2 guard][width] buffer filled with a sentinel; the operand is columns c0 : c0 + C of the middle rows
    (`view`, unit column stride, row stride `width`).  seal() remembers the bytes; check() proves that every element outside
    the window still has them."""

    def __init__(self, rows, C, width=None, c0=0, guard=4, dtype=torch.float32, device="cpu", data=None):
        width = C if width is None else width
        assert 0 <= c0 and c0 + C <= width
        self.rows, self.C, self.c0, self.guard = rows, C, c0, guard
        self.buf = torch.full((rows + 2 * guard, width), SENTINEL, dtype=dtype, device=device)
        self.view = self.buf[guard:guard + rows, c0:c0 + C]
        if data is not None:
            self.view.copy_(data.reshape(rows, C).to(dtype))
        self.seal()

    def seal(self):
        self._before = self._outside(self.buf)

    def _outside(self, buf):
        bits = buf.clone().view(torch.int16 if buf.element_size() == 2 else torch.int32)
        bits[self.guard:self.guard + self.rows, self.c0:self.c0 + self.C] = 0
        return bits

    def intact(self):
        return torch.equal(self._outside(self.buf), self._before)

    def check(self, what=""):
        assert self.intact(), f"bytes outside the window changed ({what})"

    def get(self):
        """the window as a contiguous float64 CPU tensor [rows][C]"""
        return self.view.detach().to("cpu", F64).contiguous()
