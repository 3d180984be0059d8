"""The fp64 GroupNorm oracle of tests/gn_reference.py against torch.autograd on F.group_norm in double, at the edge shapes
of tests/test_groupnorm_gpu.py, with and without FiLM and SiLU: forward, dx, the backward means (m1, m2) and the gn_prep
table.  Agreement to 1e-12 (relative to max(1, max |reference|)): both sides are fp64 evaluations of the same formula."""
import pytest
import torch
import torch.nn.functional as F

import gn_reference as R

SHAPES = [  # G, C, HW
    (2, 8, 1), (2, 8, 3), (2, 8, 153), (4, 48, 5), (4, 48, 323), (32, 96, 37), (3, 6, 1), (3, 6, 37), (1, 512, 65),
    (256, 1024, 16),
]
TOL = 1e-12


def _err(a, b):
    return float((a - b).abs().max()) / max(1.0, float(b.abs().max()))


def _inputs(G, C, HW, film, B=3):
    g = torch.Generator().manual_seed(1000 * G + C + HW)
    x = torch.randn(B, HW, C, generator=g, dtype=torch.float64) * 1.7 + 0.4
    gamma = 1 + 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    beta = 0.1 * torch.randn(C, generator=g, dtype=torch.float64)
    fl = 0.3 * torch.randn(B, 2 * C, generator=g, dtype=torch.float64) if film else None
    dy = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    add = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    add2 = torch.randn(B, HW, C, generator=g, dtype=torch.float64)
    return x, gamma, beta, fl, dy, add, add2


def _act(z, C, fl, silu):      # z: [B][C][HW]
    if fl is not None:
        z = z * (1 + fl[:, :C, None]) + fl[:, C:, None]
    return F.silu(z) if silu else z


@pytest.mark.parametrize("silu", [False, True])
@pytest.mark.parametrize("film", [False, True])
@pytest.mark.parametrize("G,C,HW", SHAPES)
def test_reference_matches_autograd(G, C, HW, film, silu):
    eps = 1e-5
    x, gamma, beta, fl, dy, add, add2 = _inputs(G, C, HW, film)
    xr = x.permute(0, 2, 1).contiguous().requires_grad_(True)          # [B][C][HW]
    y = _act(F.group_norm(xr, G, gamma, beta, eps=float(torch.tensor(eps, dtype=torch.float32))), C, fl, silu)
    (dxr,) = torch.autograd.grad(y, xr, dy.permute(0, 2, 1))
    assert _err(R.forward(x, G, gamma, beta, fl, silu, eps), y.detach().permute(0, 2, 1)) < TOL
    dx, m1, m2 = R.backward(x, dy, G, gamma, beta, fl, silu, eps)
    assert _err(dx, dxr.permute(0, 2, 1)) < TOL
    dx2, _, _ = R.backward(x, dy, G, gamma, beta, fl, silu, eps, addend=add, addend2=add2)
    assert _err(dx2, dxr.permute(0, 2, 1) + add + add2) < TOL

    # m1, m2 from the gradient that autograd gives for xh itself (xh a leaf: no closed-form silu' on this side)
    xh = F.group_norm(x.permute(0, 2, 1), G, eps=float(torch.tensor(eps, dtype=torch.float32))).detach().requires_grad_(True)
    y2 = _act(xh * gamma[None, :, None] + beta[None, :, None], C, fl, silu)
    (dxh,) = torch.autograd.grad(y2, xh, dy.permute(0, 2, 1))
    B = x.shape[0]
    m1r = dxh.reshape(B, G, -1).mean(2)
    m2r = (dxh * xh.detach()).reshape(B, G, -1).mean(2)
    assert _err(m1, m1r) < TOL and _err(m2, m2r) < TOL

    # statistics: mean and rstd of every (image, group) slice
    mean, rstd = R.stats(x, G, eps)
    xg = x.reshape(B, HW, G, C // G)
    assert _err(mean, xg.mean(dim=(1, 3))) < TOL
    assert _err(rstd, (xg.var(dim=(1, 3), unbiased=False) + float(torch.tensor(eps, dtype=torch.float32))).rsqrt()) < TOL
    assert R.pack_stats(mean, rstd).reshape(B, G, 2)[1, G - 1, 1] == rstd[1, G - 1]

    # the table, applied per channel as a convolution does while staging, reproduces the forward
    t = R.table(x, G, gamma, beta, fl, eps)
    assert t.shape == (B, 4, C)
    z = (x - t[:, None, 0]) * t[:, None, 1] * t[:, None, 2] + t[:, None, 3]
    assert _err(F.silu(z) if silu else z, y.detach().permute(0, 2, 1)) < TOL


def test_cols_combine_matches_stats():
    """column sums of x and x^2 over row chunks, combined, give the statistics of x (mode 0) and plain means (mode 1)"""
    G, C, HW, B, nchunk = 4, 48, 40, 3, 5
    x = _inputs(G, C, HW, False)[0]
    xs = x.reshape(B, nchunk, HW // nchunk, C)
    cs = torch.stack([xs.sum(2), (xs * xs).sum(2)], dim=2)              # [B][nchunk][2][C]
    mean, rstd = R.cols_combine(cs, B, nchunk, HW, C, G, 0)
    mr, rr = R.stats(x, G)
    assert _err(mean, mr) < TOL and _err(rstd, rr) < 1e-10            # E[x^2] - mean^2 in fp64: cancellation of a few digits
    a, b = R.cols_combine(cs, B, nchunk, HW, C, G, 1)
    assert _err(a, mr) < TOL and _err(b, (x * x).reshape(B, HW, G, -1).mean(dim=(1, 3))) < TOL


def test_guarded_buffer_detects_writes_outside_the_window():
    for dtype in (torch.float32, torch.float16):
        data = torch.arange(6 * 5, dtype=torch.float64).reshape(6, 5)
        gb = R.Guarded(6, 5, width=9, c0=2, guard=3, dtype=dtype, data=data)
        assert gb.view.shape == (6, 5) and gb.view.stride() == (9, 1)
        assert torch.equal(gb.get(), data)
        gb.view.mul_(2.0)                       # inside: allowed
        gb.check()
        for r, c in ((2, 4), (3, 1), (3, 7), (9, 2), (11, 8)):      # above, left, right, below, last element
            old = gb.buf[r, c].clone()
            gb.buf[r, c] = 1.0
            assert not gb.intact()
            gb.buf[r, c] = old
            assert gb.intact()
