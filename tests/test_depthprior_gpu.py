"""The range-map depth prior on the GPU (include/osmosis_depthprior.h, csrc/depthprior.hip).

Kernel level: the three kernels against the float64 oracle (tests/depthprior_oracle.py) on the same fp32 x0, z, m; what is and is
not written of g; bit-equalities (one C call against the three launches, B = 2 against two B = 1 calls, repeats); every guard;
torch.library.opcheck; weight = 0.
`loss_grad_x0` with a prior against the composed oracle on the plain, masked, composed and grouped routes.
Chain level (the tiny 4 -> 8 network in f32, a 16 x 24 image, a 10-index respaced chain, injected noise, `_generic_loop` patched to
raise): fused against the oracle's loop with the term, against `_generic_loop`, chunked, tiled, and the effect of the prior."""
import math
import os

import numpy as np
import pytest
import torch

import depthprior_oracle as DO
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from physlin_oracle import DEGRADATIONS
from test_mask_gpu import (AUX, COND, OPERATORS, OPS, PATTERN, TINY_KW, T, _free_running_bar, _no_generic, _replay_randn_like, _same_bits,
                           etas, make_masks, make_sampler, model48, pkg)  # noqa: F401  (fixtures)
from test_physgroup_gpu import gcond, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
NAN = float("nan")
# depth conversions: (oracle's depth_type, value, the kernels' code, dval)
DEPTHS = {"original": ("original", None, 0, (0.0, 1.0, 1.0)), "move": ("move", 0.7, 2, (0.7, 1.0, 1.0)),
          "gamma": ("gamma", "1.4,0.9,1.3", 1, (1.4, 0.9, 1.3))}


def run_kernels(x0, z, m, prior, code, dval, g=None, single=False):
    """The prior's launches on device copies of fp32 x0 [B,4,H,W], z, m [B,1,H,W]: (g, depth_loss [B], fit [B,4]) on the CPU.
    Workspaces start as NaN: whatever is read must have been written."""
    from osmosis_diffusion_code_amd import ops
    B, _, H, W = x0.shape
    HW = H * W
    desc = ops.depth_desc(prior["align"], prior["loss"], prior["weight"], prior.get("scale", 1.0), prior.get("scale_min", 1e-3), code, dval,
                          B, HW)
    f64 = dict(device=DEV, dtype=torch.float64)
    part, fit = torch.full((B * ops.depth_nblk(HW) * 8,), NAN, **f64), torch.full((B, 4), NAN, **f64)
    loss = torch.full((B,), NAN, device=DEV)
    gd_ = (torch.zeros_like(x0) if g is None else g.clone()).to(DEV).contiguous()
    xd, zd, md = x0.to(DEV).contiguous(), z.reshape(B, 1, HW).to(DEV).contiguous(), m.reshape(B, 1, HW).to(DEV).contiguous()
    if single:
        ops.depth_reduce(desc, xd, zd, md, part)
        ops.depth_fit(desc, part, fit, loss)
        ops.depth_grad(desc, xd, zd, md, fit, gd_)
    else:
        ops.depth_loss_grad(desc, xd, zd, md, part, fit, loss, gd_)
    return gd_.cpu(), loss.cpu(), fit.cpu()


def rel(a, b):
    return abs(a - b) / abs(b) if b != 0 else abs(a)


# ------------------------------------------------------------------------------------------------------------ 1: against the oracle
# (B, H, W, valid fraction, fractional confidences): two reduce workgroups with a ragged tail; nblk = 5 (odd, the second round of
# the four-lane walk); one partial workgroup
COVER = [("b2_36x34_dense", 2, 36, 34, 1.0, False), ("b2_36x34_3pct", 2, 36, 34, 0.03, False), ("b3_74x58_frac", 3, 74, 58, 0.6, True),
         ("b3_74x58_3pct", 3, 74, 58, 0.03, True), ("b1_8x12_frac", 1, 8, 12, 0.7, True)]


@pytest.mark.parametrize("depth", list(DEPTHS))
@pytest.mark.parametrize("loss", ["norm", "mse"])
@pytest.mark.parametrize("align", ["none", "scale", "affine"])
@pytest.mark.parametrize("cover", COVER, ids=[c[0] for c in COVER])
def test_kernels_vs_the_oracle(pkg, cover, align, loss, depth):
    """a, c, L and the increment into a zeroed g.  original / move: the oracle is fed the identical fp32 d, so only the fp64
    summation order differs (N 2^-53 times the cancellation factor S_dd / S, asserted <= 1e3 on the oracle's side): 1e-9 relative;
    the increment per element within 4 x 2^-24 of its value.  gamma (powf in fp32): 5 x the oracle's own float64-d versus
    float32-d distance on the same inputs.  z holds NaN wherever m = 0."""
    name, B, H, W, frac, fractional = cover
    dtype, value, code, dval = DEPTHS[depth]
    x0, z, m = DO.problem(B, H, W, seed=11 + len(name) + 3 * B, frac=frac, fractional=fractional)
    assert bool(torch.isnan(z[m == 0]).all()) and int((m == 0).sum()) > 0 or frac == 1.0
    prior = dict(align=align, loss=loss, weight=0.625, scale=0.375, scale_min=1e-3)      # (exact in the fp32 descriptor)
    g, L, fit = run_kernels(x0, z, m, prior, code, dval)
    if depth == "gamma":
        want_L, want_inc, info = DO.term_and_increment(x0, z, m, prior, dtype, value)

        def d32(Dp):        # the conversion evaluated in fp32 by torch, carried by the float64 formula's derivative
            d64 = DO.conv_depth(Dp, dtype, value)
            return d64 + (DO.conv_depth(Dp.detach().float(), dtype, value).double() - d64.detach())
        alt_L, alt_inc, alt = DO.term_and_increment(x0, z, m, prior, dtype, value, d_override=d32)
        dist = {k: max(rel(alt[b][k], info[b][k]) for b in range(B)) for k in ("a", "c")}
        dist["L"] = max(rel(float(alt_L[b]), float(want_L[b])) for b in range(B))
        dist["inc"] = float((alt_inc - want_inc).abs().max()) / float(want_inc.abs().max())
        bars = {k: 5.0 * v for k, v in dist.items()}
    else:
        want_L, want_inc, info = DO.term_and_increment(x0, z, m, prior, dtype, value,
                                                       d_override=lambda Dp: DO.Fp32Depth.apply(Dp, dtype, value))
        bars = {"a": 1e-9, "c": 1e-9, "L": 1e-9, "inc": None}
    for b in range(B):
        assert not info[b]["skipped"] and info[b]["S"] > 0 and info[b]["Sdd"] / info[b]["S"] <= 1e3, (name, b, info[b])   # preconditions
    e = {"a": max(rel(float(fit[b, 0]), info[b]["a"]) for b in range(B)), "c": max(rel(float(fit[b, 1]), info[b]["c"]) for b in range(B)),
         "L": max(rel(float(fit[b, 3]), float(want_L[b])) for b in range(B))}
    inc = g[:, 3:4].double()
    if bars["inc"] is None:
        e["inc"] = float(((inc - want_inc).abs() / want_inc.abs().clamp_min(1e-300)).max()) / EPS      # in units of 2^-24 of the value
        ok_inc = bool(((inc - want_inc).abs() <= 4.0 * EPS * want_inc.abs()).all())
    else:
        e["inc"] = float((inc - want_inc).abs().max()) / float(want_inc.abs().max())
        ok_inc = e["inc"] <= bars["inc"]
    print(f"DEPTHPRIOR {name} {align} {loss} {depth}: a {e['a']:.2e} c {e['c']:.2e} L {e['L']:.2e} inc {e['inc']:.2e} bars {bars}")
    assert e["a"] <= bars["a"] and e["c"] <= bars["c"] and e["L"] <= bars["L"] and ok_inc, (name, align, loss, depth, e, bars)
    assert torch.equal(L, fit[:, 3].float()) and float(want_inc.abs().max()) > 0
    gs = [prior["weight"] / float(want_L[b]) if loss == "norm" else 2 * prior["weight"] / float(m[b].double().sum()) for b in range(B)]
    assert max(rel(float(fit[b, 2]), gs[b]) for b in range(B)) <= 1e-8 + (bars["L"] if depth == "gamma" else 0.0)      # (norm: gs = lambda / L)
    assert float(g[:, 0:3].abs().max()) == 0.0 and float(g[:, 3:4][m == 0].abs().max() if bool((m == 0).any()) else 0.0) == 0.0
    # a pre-filled g: g_in + inc in fp32, bit for bit; the colour planes and the m = 0 pixels keep their NaN sentinels' bits
    gen = torch.Generator().manual_seed(5)
    g_in = torch.randn(B, 4, H, W, generator=gen)
    want = g_in.clone()
    want[:, 3:4] = g_in[:, 3:4] + g[:, 3:4]
    g_in[:, 0:3] = NAN
    g_in[:, 3:4][m == 0] = NAN
    g2, L2, fit2 = run_kernels(x0, z, m, prior, code, dval, g=g_in)
    on = (m > 0).expand(B, 1, H, W)
    assert torch.equal(g2[:, 3:4][on], want[:, 3:4][on]) and torch.equal(fit2, fit) and torch.equal(L2, L)
    assert bool(torch.isnan(g2[:, 0:3]).all()) and bool(torch.isnan(g2[:, 3:4][~on]).all())


# ------------------------------------------------------------------------------------------------------------ 2: bit-equalities
@pytest.mark.parametrize("align,loss", [("affine", "norm"), ("scale", "mse"), ("none", "norm")])
def test_one_call_is_the_three_launches_batches_are_independent_and_a_repeat_repeats(pkg, align, loss):
    x0, z, m = DO.problem(2, 36, 34, seed=21, frac=0.5, fractional=True)
    prior = dict(align=align, loss=loss, weight=0.625, scale=0.375)
    code, dval = DEPTHS["gamma"][2:]
    one = run_kernels(x0, z, m, prior, code, dval)
    for other, what in ((run_kernels(x0, z, m, prior, code, dval, single=True), "three launches"),
                        (run_kernels(x0, z, m, prior, code, dval), "repeat")):
        assert all(torch.equal(a, b) for a, b in zip(one, other)), what
    for b in range(2):
        alone = run_kernels(x0[b:b + 1], z[b:b + 1], m[b:b + 1], prior, code, dval)
        assert all(torch.equal(a[b:b + 1], c) for a, c in zip(one, alone)), b
    assert float(one[0][:, 3].abs().max()) > 0


# ------------------------------------------------------------------------------------------------------------ 3: the guards
def _guard_case(name):
    """(x0, z, m, prior, code, dval, expectations) with image 1 an ordinary image beside the guarded image 0."""
    x0, z, m = DO.problem(2, 36, 34, seed=31, frac=0.5)
    z = torch.where(m > 0, z, torch.zeros_like(z))
    prior = dict(align="affine", loss="norm", weight=0.625)
    code, dval = DEPTHS["original"][2:]
    if name == "all_masked":
        m[0] = 0.0
        z[0] = NAN
    elif name == "constant_z_affine":
        z[0] = torch.where(m[0] > 0, torch.full_like(z[0], 2.5), z[0])
    elif name == "zero_z_scale":
        prior["align"] = "scale"
        z[0] = 0.0
    elif name == "nan_depth":
        idx = torch.nonzero(m[0].reshape(-1) > 0)[7]
        x0[0, 3].reshape(-1)[idx] = NAN
    elif name == "perfect_fit":
        # d = a z + c exactly in fp32: z multiples of 1/8 in [0.5, 4.5), a = 0.125, c = 0.25, D = 2 d - 1 (all exact)
        z[0] = torch.floor(z[0] * 8.0) / 8.0
        x0[0, 3] = 2.0 * (0.125 * z[0, 0] + 0.25) - 1.0
    elif name == "negative_fit":
        x0[0, 3] = (2.0 * (0.9 - 0.15 * z[0, 0] + 0.02 * torch.randn(36, 34, generator=torch.Generator().manual_seed(3))) - 1.0)
    else:
        raise KeyError(name)
    return x0.contiguous(), z.contiguous(), m.contiguous(), prior, code, dval


@pytest.mark.parametrize("name", ["all_masked", "constant_z_affine", "zero_z_scale", "nan_depth", "perfect_fit", "negative_fit"])
def test_guards(pkg, name):
    x0, z, m, prior, code, dval = _guard_case(name)
    gen = torch.Generator().manual_seed(8)
    g_in = torch.randn(2, 4, 36, 34, generator=gen)
    g, L, fit = run_kernels(x0, z, m, prior, code, dval, g=g_in)
    want_L, want_inc, info = DO.term_and_increment(x0, z, m, prior, "original", None,
                                                   d_override=lambda Dp: DO.Fp32Depth.apply(Dp, "original", None))
    # image 1 is served as ever
    assert not info[1]["skipped"] and rel(float(fit[1, 3]), float(want_L[1])) <= 1e-9 and not torch.equal(g[1, 3], g_in[1, 3])
    assert torch.equal(g[:, 0:3], g_in[:, 0:3])
    if name == "negative_fit":
        assert info[0]["a"] == 1e-3 and float(fit[0, 0]) == float(np.float32(1e-3))          # a sits on scale_min (an fp32 field) ...
        on = m[0] > 0
        c = float((m[0].double() * (DO.Fp32Depth.apply(x0[0:1, 3:4].double(), "original", None)[0] - float(fit[0, 0]) * z[0].double()))[on].sum()
                  / m[0].double()[on].sum())
        assert rel(float(fit[0, 1]), c) <= 1e-9 and float(fit[0, 3]) > 0                       # ... and c is re-solved for it
        assert not torch.equal(g[0, 3], g_in[0, 3])
        return
    assert torch.equal(g[0], g_in[0]), name                                                   # g is not written for the image
    assert float(fit[0, 2]) == 0.0
    if name == "nan_depth":
        assert math.isnan(float(L[0])) and math.isnan(float(fit[0, 3])) and info[0]["nan"]
    else:
        assert float(L[0]) == 0.0 and float(fit[0, 3]) == 0.0 and float(want_L[0]) == 0.0
    if name == "perfect_fit":
        assert not info[0]["skipped"] and rel(float(fit[0, 0]), 0.125) <= 1e-9 and rel(float(fit[0, 1]), 0.25) <= 1e-9
    elif name != "nan_depth":
        assert info[0]["skipped"] and math.isnan(float(fit[0, 0])) and math.isnan(float(fit[0, 1]))


def test_opcheck_and_zero_weight(pkg):
    x0, z, m = DO.problem(2, 12, 20, seed=41, frac=0.5, fractional=True)
    z = torch.where(m > 0, z, torch.zeros_like(z))
    xd, zd, md = x0.to(DEV), z.to(DEV), m.to(DEV)
    g0 = torch.randn(2, 4, 12, 20, generator=torch.Generator().manual_seed(2)).to(DEV)
    args = lambda g, w: (xd, zd, md, g, "affine", "norm", w, 1.0, 1e-3, 1, [1.4, 1.4, 1.0])      # noqa: E731
    g = g0.clone()
    L, fit = torch.ops.osmosis.depth_prior_loss_grad(*args(g, 0.6))
    want = run_kernels(x0, z, m, dict(align="affine", loss="norm", weight=0.6), 1, (1.4, 1.4, 1.0), g=g0.cpu())
    assert torch.equal(g.cpu(), want[0]) and torch.equal(L.cpu(), want[1]) and torch.equal(fit.cpu(), want[2])
    assert fit.dtype == torch.float64 and tuple(fit.shape) == (2, 4) and not torch.equal(g, g0)
    gz = g0.clone()
    Lz, fitz = torch.ops.osmosis.depth_prior_loss_grad(*args(gz, 0.0))
    assert torch.equal(gz, g0) and torch.equal(Lz, L) and float(fitz[:, 2].abs().max()) == 0.0     # weight 0: g is not touched
    with pytest.raises(Exception, match="align"):
        torch.ops.osmosis.depth_prior_loss_grad(xd, zd, md, g0.clone(), "log", "norm", 0.6, 1.0, 1e-3, 1, [1.4, 1.4, 1.0])
    torch.library.opcheck(torch.ops.osmosis.depth_prior_loss_grad.default, args(g0.clone(), 0.6))
    torch.library.opcheck(torch.ops.osmosis.depth_prior_loss_grad.default,
                          (xd, zd, md, g0.clone(), "scale", "mse", 0.3, 1.0, 1e-3, 0, [0.0, 1.0, 1.0]))


# ------------------------------------------------------------------------------------------------------------ 4: loss_grad_x0
ROUTES = {"plain": (2, None, None, None), "masked": (2, None, "uniform", None), "blur": (2, "gaussian_blur", None, None),
          "group": (3, None, None, (2, 1))}


def route_prior(B, H, W, seed):
    x0p, z, m = DO.problem(B, H, W, seed=seed, frac=0.4, fractional=True)
    return torch.where(m > 0, z, torch.zeros_like(z)), m


@pytest.mark.parametrize("py_loop", [False, True], ids=["one_call", "py_loop"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_loss_grad_x0_with_a_prior_vs_the_composed_oracle(pkg, monkeypatch, route, py_loop):
    """B images at 36 x 34, 5 inner iterations: loss 3e-5 relative, phi 3e-6, gradient 3e-5 of its max per image (the plain kernels'
    own bars); phi and the data loss with a prior are torch.equal to those without, and weight = 0 is no prior at all."""
    B, degname, mkind, groups = ROUTES[route]
    H, W = 36, 34
    monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1" if py_loop else "0")
    deg = None if degname is None else DEGRADATIONS[degname]
    opname = "underwater_physical_revised"
    z, m = route_prior(B, H, W, 51)
    out = {}
    for tag, weight in (("none", None), ("zero", 0.0), ("prior", 0.8)):
        cond = gcond(pkg, opname, B, groups, "mean", "sgd", 5, AUX, "norm", "depth", deg)
        h, w = cond.operator.out_shape(H, W)
        x0, y = inputs(B, H, W, h, w, 52)
        mask = None if mkind is None else make_masks(mkind, B, h, w, 53)
        if mask is not None:
            cond.set_measurement_mask(mask, batch=B, device=DEV)
        if weight is not None:
            cond.set_depth_prior(z, confidence=m, weight=weight, align="affine", loss="norm", batch=B, device=DEV)
        g, sep = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
        out[tag] = (g.cpu().clone(), sep.cpu().clone(), cond.operator.phi.cpu().clone(), cond)
    g, sep, phi, cond = out["prior"]
    for tag in ("none", "zero"):
        assert torch.equal(sep, out[tag][1]) and torch.equal(phi, out[tag][2]), (route, tag)      # the term does not touch them
    assert torch.equal(out["zero"][0], out["none"][0]) and not torch.equal(g, out["none"][0])
    assert torch.equal(g[:, 0:3], out["none"][0][:, 0:3]) and out["none"][3].depth_prior_values() is None
    okw = dict(OPS[opname], **etas(OPS[opname], 1e-3))
    prior = dict(z=z.double(), m=m.double(), weight=0.8, align="affine", loss="norm")
    want_sep, want_phi, want_g, want_Ld, info = DO.inner_loop(groups or (1,) * B, opname, okw, cond.operator.degradation, x0.double(),
                                                              y.double(), None if mask is None else mask.double(), 5, AUX, "norm", "depth",
                                                              prior)
    got_phi = {n: v.cpu() for n, v in cond.operator.variables().items()}
    e_loss = float((np.abs(sep.numpy().astype(np.float64) - want_sep) / np.abs(want_sep)).max())
    e_phi = max(float((got_phi[n].double() - want_phi[n].double()).abs().max()) for n in want_phi)
    e_g = max(float((g[b].double() - want_g[b]).abs().max()) / float(want_g[b].abs().max()) for b in range(B))
    vals = cond.depth_prior_values()
    e_Ld = float(((vals["loss"].cpu().double() - want_Ld).abs() / want_Ld).max())
    e_a = max(rel(float(vals["scale"][b]), info[b]["a"]) for b in range(B))
    print(f"DEPTHPRIOR route {route} py_loop {py_loop}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of its max, "
          f"L_depth(rel) {e_Ld:.2e} a(rel) {e_a:.2e}")
    assert e_loss <= 3e-5 and e_phi <= 3e-6 and e_g <= 3e-5 and e_Ld <= 3e-5 and e_a <= 3e-5, (route, e_loss, e_phi, e_g, e_Ld, e_a)
    assert float((want_g - DO.inner_loop(groups or (1,) * B, opname, okw, cond.operator.degradation, x0.double(), y.double(),
                                         None if mask is None else mask.double(), 5, AUX, "norm", "depth", None)[2])[:, 3].abs().max()) \
        > 1e-3 * float(want_g[:, 3].abs().max())                                              # (the prior matters in this case)


def test_prior_rows_of_a_chunk_and_errors(pkg):
    """A chunk takes its rows of the stored prior by `rows=`; a range that is not the call's images, or that ends past the batch, and
    a grid mismatch raise before any launch."""
    B, H, W = 3, 36, 34
    z, m = route_prior(B, H, W, 61)
    x0, y = inputs(B, H, W, H, W, 62)
    whole = gcond(pkg, "underwater_physical_revised", B, None, n_iter=3)
    whole.set_depth_prior(z, confidence=m, weight=0.5, batch=B, device=DEV)
    g, _ = whole.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g, phi = g.cpu().clone(), whole.operator.phi.cpu().clone()
    chunks = gcond(pkg, "underwater_physical_revised", B, None, n_iter=3)
    chunks.set_depth_prior(z, confidence=m, weight=0.5, batch=B, device=DEV)
    chunks.open_batch(B, (H, W), (H, W), DEV)
    for lo, hi in ((0, 2), (2, 3)):
        gc, _ = chunks.loss_grad_x0(x0[lo:hi].to(DEV), y[lo:hi].to(DEV), rows=(lo, hi))
        assert torch.equal(gc.cpu(), g[lo:hi]), (lo, hi)
    assert torch.equal(chunks.operator.phi.cpu(), phi)
    for a, b in zip(whole.depth_prior_values().values(), chunks.depth_prior_values().values()):
        assert torch.equal(a, b)
    with pytest.raises(ValueError, match="does not fit"):
        whole.loss_grad_x0(x0[:, :, :, :32].contiguous().to(DEV), y[:, :, :, :32].contiguous().to(DEV))
    for bad in ((0, 3), (2, 4)):        # not this call's two images; past the batch's three: fit + b * 4 would be written out of bounds
        with pytest.raises(ValueError, match="rows must be"):
            chunks.loss_grad_x0(x0[0:2].to(DEV), y[0:2].to(DEV), rows=bad)
    assert torch.equal(chunks.operator.phi.cpu(), phi)


# ============================================================================================================ chain level
CH, CW = 16, 24
CHAINS = {"revised+affine+norm": ("underwater_physical_revised", "affine", "norm", False),
          "haze+scale+mse+mask": ("haze_physical", "scale", "mse", True)}
WEIGHT = {"norm": 2.0, "mse": 8.0}


def chain_inputs(B, seed, masked, n=T, hw=(CH, CW)):
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, 4, H, W, generator=g)
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, 4, H, W, generator=g)
    mask = None
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    # a smooth range map (a ramp plus a bump) with holes, confidences in (0.2, 1]
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    z = torch.stack([1.0 + 2.5 * (0.3 * b + yy) + 1.5 * torch.exp(-((xx - 0.5) ** 2 + (yy - 0.4) ** 2) / 0.05) for b in range(B)])[:, None]
    m = (torch.rand(B, 1, H, W, generator=g) > 0.25).float() * (0.2 + 0.8 * torch.rand(B, 1, H, W, generator=g))
    z = torch.where(m > 0, z, torch.zeros_like(z))
    return x_T, y, noise, mask, z.contiguous(), m.contiguous()


def chain_cond(pkg, opname, B=1, groups=None, pattern=PATTERN):
    _, _, M, CM = pkg
    kw = {} if groups is None else dict(phi_groups=list(groups), phi_reduce="mean")
    operator = M.get_operator(opname, device=DEV, batch_size=B, **OPERATORS[opname], **kw)
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **pattern, aux_loss=AUX)


def prior_kw(z, m, align, loss, weight=None):
    return dict(z=z, confidence=m, weight=WEIGHT[loss] if weight is None else weight, align=align, loss=loss)


def oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask, prior, model=None):
    """The oracle's p_sample_loop image by image with the term in the objective (prior None: without).  Returns the merged trace
    and, per image, L_depth of the last evaluation."""
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    net = model if model is not None else (lambda x, t: U.unet_forward(sd, cfg, x, t))
    traces, Ld = [], []
    for b in range(x_T.shape[0]):
        sl = slice(b, b + 1)
        rg = DO.make_guidance(opname, dict(okw, depth_type="gamma", value="1.4,1.4,1"), None, *x_T.shape[-2:],
                              None if mask is None else mask[sl], 20, AUX, COND["loss_function"], COND["loss_weight"], DO.rows(prior, b, b + 1),
                              scale=COND["scale"], gradient_clip=COND["gradient_clip"])
        trace = []
        D.p_sample_loop(net, tb, x_T[sl], y[sl], rg, PATTERN, [noise[k][sl] for k in range(T)], trace)
        traces.append(trace)
        Ld.append(None if rg.depth_last is None else float(rg.depth_last[0][0]))
    merged = []
    for k in range(T):
        recs = [t[k] for t in traces]
        merged.append({"x_in": torch.cat([r["x_in"] for r in recs]), "x_out": torch.cat([r["x_out"] for r in recs]),
                       "x0": torch.cat([r["x0"] for r in recs]), "loss": np.concatenate([np.asarray(r["loss"]).reshape(-1) for r in recs]),
                       "phi": {name: torch.cat([r["phi"][name] for r in recs]) for name in recs[0]["phi"]}})
    return merged, Ld


def depth_loss_of(x0, z, m, align, loss):
    """L_depth [B] of a pred_xstart under the chains' gamma conversion, float64."""
    d = DO.conv_depth(x0[:, 3:4].double(), "gamma", "1.4,1.4,1")
    return DO.term(d, z.double(), m.double(), align, loss)[0]


def fused_vs_oracle(pkg, monkeypatch, model, tag, opname, ref, pert, x_T, y, noise, mask, depth_prior, tiling=None):
    """The project's chain protocol (tests/test_mask_gpu.py, test_tiled_gpu.py): free-running at 10 x the oracle's own drift under a
    1e-6 perturbation of x_T (`_free_running_bar`; loss 20 x that, phi 2e-6); where the oracle cannot reproduce itself to 1e-3,
    teacher-forced per index at 1e-3 / 2e-5 / 2e-6.  Returns (the fused chain's last trace record and conditioner, bar)."""
    _, gd, _, _ = pkg
    B = x_T.shape[0]
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)

    def hip(x_start, index_range=None, phi0=None, k0=0):
        cond = chain_cond(pkg, opname, B)
        if phi0 is not None:
            for name, (off, n) in cond.operator._slots().items():
                cond.operator.phi[:, off:off + n] = phi0[name].reshape(B, -1)[:, :n].to(DEV)
        trace = []
        kw = {} if index_range is None else {"index_range": index_range}
        if tiling is not None:
            kw["tiling"] = tiling
        sampler.p_sample_loop(model=model, x_start=x_start.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k0 + k], trace=trace, measurement_mask=mask, depth_prior=depth_prior, **kw)
        return trace, cond

    def errs(a, b, slots):
        e_phi = max(float((a["phi"][:, off:off + n].cpu() - b["phi"][name].reshape(B, -1)[:, :n]).abs().max())
                    for name, (off, n) in slots.items())
        want = np.asarray(b["loss"], dtype=np.float64).reshape(-1)
        return (float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max()),
                float((np.abs(a["loss"].cpu().numpy().reshape(-1) - want) / want).max()), e_phi)
    if bar is not None:
        trace, cond = hip(x_T)
        assert len(trace) == T
        f_img, f_x0, f_loss, f_phi = errs(trace[-1], ref[-1], cond.operator._slots())
        msg = (f"DEPTHPRIORCHAIN {tag}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
               f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}")
        print(msg)
        assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
        return trace[-1], cond, bar, True
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(T):
        idx = T - 1 - k
        trace, cond = hip(ref[k]["x_in"], (idx, idx), None if k == 0 else ref[k - 1]["phi"], k0=k)
        worst = [max(w_, e) for w_, e in zip(worst, errs(trace[0], ref[k], cond.operator._slots()))]
    msg = (f"DEPTHPRIORCHAIN {tag}: oracle drift_1e-6 {drift:.2e} > 1e-3, teacher-forced per index: x_out {worst[0]:.2e} x0 {worst[1]:.2e} "
           f"loss(rel) {worst[2]:.2e} phi {worst[3]:.2e}")
    print(msg)
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 2e-5 and worst[3] < 2e-6, msg
    return trace[0], cond, 1e-3, False


def _ref_setup():
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    return cfg, sd, tb


@pytest.mark.parametrize("case", list(CHAINS))
def test_fused_chain_with_a_prior_vs_the_oracle_and_the_effect_of_the_prior(pkg, monkeypatch, model48, case):
    """B = 2, free-running against the oracle's loop with the term.  The effect: the oracle's chain with the prior ends with a
    smaller L_depth than its chain without (the precondition: a ratio below 0.97 -- `WEIGHT` was chosen on the CPU for that), and the
    fused chains reproduce both values to the chain bar: |L_fused - L_oracle| <= bar x L_oracle, the bar being the one the final image
    and pred_xstart are held to (10 x the oracle's own drift).  The chains are fixed CPU quantities whose drift stays below 1e-4, so
    the comparison is free-running: asserted as a precondition, the effect is never skipped."""
    opname, align, loss, masked = CHAINS[case]
    cfg, sd, tb = _ref_setup()
    x_T, y, noise, mask, z, m = chain_inputs(2, 301, masked)
    prior = dict(z=z, m=m, weight=WEIGHT[loss], align=align, loss=loss)
    ref, ref_Ld = oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask, prior)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert, _ = oracle_chain(opname, cfg, sd, tb, x_T + bump, y, noise, mask, prior)
    last, cond, bar, free_running = fused_vs_oracle(pkg, monkeypatch, model48, case, opname, ref, pert, x_T, y, noise, mask, prior_kw(z, m, align, loss))
    # the effect of the prior, on the oracle first
    free, _ = oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask, None)
    L_with, L_without = depth_loss_of(ref[-1]["x0"], z, m, align, loss), depth_loss_of(free[-1]["x0"], z, m, align, loss)
    assert np.allclose(L_with.numpy(), ref_Ld, rtol=1e-12)
    ratio = (L_with / L_without).numpy()
    print(f"DEPTHPRIORCHAIN {case}: oracle L_depth with / without the prior {L_with.numpy()} / {L_without.numpy()}, ratio {ratio}")
    assert float(ratio.max()) < 0.97, ratio
    assert free_running, f"{case}: the oracle's drift left only teacher forcing: no free-running fused chain to read L_depth from"
    got_with = depth_loss_of(last["x0"].cpu(), z, m, align, loss)
    vals = cond.depth_prior_values()
    e_with = float(((got_with - L_with).abs() / L_with).max())
    e_vals = float(((vals["loss"].cpu().double() - L_with).abs() / L_with).max())
    assert e_with <= bar and e_vals <= bar, (case, e_with, e_vals, bar)
    assert bool(torch.isfinite(vals["scale"]).all()) and bool(torch.isfinite(vals["shift"]).all())
    # ... and without the prior (no prior set: the chain as it always was)
    _, gd, _, _ = pkg
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)
    cond0 = chain_cond(pkg, opname, 2)
    out0 = sampler.p_sample_loop(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond0.conditioning,
                                 record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                                 noise_fn=lambda k, shape: nd[k], measurement_mask=mask)
    got_without = depth_loss_of(out0[3].cpu(), z, m, align, loss)
    e_without = float(((got_without - L_without).abs() / L_without).max())
    print(f"DEPTHPRIORCHAIN {case}: fused L_depth against the oracle's, relative: with the prior {e_with:.2e} (its reported value "
          f"{e_vals:.2e}), without {e_without:.2e}; bar {bar:.2e}")
    assert e_without <= bar, (case, e_without, bar)
    assert cond0.depth_prior_values() is None


def _chain(pkg, monkeypatch, model, B, sizes=None, groups=None, seed=302, tiling=None, prior=True, weight=None, fused=True, hw=(CH, CW)):
    _, gd, _, _ = pkg
    x_T, y, noise, mask, z, m = chain_inputs(B, seed, True, hw=hw)
    nd = noise.to(DEV)
    sampler = make_sampler(gd)
    if sizes is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: list(sizes)))
    cond = chain_cond(pkg, "underwater_physical_revised", B, groups)
    kw = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False, save_root=None,
              pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN, measurement_mask=mask)
    if prior:
        kw["depth_prior"] = prior_kw(z, m, "affine", "norm", weight)
    if tiling is not None:
        kw["tiling"] = tiling
    if fused:
        _no_generic(monkeypatch, sampler)
        out = sampler.p_sample_loop(noise_fn=lambda k, shape: nd[k], **kw)
    else:
        cond.hip_ok = lambda: False             # the conditioner declines the fused loop; its step (the kernels) stays
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, PATTERN, tuple(x_T.shape)) is None
        _replay_randn_like(monkeypatch, nd, 4)
        out = sampler.p_sample_loop(**kw)
    monkeypatch.undo()
    return out, cond


def test_chunks_groups_one_tile_and_zero_weight_bit_for_bit(pkg, monkeypatch, model48):
    """A B = 3 chain with a prior walked as chunks of [2, 1] is the one-pass chain; with shared water ([2, 1] groups, the fit stays
    per image) likewise; one tile covering the canvas is the untiled chain; weight = 0 is the chain without a prior.  Bit for bit."""
    whole, cond = _chain(pkg, monkeypatch, model48, 3, [3])
    assert bool(torch.isfinite(whole[0]).all()) and tuple(cond.depth_prior_values()["loss"].shape) == (3,)
    _same_bits(_chain(pkg, monkeypatch, model48, 3, [2, 1])[0], whole, "prior: one pass vs chunks of [2, 1]")
    grouped = _chain(pkg, monkeypatch, model48, 3, [3], groups=(2, 1))[0]
    _same_bits(_chain(pkg, monkeypatch, model48, 3, [2, 1], groups=(2, 1))[0], grouped, "prior + shared water: one pass vs chunks of [2, 1]")
    assert not torch.equal(grouped[0], whole[0])
    free = _chain(pkg, monkeypatch, model48, 3, [3], prior=False)[0]
    assert not torch.equal(free[0], whole[0])                                               # the prior matters
    _same_bits(_chain(pkg, monkeypatch, model48, 3, [3], weight=0.0)[0], free, "weight = 0 vs no prior")
    one = _chain(pkg, monkeypatch, model48, 1, seed=303)[0]
    tiled = _chain(pkg, monkeypatch, model48, 1, seed=303, tiling=dict(tile=(CH, CW), stride=(CH, CW), window="uniform"))[0]
    _same_bits(tiled, one, "prior: one 16 x 24 tile vs the untiled fused chain")


@pytest.mark.parametrize("B,sizes", [(3, [2, 1]), (4, [2, 2])], ids=["2+1", "2+2"])
def test_a_chunked_walk_reports_every_images_own_fit(pkg, monkeypatch, model48, B, sizes):
    """`depth_prior_values()` after a batch walked in chunks ([2, 1]: two workspaces; [2, 2]: one workspace used twice) is [B] and
    equals the one-pass values row by row, bit for bit -- every chunk writes its rows of the per-batch results."""
    whole, cw = _chain(pkg, monkeypatch, model48, B, [B], seed=306)
    chunked, cc = _chain(pkg, monkeypatch, model48, B, sizes, seed=306)
    _same_bits(chunked, whole, f"prior: one pass vs chunks of {sizes}")
    vw, vc = cw.depth_prior_values(), cc.depth_prior_values()
    for k in ("loss", "scale", "shift"):
        assert tuple(vc[k].shape) == (B,) and bool(torch.isfinite(vc[k]).all()) and torch.equal(vc[k], vw[k]), (k, vc[k], vw[k])
    assert len(set(vc["loss"].tolist())) == B                                               # (the images differ: a mix-up would show)


def test_fused_chain_with_a_prior_equals_the_generic_loop(pkg, monkeypatch, model48):
    """Both loops on B = 2 with the same mask, prior and injected noise, at tests/test_physgroup_gpu.py's fused-versus-generic bars
    (image and pred_xstart 1e-4, loss rtol 1e-5, phi 1e-6)."""
    (f, cf), (g, cg) = _chain(pkg, monkeypatch, model48, 2, seed=304), _chain(pkg, monkeypatch, model48, 2, seed=304, fused=False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"DEPTHPRIORGENERIC: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6 and np.allclose(f[2], g[2], rtol=1e-5)
    assert torch.allclose(cf.depth_prior_values()["loss"], cg.depth_prior_values()["loss"], rtol=1e-4)
    free = _chain(pkg, monkeypatch, model48, 2, seed=304, prior=False)[0]
    assert float((f[0] - free[0]).abs().max()) > 10 * max(e_img, 1e-6)                      # (a difference the bars would see)


def test_tiled_chain_with_a_prior_over_the_canvas_vs_the_tiled_oracle(pkg, monkeypatch, model48):
    """A 24 x 36 canvas of six 16 x 16 tiles (hann window) with a range map over the canvas -- ONE fit for it -- against the oracle's
    loop around tests/test_tiled_gpu.py's tiled wrapper of the oracle's network, with the term; that file's protocol and bars."""
    from test_tiled_gpu import CANVAS, TILING, tiled_oracle_model
    _, gd, _, _ = pkg
    cfg, sd, tb = _ref_setup()
    opname = "underwater_physical_revised"
    x_T, y, noise, mask, z, m = chain_inputs(1, 305, False, hw=CANVAS)
    tiling = dict(TILING, window="hann")
    origins, wy, wx, inv = gd.tile_grid(*CANVAS, TILING["tile"], TILING["stride"], "hann")
    net = tiled_oracle_model(sd, cfg, origins, wy, wx, inv, *TILING["tile"])
    prior = dict(z=z, m=m, weight=WEIGHT["norm"], align="affine", loss="norm")
    ref, _ = oracle_chain(opname, cfg, sd, tb, x_T, y, noise, None, prior, model=net)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert, _ = oracle_chain(opname, cfg, sd, tb, x_T + bump, y, noise, None, prior, model=net)
    free, _ = oracle_chain(opname, cfg, sd, tb, x_T, y, noise, None, None, model=net)
    assert float((free[-1]["x_out"] - ref[-1]["x_out"]).abs().max()) > 1e-3                 # (the prior matters on this canvas)
    fused_vs_oracle(pkg, monkeypatch, model48, "tiled 24x36 hann", opname, ref, pert, x_T, y, noise, None,
                    prior_kw(z, m, "affine", "norm"), tiling=tiling)


# ------------------------------------------------------------------------------------------------------------ the driver
RESULT_KEYS = {"depth_prior", "depth_confidence", "depth_scale", "depth_shift", "depth_loss_final", "depth_metric"}


def driver_cfg(depth=None):
    op_cfg = dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised")
    cfg = {"measurement": {"operator": op_cfg, "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    if depth is not None:
        cfg["measurement"]["depth"] = depth
    return cfg


def driver_range(seed, n=1):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 256), torch.linspace(0, 1, 256), indexing="ij")
    zs = [(1.0 + (2.0 + i) * yy + 0.5 * xx + 0.05 * torch.randn(256, 256, generator=g))[None, None] for i in range(n)]
    for z in zs:
        z[..., 40:90, 100:180] = NAN                                  # a hole in the range map
    return zs


def test_restore_image_with_a_range_map(pkg, monkeypatch, model48, tmp_path):
    """`restore_image(depth=)` on the 3-index low-noise sub-chain: every result key of the prior is there, `depth_metric` inverts the
    fit on the converted depth and is finite (a is defined), `phi_metric` exists for align 'scale' only, `save_outputs` writes the
    two pictures, and the config key `measurement.depth.path` (a .npy at the photo's resolution) is the same chain."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    photo = (torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(401)) * 1.2 - 0.6).to(DEV)
    (z,) = driver_range(402)
    sub = dict(index_range=(2, 0), x_scale=0.05, noise_seed=7)
    res = sampling.restore_image(model48, photo, driver_cfg(dict(weight=2.0, align="affine")), depth=z, **sub)[-1]
    assert RESULT_KEYS <= set(res) and "phi_metric" not in res
    a, c = res["depth_scale"], res["depth_shift"]
    assert math.isfinite(a) and math.isfinite(c) and a >= 1e-3 and res["depth_loss_final"] > 0
    assert res["depth_metric"].shape == (256, 256) and bool(torch.isfinite(res["depth_metric"]).all())
    assert torch.allclose(res["depth_metric"] * a + c, res["depth_calc"][0], atol=1e-5)
    hole = res["depth_confidence"][40:90, 100:180]
    assert float(hole.max()) == 0.0 and float(res["depth_prior"][40:90, 100:180].abs().max()) == 0.0
    assert float(res["depth_confidence"].sum()) == 256 * 256 - 50 * 80
    paths = sampling.save_outputs(res, photo, str(tmp_path), "photo")
    assert {"depth_metric", "depth_prior"} <= set(paths) and all(os.path.getsize(p) > 0 for p in paths.values())
    free = sampling.restore_image(model48, photo, driver_cfg(), **sub)[-1]
    assert not RESULT_KEYS & set(free) and not torch.equal(free["sample"], res["sample"])
    assert "depth_metric" not in sampling.save_outputs(free, photo, str(tmp_path / "free"), "photo")
    # align = scale through the config file's path: phi per unit of range
    np.save(str(tmp_path / "range.npy"), z[0, 0].numpy())
    cfg = driver_cfg(dict(weight=2.0, align="scale", loss="mse", path=str(tmp_path / "range.npy")))
    by_path = sampling.restore_image(model48, photo, cfg, **sub)[-1]
    by_arg = sampling.restore_image(model48, photo, driver_cfg(dict(weight=2.0, align="scale", loss="mse")), depth=z, **sub)[-1]
    assert torch.equal(by_path["sample"], by_arg["sample"]) and by_path["depth_shift"] == 0.0
    for k, v in by_path["phi"].items():
        want = v if k == "phi_inf" else v * by_path["depth_scale"]
        assert torch.equal(by_path["phi_metric"][k], want), k
    with pytest.raises(ValueError, match="unknown key"):
        sampling.restore_image(model48, photo, driver_cfg(dict(weight=2.0, huber=1.0)), depth=z, **sub)
    with pytest.raises(ValueError, match="image grid"):
        sampling.restore_image(model48, photo, driver_cfg(), depth=z[..., :128], **sub)


def test_restore_images_in_batches_gives_each_image_its_own_row(pkg, monkeypatch, model48):
    """`restore_images(batch_size=2, depths=)`: three photos, the second without a range map.  Every image with a map carries its own
    map and fit; in the batch of two, the image without one has confidence 0 (no prior: an undefined fit, NaN metric depth) and the
    other's fit is the one its batch-1 run finds (1e-4 relative: the bar of tests/test_configs_gpu.py's batched sub-chains)."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(403)
    photos = [(torch.rand(1, 3, 256, 256, generator=g) * 1.2 - 0.6).to(DEV) for _ in range(3)]
    zs = driver_range(404, 3)
    depths = [zs[0], None, zs[2]]
    sub = dict(index_range=(2, 0), x_scale=0.05, noise_seed=7)
    cfg = driver_cfg(dict(weight=2.0, align="affine", loss="norm"))
    two = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=2, depths=depths, **sub)
    one = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=1, depths=depths, **sub)
    assert sorted(two) == sorted(one) == [0, 1, 2]
    for i in (0, 2):
        r = two[i]
        assert RESULT_KEYS <= set(r) and bool(torch.isfinite(r["depth_metric"]).all())
        want = torch.where(torch.isfinite(zs[i][0, 0]), zs[i][0, 0], torch.zeros(()))
        assert torch.equal(r["depth_prior"], want)
        assert abs(r["depth_scale"] - one[i]["depth_scale"]) <= 1e-4 * abs(one[i]["depth_scale"])
        assert abs(r["depth_loss_final"] - one[i]["depth_loss_final"]) <= 1e-4 * one[i]["depth_loss_final"]
        assert abs(r["depth_shift"] - one[i]["depth_shift"]) <= 1e-4 * abs(one[i]["depth_shift"])
    assert two[0]["depth_shift"] != two[2]["depth_shift"] and two[0]["depth_loss_final"] != two[2]["depth_loss_final"]
    r = two[1]                                                          # batched beside image 0: a row of zeros
    assert float(r["depth_confidence"].max()) == 0.0 and math.isnan(r["depth_scale"]) and r["depth_loss_final"] == 0.0
    assert bool(torch.isnan(r["depth_metric"]).all())
    assert not RESULT_KEYS & set(one[1])                                # alone: no prior at all


def test_restore_image_on_a_chunked_batch_attaches_each_images_own_fit(pkg, monkeypatch, model48):
    """A batch of two walked as chunks of [1, 1] (what little free memory or a cap on the images in flight does): `restore_image`
    with the image-0 post-processing attaches image 0's fit, `restore_images(batch_size=2)` every image's own -- the values of the
    one-pass walk to 1e-4 relative (the full-size network's rounding depends on the engine's batch: the bar of the batched sub-chains
    above), far below the difference between the two images."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(405)
    photos = [(torch.rand(1, 3, 256, 256, generator=g) * 1.2 - 0.6).to(DEV) for _ in range(2)]
    zs = driver_range(406, 2)
    zs[1][..., 128:, :] = NAN             # the second map covers the upper half only: its L_depth is that of half the pixels
    sub = dict(index_range=(2, 0), x_scale=0.05, noise_seed=7)
    cfg = driver_cfg(dict(weight=2.0, align="affine", loss="norm"))
    keys = ("depth_scale", "depth_shift", "depth_loss_final")

    def run():
        both = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=2, depths=zs, **sub)
        first = sampling.restore_image(model48, torch.cat(photos, 0), cfg, device=DEV, same_seed_per_image=True, depth=torch.cat(zs, 0),
                                       **sub)[-1]
        return both, first
    whole, whole0 = run()
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: [1] * B_))
    chunked, chunked0 = run()
    def close(a, b):
        return a == b or abs(a - b) <= 1e-4 * abs(b)
    for i in range(2):
        assert RESULT_KEYS <= set(chunked[i]) and all(close(chunked[i][k], whole[i][k]) and math.isfinite(chunked[i][k]) for k in keys), \
            (i, [(chunked[i][k], whole[i][k]) for k in keys])
        assert torch.equal(chunked[i]["depth_prior"], whole[i]["depth_prior"]) and bool(torch.isfinite(chunked[i]["depth_metric"]).all())
    assert abs(whole[0]["depth_loss_final"] - whole[1]["depth_loss_final"]) > 0.1 * whole[1]["depth_loss_final"]     # a mix-up would show
    # the image-0 post-processing reads image 0's row, not the last chunk's: the same walk, the same bits
    assert all(chunked0[k] == chunked[0][k] for k in keys) and all(whole0[k] == whole[0][k] for k in keys)
