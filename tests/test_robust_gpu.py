"""The robust data term on the GPU (include/osmosis_robust.h, csrc/robust.hip).

Kernel level: the select bit for bit against the float32 restatement of the contract (tests/robust_oracle.sigma32, numpy sort), the
weights against float64 from the same fp32 e and sigma, the exact cases, the bit-equalities, torch.library.opcheck.
`loss_grad_x0` with the term against the masked guidance oracle with the robust weights in float64, on the plain, masked and grouped
routes and on the 'ps' identity term; omega = 1; OSM_PHYS_PY_LOOP; all-zero weights; the effect on phi under outliers.
Chain level (the tiny 4 -> 8 network in f32, 16 x 24, a 10-index chain, injected noise): fused against the oracle's loop with the
term, chunked, tiled, against `_generic_loop`; the driver."""
import math
import os

import numpy as np
import pytest
import torch

import robust_oracle as RO
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from test_mask_gpu import (AUX, COND, OPERATORS, OPS, PATTERN, TINY_KW, T, _free_running_bar, _no_generic, _replay_randn_like, _same_bits,
                           etas, make_masks, make_sampler, model36, model48, pkg)  # noqa: F401  (fixtures)
from test_physgroup_gpu import gcond, inputs

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
NAN = float("nan")
SHAPES = [(2, 36, 34), (3, 74, 58), (1, 8, 12)]     # 3672 keys: ragged against 1024 lanes; 12876; 288: fewer keys than lanes
C32 = {k: float(np.float32(v)) for k, v in RO.C_DEFAULT.items()}


def run_kernels(pred, pa, pb, y, M0, robust, single=False):
    """The launches on device copies of fp32 pred [B,P,hw], y [B,3,hw], M0 [B,3,hw] or None: a dict of CPU tensors.  Every output
    starts as NaN (n_valid as -7): whatever is read must have been written."""
    from osmosis_diffusion_code_amd import ops
    B, _, hw = y.shape
    d = ops.robust_desc(robust["loss"], robust.get("c"), robust.get("scale", "mad"), robust.get("sigma_min", RO.SIGMA_MIN),
                        robust.get("per_pixel", False), B, hw)
    f = lambda: torch.full((B, 3, hw), NAN, device=DEV)     # noqa: E731
    e, meff, omega, sigma = f(), f(), f(), torch.full((B,), NAN, device=DEV)
    n = torch.full((B,), -7, device=DEV, dtype=torch.int32)
    pd, yd, md = pred.to(DEV).contiguous(), y.to(DEV).contiguous(), None if M0 is None else M0.to(DEV).contiguous()
    if single:
        ops.robust_resid(d, pd, pa, pb, yd, e)
        if d.scale_mode == 0:
            ops.robust_scale(d, e, md, sigma, n)
        ops.robust_weights(d, e, md, sigma, meff, omega)
    else:
        ops.robust_mask(d, pd, pa, pb, yd, md, e, sigma, n, meff, omega)
    torch.cuda.synchronize()
    return {"e": e.cpu(), "sigma": sigma.cpu(), "n": n.cpu(), "meff": meff.cpu(), "omega": omega.cpu()}


def from_e(e, M0, robust, **kw):
    """Feed a chosen residual: pred = 0 with (pa, pb) = (1, 0) makes e = y - 0 = y, bit for bit (-0 included)."""
    out = run_kernels(torch.zeros_like(e), 1.0, 0.0, e, M0, robust, **kw)
    assert _bits_equal(out["e"], e)
    return out


def _bits_equal(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


# ------------------------------------------------------------------------------------------------------------ 1: the inputs
KINDS = ["dense", "3pct", "fractional", "odd", "even", "n1", "n0", "ties", "all_equal", "wide", "negzero_denormals", "nonfinite"]


def kernel_case(kind, B, H, W, seed):
    """(e [B,3,hw] fp32, M0 [B,3,hw] or None, sigma_min)."""
    g = torch.Generator().manual_seed(seed)
    hw = H * W
    e = 0.05 * torch.randn(B, 3, hw, generator=g)
    out = torch.rand(B, 1, hw, generator=g) < 0.05                        # 5 % outlier pixels on all channels
    e = torch.where(out, 0.6 + 0.4 * torch.rand(B, 3, hw, generator=g), e)
    M0, sigma_min = None, RO.SIGMA_MIN
    if kind == "3pct":
        M0 = (torch.rand(B, 3, hw, generator=g) < 0.03).float()
    elif kind == "fractional":
        M0 = torch.rand(B, 3, hw, generator=g) * (torch.rand(B, 3, hw, generator=g) > 0.3).float()
    elif kind in ("odd", "even"):
        M0 = (torch.rand(B, 3, hw, generator=g) > 0.4).float()
        for b in range(B):
            n = int((M0[b] > 0).sum())
            if (n % 2 == 1) != (kind == "odd"):
                M0[b].view(-1)[int(torch.nonzero(M0[b].view(-1) > 0)[0])] = 0.0
            assert int((M0[b] > 0).sum()) % 2 == (1 if kind == "odd" else 0)
    elif kind == "n1":
        M0 = torch.zeros(B, 3, hw)
        for b in range(B):
            M0[b].view(-1)[(7 + 13 * b) % (3 * hw)] = 0.75
    elif kind == "n0":
        M0 = (torch.rand(B, 3, hw, generator=g) > 0.5).float()
        M0[0] = 0.0                                                      # image 0 has no valid entry; the others are ordinary
    elif kind == "ties":
        e = torch.round(e * 255.0) / 255.0
    elif kind == "all_equal":
        e = torch.full((B, 3, hw), 0.125)
        e[-1] = 0.0                                                      # ... and an all-zero image: sigma = sigma_min, u = 0
    elif kind == "wide":
        e = torch.sign(torch.randn(B, 3, hw, generator=g)) * 10.0 ** (torch.rand(B, 3, hw, generator=g) * 30.3 - 30.0)   # 1e-30 .. 2
        sigma_min = 0.0
    elif kind == "negzero_denormals":
        r = torch.rand(B, 3, hw, generator=g)
        e = torch.where(r < 0.2, torch.full_like(e, -0.0), e)
        e = torch.where((r >= 0.2) & (r < 0.45), torch.full_like(e, 1e-41) * torch.randint(1, 9, e.shape, generator=g).float(), e)
        M0 = (torch.rand(B, 3, hw, generator=g) > 0.2).float()
    elif kind == "nonfinite":
        M0 = (torch.rand(B, 3, hw, generator=g) > 0.4).float() * torch.rand(B, 3, hw, generator=g)
        r = torch.rand(B, 3, hw, generator=g)
        e = torch.where(r < 0.02, torch.full_like(e, NAN), e)
        e = torch.where((r >= 0.02) & (r < 0.04), torch.full_like(e, float("inf")), e)
        e = torch.where((r >= 0.04) & (r < 0.06), torch.full_like(e, -float("inf")), e)
        bad = ~torch.isfinite(e)
        assert bool((bad & (M0 > 0)).any()) and bool((bad & (M0 == 0)).any())       # at valid and at masked-out places
    elif kind != "dense":
        raise KeyError(kind)
    return e.contiguous(), None if M0 is None else M0.contiguous(), sigma_min


WORST = {"meff": 0.0, "omega": 0.0}


@pytest.mark.parametrize("shape", SHAPES, ids=["b2_36x34", "b3_74x58", "b1_8x12"])
@pytest.mark.parametrize("kind", KINDS)
def test_kernels_vs_the_contract(pkg, kind, shape):
    """sigma and n: bit-equal to the float32 restatement (0 ulp: every step is one correctly rounded fp32 operation).  M_eff and omega:
    within 8 x 2^-24 absolute of float64 from the same fp32 e, sigma and c (at most six roundings on quantities <= 1; the three omega
    are continuous, so the u = 1 branch cannot break it).  Exact: 0 where M0 = 0, M0's bits where e is not finite."""
    B, H, W = shape
    i = KINDS.index(kind)
    e, M0, sigma_min = kernel_case(kind, B, H, W, seed=100 + 7 * i + B)
    want_sigma, want_n = RO.sigma32(e.numpy(), None if M0 is None else M0.numpy(), sigma_min)
    per_pixel = bool((i + B) % 2)
    for loss in RO.LOSSES:
        out = from_e(e, M0, dict(loss=loss, sigma_min=sigma_min, per_pixel=per_pixel))
        got_sigma = out["sigma"].numpy()
        assert np.array_equal(out["n"].numpy().astype(np.int64), want_n), (kind, shape, out["n"], want_n)
        assert np.array_equal(np.isnan(got_sigma), np.isnan(want_sigma)) and \
            np.array_equal(got_sigma[~np.isnan(want_sigma)].view(np.int32), want_sigma[~np.isnan(want_sigma)].view(np.int32)), \
            (kind, shape, got_sigma, want_sigma)
        m64, o64 = RO.weights64(e.numpy(), None if M0 is None else M0.numpy(), got_sigma, loss, C32[loss], per_pixel)
        d_m = float(np.abs(out["meff"].numpy().astype(np.float64) - m64).max())
        d_o = float(np.abs(out["omega"].numpy().astype(np.float64) - o64).max())
        WORST["meff"], WORST["omega"] = max(WORST["meff"], d_m / (8 * EPS)), max(WORST["omega"], d_o / (8 * EPS))
        print(f"ROBUST {kind} {shape} {loss} per_pixel {per_pixel}: sigma {got_sigma} n {want_n} |dM_eff| {d_m / EPS:.2f} |domega| "
              f"{d_o / EPS:.2f} x 2^-24 (bar 8); worst so far / bar: M_eff {WORST['meff']:.3f} omega {WORST['omega']:.3f}")
        assert not np.isnan(out["meff"].numpy()[np.isfinite(e.numpy())]).any() and d_m <= 8 * EPS and d_o <= 8 * EPS, (kind, loss, d_m, d_o)
        m0 = torch.ones_like(e) if M0 is None else M0
        assert float(out["meff"][m0 == 0].abs().max() if bool((m0 == 0).any()) else 0.0) == 0.0
        bad = ~torch.isfinite(e)
        assert _bits_equal(out["meff"][bad], m0[bad]) and bool((out["omega"][bad] == 1.0).all())
        if per_pixel:       # one weight per pixel: the valid channels of a pixel carry the same omega, that of the worst of them
            ok = torch.isfinite(e) & (m0 > 0) & ~torch.isnan(out["sigma"])[:, None, None]
            om = torch.where(ok, out["omega"], torch.full_like(e, 2.0))
            lo = om.min(dim=1, keepdim=True).values
            assert bool(((om == lo) | ~ok).all())
            own = from_e(e, M0, dict(loss=loss, sigma_min=sigma_min, per_pixel=False))["omega"]
            assert bool(((out["omega"] <= own) | ~ok).all())
    if kind == "n0":
        assert want_n[0] == 0 and math.isnan(float(out["sigma"][0])) and _bits_equal(out["meff"][0], M0[0])
    if kind == "n1":
        assert (want_n == 1).all()
    if kind == "all_equal":
        assert float(out["sigma"][-1]) == float(np.float32(RO.SIGMA_MIN)) and bool((out["omega"][-1] == 1.0).all())


@pytest.mark.parametrize("pa,pb,P", [(2.0, -1.0, 3), (2.0, -1.0, 4), (1.0, 0.0, 3), (1.0, 0.0, 4)])
def test_residual_is_the_unfused_form_and_reads_pred_with_its_batch_stride(pkg, pa, pb, P):
    g = torch.Generator().manual_seed(3)
    B, hw = 2, 36 * 34
    pred, y = torch.rand(B, P, hw, generator=g), torch.rand(B, 3, hw, generator=g) * 2 - 1
    got = run_kernels(pred, pa, pb, y, None, dict(loss="tukey"))["e"]
    t = (np.float32(pa) * pred[:, 0:3].numpy()).astype(np.float32)
    want = y.numpy() - (t + np.float32(pb)).astype(np.float32)
    assert _bits_equal(got, torch.from_numpy(want.astype(np.float32)))


# ------------------------------------------------------------------------------------------------------------ 2: bit-equalities
@pytest.mark.parametrize("loss", RO.LOSSES)
def test_one_call_is_the_three_launches_batches_are_independent_a_repeat_repeats_and_a_fixed_scale_is_the_mad_scale(pkg, loss):
    e, M0, _ = kernel_case("fractional", 2, 36, 34, seed=21)
    rb = dict(loss=loss, per_pixel=loss == "huber")
    one = from_e(e, M0, rb)
    for other, what in ((from_e(e, M0, rb, single=True), "three launches"), (from_e(e, M0, rb), "repeat")):
        assert all(_bits_equal(one[k].float(), other[k].float()) for k in one), what
    for b in range(2):
        alone = from_e(e[b:b + 1], M0[b:b + 1], rb)
        assert all(_bits_equal(one[k][b:b + 1].float(), alone[k].float()) for k in one), b
        fixed = from_e(e[b:b + 1], M0[b:b + 1], dict(rb, scale=float(alone["sigma"][0])))
        assert _bits_equal(fixed["meff"], alone["meff"]) and _bits_equal(fixed["omega"], alone["omega"])
        assert math.isnan(float(fixed["sigma"][0])) and int(fixed["n"][0]) == -7          # a fixed scale: neither is written
    assert float(one["omega"].min()) < 0.5 and float(one["omega"].max()) == 1.0


def test_opcheck_and_the_operator_is_the_c_call(pkg):
    g = torch.Generator().manual_seed(5)
    B, H, W = 2, 12, 20
    pred, y = torch.rand(B, 4, H, W, generator=g).to(DEV), (torch.rand(B, 3, H, W, generator=g) * 2 - 1).to(DEV)
    mask = (torch.rand(B, 1, H, W, generator=g) > 0.2).float().to(DEV)

    def args(scale=0.0, loss="tukey", m=mask):
        return (pred, y, m, torch.empty(B, 3, H, W, device=DEV), torch.empty(B, 3, H, W, device=DEV), torch.full((B,), NAN, device=DEV),
                torch.zeros(B, device=DEV, dtype=torch.int32), 2.0, -1.0, loss, 4.685, scale, RO.SIGMA_MIN, False)
    a = args()
    assert torch.ops.osmosis.robust_mask(*a) is None
    want = run_kernels(pred.view(B, 4, H * W).cpu(), 2.0, -1.0, y.view(B, 3, H * W).cpu(),
                       mask.expand(B, 3, H, W).reshape(B, 3, H * W).cpu(), dict(loss="tukey", c=4.685))
    assert _bits_equal(a[3].cpu().view(B, 3, -1), want["meff"]) and _bits_equal(a[4].cpu().view(B, 3, -1), want["omega"])
    assert _bits_equal(a[5].cpu(), want["sigma"]) and torch.equal(a[6].cpu(), want["n"])
    with pytest.raises(Exception, match="loss"):
        torch.ops.osmosis.robust_mask(*args(loss="l1"))
    torch.library.opcheck(torch.ops.osmosis.robust_mask.default, args())
    torch.library.opcheck(torch.ops.osmosis.robust_mask.default, args(scale=0.05, loss="huber", m=None))


# ------------------------------------------------------------------------------------------------------------ 3: loss_grad_x0
def with_outliers(y, seed, frac=0.05):
    """`frac` of the pixels of y [B,3,h,w] replaced on all channels by white, U(0.8, 1.0)."""
    g = torch.Generator().manual_seed(seed)
    B, _, h, w = y.shape
    out = torch.rand(B, 1, h, w, generator=g) < frac
    return torch.where(out, 0.8 + 0.2 * torch.rand(B, 3, h, w, generator=g), y).contiguous(), out


# (operator, loss, weight, base mask, robust loss, per_pixel): the three operators, norm / mse, none / depth, mask on / off and the
# three losses cycled; B = 2 at 36 x 34 independent, B = 3 at 74 x 58 grouped [2, 1]
TERM = [("underwater_physical_revised", "norm", "depth", None, "tukey", False), ("haze_physical", "mse", "none", "uniform", "huber", False),
        ("underwater_physical", "norm", "none", "binary", "cauchy", True), ("underwater_physical_revised", "mse", "depth", "uniform", "cauchy", False),
        ("haze_physical", "norm", "depth", None, "huber", True), ("underwater_physical", "mse", "depth", None, "tukey", False)]
TERM_G = [("underwater_physical_revised", "norm", "depth", "uniform", "tukey", False), ("haze_physical", "norm", "none", None, "cauchy", False),
          ("underwater_physical", "mse", "depth", "binary", "huber", True)]


def term_errors(cond, g, sep, want_sep, want_phi, want_g, B):
    got_phi = {n: v.cpu() for n, v in cond.operator.variables().items()}
    e_loss = float((np.abs(sep.cpu().numpy().astype(np.float64) - want_sep) / np.abs(want_sep)).max())
    e_phi = max(float((got_phi[n].double() - want_phi[n].double()).abs().max()) for n in want_phi)
    e_g = max(float((g[b].cpu().double() - want_g[b]).abs().max()) / float(want_g[b].abs().max()) for b in range(B))
    return e_loss, e_phi, e_g


def run_term(pkg, case, B, H, W, groups, seed):
    opname, lf, lw, mkind, rloss, pp = case
    cond = gcond(pkg, opname, B, groups, "mean", "sgd", 5, AUX, lf, lw)
    x0, y = inputs(B, H, W, H, W, seed)
    y, _ = with_outliers(y, seed + 1)
    mask = None if mkind is None else make_masks(mkind, B, H, W, seed + 2)
    if mask is not None:
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    robust = dict(loss=rloss, per_pixel=pp)
    cond.set_robust(**robust)
    g, sep = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
    okw = dict(OPS[opname], **etas(OPS[opname], 1e-3))
    args = (groups or (1,) * B, opname, okw, x0.double(), y.double(), None if mask is None else mask.double(), 5, "sgd", AUX, lf, lw, "mean")
    want = RO.inner_loop(*args, robust)
    alt = RO.inner_loop(*args, robust, fp32_e=True)           # the oracle's own float64-versus-float32-e distance on this case
    own = (float((np.abs(alt[0] - want[0]) / np.abs(want[0])).max()),
           max(float((alt[1][n].double() - want[1][n].double()).abs().max()) for n in want[1]),
           max(float((alt[2][b] - want[2][b]).abs().max()) / float(want[2][b].abs().max()) for b in range(B)))
    return cond, g, sep, want, own


@pytest.mark.parametrize("case", TERM + TERM_G, ids=lambda c: "-".join(str(v) for v in c))
def test_loss_grad_x0_with_the_term_vs_the_masked_oracle_with_the_weights(pkg, case):
    """5 inner iterations; the masked kernels' bars (loss 3e-5 relative, phi 3e-6, gradient 3e-5 of its max), or where a case needs
    more 5 x the oracle's own float64-versus-float32-e distance on it (an entry whose u sits at a branch of omega moves with the
    rounding of e).  sigma and omega are held to the oracle's as well."""
    grouped = case in TERM_G
    B, H, W, groups = (3, 74, 58, (2, 1)) if grouped else (2, 36, 34, None)
    cond, g, sep, want, own = run_term(pkg, case, B, H, W, groups, 500 + 10 * (TERM + TERM_G).index(case))
    e_loss, e_phi, e_g = term_errors(cond, g, sep, *want[:3], B)
    bars = (max(3e-5, 5 * own[0]), max(3e-6, 5 * own[1]), max(3e-5, 5 * own[2]))
    vals = cond.robust_values()
    e_sig = float(np.abs(vals["scale"].cpu().numpy().astype(np.float64) / want[4] - 1).max())
    e_om = float((vals["weight"].cpu().double().view(B, 3, H, W) - want[3]).abs().max())
    print(f"ROBUSTTERM {case}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of its max; bars {bars}, the oracle's own f64-vs-f32-e "
          f"distance {own}; sigma(rel) {e_sig:.2e} omega {e_om:.2e}; mean omega {float(want[3].mean()):.3f}")
    assert e_loss <= bars[0] and e_phi <= bars[1] and e_g <= bars[2], (case, e_loss, e_phi, e_g, bars)
    assert e_sig <= 1e-5 and e_om <= 1e-4 and float(want[3].min()) < 0.9
    assert vals["n_valid"].dtype == torch.int32 and int(vals["n_valid"].min()) > 0


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("rloss", RO.LOSSES)
def test_ps_identity_term_with_the_weights(pkg, C, rloss):
    """loss[b] = ||M_eff (y - x0[0:3])|| and its gradient at the identity term's bars (loss 2e-6 relative, gradient 1e-5 of its max),
    M_eff from float64."""
    _, _, M, CM = pkg
    B, H, W = 2, 36, 34
    g_ = torch.Generator().manual_seed(40 + C)
    x0 = (0.6 * torch.randn(B, C, H, W, generator=g_)).clamp(-1, 1)
    y = (x0[:, 0:3] + 0.03 * torch.randn(B, 3, H, W, generator=g_)).contiguous()
    y, _ = with_outliers(y, 41)
    mask = make_masks("uniform", B, H, W, 42) if C == 4 else None
    cond = CM.get_conditioning_method("ps", M.get_operator("noise", device=DEV, batch_size=B), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    if mask is not None:
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    cond.set_robust(loss=rloss)
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    e = (y.double() - x0[:, 0:3].double()).numpy().reshape(B, 3, -1)
    meff, om, sigma = RO.mask64(e, None if mask is None else mask.double().numpy().reshape(B, 3, -1), rloss)
    r = torch.from_numpy(meff * e).view(B, 3, H, W)
    want_loss = torch.linalg.vector_norm(r, dim=(1, 2, 3))
    want_g = torch.zeros(B, C, H, W, dtype=torch.float64)
    want_g[:, 0:3] = -torch.from_numpy(meff).view(B, 3, H, W) * r / want_loss[:, None, None, None]
    e_loss = float(((loss.cpu().double() - want_loss).abs() / want_loss).max())
    e_g = max(float((g[b].cpu().double() - want_g[b]).abs().max()) / float(want_g[b].abs().max()) for b in range(B))
    print(f"ROBUSTPS C {C} {rloss}: loss(rel) {e_loss:.2e} grad {e_g:.2e} of its max; sigma {sigma}")
    assert e_loss <= 2e-6 and e_g <= 1e-5 and float(om.min()) < 0.5, (C, rloss, e_loss, e_g)


def _snapshot(cond, g, sep):
    return (g.cpu().clone(), sep.cpu().clone(), cond.operator.phi.cpu().clone(), None if cond._opt is None else cond._opt.cpu().clone())


@pytest.mark.parametrize("masked", [False, True], ids=["no_mask", "mask"])
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_omega_one_is_the_masked_run(pkg, masked, optimizer):
    """huber with c = 1e30: omega = 1 everywhere, so M_eff = M0 bit for bit -- phi, loss, g and the optimiser state are torch.equal to
    the masked run with M0, and with no base mask to the run with a mask of ones."""
    B, H, W = 2, 36, 34
    x0, y = inputs(B, H, W, H, W, 61)
    y, _ = with_outliers(y, 62)
    mask = make_masks("uniform", B, H, W, 63) if masked else torch.ones(B, 3, H, W)
    out = {}
    for tag in ("robust", "plain"):
        cond = gcond(pkg, "underwater_physical_revised", B, None, "mean", optimizer, 5, AUX, "norm", "depth")
        if masked or tag == "plain":
            cond.set_measurement_mask(mask, batch=B, device=DEV)
        if tag == "robust":
            cond.set_robust(loss="huber", c=1e30)
        out[tag] = _snapshot(cond, *cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False))
        if tag == "robust":
            assert bool((cond.robust_values()["weight"] == 1.0).all())
    for a, b in zip(out["robust"], out["plain"]):
        assert (a is None and b is None) or torch.equal(a, b)
    assert (out["robust"][3] is not None) == (optimizer == "adam")


@pytest.mark.parametrize("scale", ["mad", 0.05])
def test_py_loop_is_the_one_call(pkg, monkeypatch, scale):
    B, H, W = 2, 36, 34
    x0, y = inputs(B, H, W, H, W, 71)
    y, _ = with_outliers(y, 72)
    out = []
    for py in ("0", "1"):
        monkeypatch.setenv("OSM_PHYS_PY_LOOP", py)
        cond = gcond(pkg, "haze_physical", B, None, "mean", "sgd", 5, AUX, "mse", "depth")
        cond.set_robust(loss="cauchy", scale=scale)
        snap = _snapshot(cond, *cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False))
        v = cond.robust_values()
        out.append(snap[:3] + (v["weight"].cpu().clone(), v["scale"].cpu().clone(), v["n_valid"].cpu().clone()))
    assert all(torch.equal(a, b) for a, b in zip(*out))
    assert int(out[0][5][0]) == (0 if scale != "mad" else 3 * H * W)          # (a fixed scale counts nothing ...)
    assert scale == "mad" or float(out[0][4][0]) == float(np.float32(scale))       # (... and reports itself)


def test_all_zero_weights_hold_the_fully_masked_guard(pkg):
    """tukey at a fixed scale of 1e-6: every weight is 0.  Loss 0, phi and the optimiser state untouched, g the auxiliary terms alone
    -- what a mask of zeros gives, bit for bit."""
    B, H, W = 2, 36, 34
    x0, y = inputs(B, H, W, H, W, 81)
    out = {}
    for tag in ("robust", "zeros"):
        cond = gcond(pkg, "underwater_physical_revised", B, None, "mean", "adam", 5, AUX, "norm", "depth")
        phi0 = cond.operator.phi.cpu().clone()
        if tag == "robust":
            cond.set_robust(loss="tukey", scale=1e-6)
        else:
            cond.set_measurement_mask(torch.zeros(B, 3, H, W), batch=B, device=DEV)
        out[tag] = _snapshot(cond, *cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False))
        if tag == "robust":
            assert float(cond.robust_values()["weight"].max()) == 0.0
    g, sep, phi, opt = out["robust"]
    assert float(sep.abs().max()) == 0.0 and torch.equal(phi, phi0) and float(g[:, 3].abs().max()) == 0.0 and float(g[:, 0:3].abs().max()) > 0
    for a, b in zip(out["robust"], out["zeros"]):
        assert torch.equal(a, b)


def test_chunk_rows_write_their_rows_and_refusals(pkg):
    """`rows=` ranges of the open batch: a [2, 1] walk is the one pass bit for bit, `robust_values()` included; a range that is not
    the call's images, or that ends past the batch, raises before any launch; a degradation and a 'ps' grid operator are refused
    naming `robust`."""
    _, _, M, CM = pkg
    B, H, W = 3, 36, 34
    x0, y = inputs(B, H, W, H, W, 91)
    y, _ = with_outliers(y, 92)
    for masked in (False, True):
        runs = []
        for walk in ([(0, 3)], [(0, 2), (2, 3)]):
            cond = gcond(pkg, "underwater_physical_revised", B, None, n_iter=3)
            if masked:
                cond.set_measurement_mask(make_masks("uniform", B, H, W, 93), batch=B, device=DEV)
            cond.set_robust(loss="tukey")
            cond.open_batch(B, (H, W), (H, W), DEV)
            v = cond.robust_values()
            assert bool(torch.isnan(v["scale"]).all()) and int(v["n_valid"].abs().max()) == 0 and float(v["weight"].abs().max()) == 0.0
            gs = []
            for lo, hi in walk:
                g, _ = cond.loss_grad_x0(x0[lo:hi].to(DEV), y[lo:hi].to(DEV), rows=(lo, hi))
                gs.append(g.cpu().clone())
            v = cond.robust_values()
            runs.append((torch.cat(gs), cond.operator.phi.cpu().clone(), v["scale"].cpu().clone(), v["n_valid"].cpu().clone(),
                         v["weight"].cpu().clone()))
        assert all(torch.equal(a, b) for a, b in zip(*runs)), masked
        assert tuple(runs[1][2].shape) == (B,) and len(set(runs[1][2].tolist())) == B
    before = [t.clone() for t in cond.robust_values().values()]
    for bad in ((0, 3), (2, 4)):        # not this call's two images; past the batch's three: sigma + b would be written out of bounds
        with pytest.raises(ValueError, match="rows must be"):
            cond.loss_grad_x0(x0[0:2].to(DEV), y[0:2].to(DEV), rows=bad, mask=torch.ones(2, 3, H * W, device=DEV))
    assert all(torch.equal(a, b) for a, b in zip(before, cond.robust_values().values()))        # (nothing was launched)
    g, _ = cond.loss_grad_x0(x0[0:2].to(DEV), y[0:2].to(DEV), rows=(0, 2), mask=torch.ones(2, 3, H * W, device=DEV))
    assert bool(torch.isfinite(g).all())                  # any mask rows for exactly the call's images are legal: `rows` has the place
    from physlin_oracle import DEGRADATIONS
    deg = gcond(pkg, "underwater_physical_revised", 1, None, deg=DEGRADATIONS["gaussian_blur"])
    with pytest.raises(NotImplementedError, match="robust"):
        deg.set_robust(loss="tukey")
    deg._robust = dict(cond._robust)
    with pytest.raises(NotImplementedError, match="robust"):
        deg.loss_grad_x0(x0[0:1].to(DEV), y[0:1].to(DEV))


EFFECT_ETA = 1e-3                                     # tests/test_robust_cpu.py states why: at this step every fit reaches its fixed point
EFFECT_STEPS = {"tukey": 1200, "huber": 1700, "ls": 1700}      # ... and has settled by then (the CPU test asserts it)
_EFFECT = {}


def _effect_run(pkg, x0, y, rb, steps, sample_every=None):
    """`steps` sub-steps of `loss_grad_x0` on the device from PHI_START: phi at the end, and (sample_every) the smallest
    max |phi - phi*| among the samples taken along the way."""
    _, _, M, CM = pkg
    okw = dict(RO.PHI_START, depth_type="move", value="0.0", **{k + "_eta": EFFECT_ETA for k in RO.PHI_START})
    oper = M.get_operator(RO.OPNAME, device=DEV, batch_size=1, optimizer="sgd", **okw)
    cond = CM.get_conditioning_method("osmosis", oper, M.get_noise("clean"), loss_function="norm", loss_weight="none", scale="1",
                                      gradient_x_prev=True, gradient_clip="False,0", n_iter=20, aux_loss=None, pattern="pcgs")
    if rb is not None:
        cond.set_robust(**rb)
    xd, yd = x0.to(DEV).contiguous(), y.to(DEV).contiguous()
    phi_now = lambda: {n: v.cpu().double().reshape(-1) for n, v in cond.operator.variables().items()}     # noqa: E731
    best = float("inf")
    for k in range(steps):
        cond.loss_grad_x0(xd, yd, freeze_phi=False)
        if sample_every and (k + 1) % sample_every == 0:
            best = min(best, RO.phi_error(phi_now()))
    return phi_now(), best


@pytest.mark.parametrize("rloss", ["tukey", "huber"])
def test_effect_on_phi_under_outliers_reproduces_the_oracles(pkg, rloss):
    """tests/test_robust_cpu.py's setup through `loss_grad_x0` on the device (the fp32 image and photo, which the oracle is fed too):
    sub-steps of 20 sgd iterations from PHI_START at EFFECT_ETA, the image held at the truth, until the fit has settled (1200 sub-steps
    for tukey, 1700 for huber).  The trajectory ends within the phi bar (3e-6) of the oracle's, and it reproduces the oracle's ratio:
    the end is at most 0.5 x the SMALLEST error the device's own least-squares fit shows at any of its cuts (sampled every 20
    sub-steps), 0.2057.
    The oracle holds phi as the reference and `oracle.diffusion_ref.PhysOperator` hold it, in a float32 parameter tensor (float64
    arithmetic, phi rounded to float32 after every step).  An oracle that carries phi in float64 is no yardstick for a 3e-6 bar here,
    settled or not: the fit has a nearly flat direction (phi_b against phi_inf) along which the roundings of a float32 phi add up, and
    that oracle's OWN distance to its float32-phi twin on this setup is 2.6e-5 (huber, 1700 sub-steps) and 8.0e-6 (tukey, 1200) --
    max |phi - phi*| is the same to four digits either way (0.0374 / 0.0295)."""
    x0, y, _ = RO.effect_problem()
    x0, y = x0.float(), y.float()
    steps = EFFECT_STEPS[rloss]
    got, _ = _effect_run(pkg, x0, y, dict(loss=rloss), steps)
    want, _, _ = RO.effect_fit_closed_form(x0.double(), y.double(), dict(loss=rloss), steps=steps, eta=EFFECT_ETA, fp32_phi=True)
    if "ls" not in _EFFECT:
        _EFFECT["ls"] = _effect_run(pkg, x0, y, None, EFFECT_STEPS["ls"], sample_every=20)[1]
    ls = _EFFECT["ls"]
    dist = max(float((got[n] - want[n]).abs().max()) for n in want)
    print(f"ROBUSTEFFECT {rloss}: max |phi - phi*| {RO.phi_error(got):.4f} (oracle {RO.phi_error(want):.4f}), the device's least squares at "
          f"its best cut {ls:.4f}; distance to the oracle's end {dist:.2e} (bar 3e-6)")
    assert RO.phi_error(got) <= 0.5 * ls, (rloss, RO.phi_error(got), ls)
    assert dist <= 3e-6, (rloss, dist)


# ============================================================================================================ chain level
CH, CW = 16, 24
# (operator, robust, base mask, solver rule, groups, tiled, seed)
CHAINS = {"revised+tukey": ("underwater_physical_revised", dict(loss="tukey"), False, None, None, False, 601),
          "haze+huber+mask": ("haze_physical", dict(loss="huber"), True, None, None, False, 602),
          "revised+cauchy+dpmpp_2m": ("underwater_physical_revised", dict(loss="cauchy"), False, "dpmpp_2m", None, False, 603),
          "shared_water[2,1]+tukey": ("underwater_physical_revised", dict(loss="tukey", per_pixel=True), False, None, (2, 1), False, 604),
          "tiled24x36+tukey": ("underwater_physical_revised", dict(loss="tukey"), False, None, None, True, 605)}


def chain_inputs(B, C, seed, hw=(CH, CW), n=T):
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H, W, generator=g)
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, H, W, generator=g)
    mask = torch.rand(B, 3, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    y, _ = with_outliers(y, seed + 50)
    return x_T, y, noise, mask


def chain_cond(pkg, opname, B=1, groups=None):
    _, _, M, CM = pkg
    kw = {} if groups is None else dict(phi_groups=list(groups), phi_reduce="mean")
    operator = M.get_operator(opname, device=DEV, batch_size=B, **OPERATORS[opname], **kw)
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **PATTERN, aux_loss=AUX)


def _ref_setup():
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    return cfg, sd, tb


def oracle_chain(case, bump=None):
    """The oracle's loop with the term, group by group (an independent image is a group of one).  Returns (merged trace, inputs)."""
    import solver_oracle as SO
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from test_tiled_gpu import CANVAS, TILING, tiled_oracle_model
    opname, robust, masked, rule, groups, tiled, seed = CHAINS[case]
    cfg, sd, tb = _ref_setup()
    B = 1 if groups is None else sum(groups)
    x_T, y, noise, mask = chain_inputs(B, 4, seed, CANVAS if tiled else (CH, CW))
    mask = mask if masked else None
    x_in = x_T if bump is None else x_T + bump
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    net = lambda x, t: U.unet_forward(sd, cfg, x, t)  # noqa: E731
    if tiled:
        origins, wy, wx, inv = gd.tile_grid(*CANVAS, TILING["tile"], TILING["stride"], "hann")
        net = tiled_oracle_model(sd, cfg, origins, wy, wx, inv, *TILING["tile"])
    traces, lo = [], 0
    for n in (groups or (1,)):
        sl = slice(lo, lo + n)
        rg = RO.make_guidance(opname, dict(okw, depth_type="gamma", value="1.4,1.4,1"), None if mask is None else mask[sl], 20, AUX,
                              COND["loss_function"], COND["loss_weight"], robust, scale=COND["scale"], gradient_clip=COND["gradient_clip"])
        trace = []
        if rule is None:
            D.p_sample_loop(net, tb, x_in[sl], y[sl], rg, PATTERN, [noise[k][sl] for k in range(T)], trace)
        else:
            SO.osmosis_loop(net, tb, x_in[sl], y[sl], rg, PATTERN, [noise[k][sl] for k in range(T)], rule, 0.0, first=T - 1, trace=trace)
        traces.append(trace)
        lo += n
    merged = []
    for k in range(T):
        recs = [t[k] for t in traces]
        merged.append({"x_out": torch.cat([r["x_out"] for r in recs]), "x0": torch.cat([r["x0"] for r in recs]),
                       "loss": np.concatenate([np.asarray(r["loss"]).reshape(-1) for r in recs]),
                       "phi": {name: torch.cat([r["phi"][name] for r in recs]) for name in recs[0]["phi"]}})
    return merged, (x_T, y, noise, mask)


def fused_chain(pkg, monkeypatch, model, opname, x_T, y, noise, mask, robust, rule=None, groups=None, tiling=None, sizes=None, fused=True,
                pass_robust=True):
    _, gd, _, _ = pkg
    B = x_T.shape[0]
    sampler = make_sampler(gd) if rule is None else make_sampler(gd, solver=rule, solver_eta=0.0)
    if sizes is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: list(sizes)))
    cond = chain_cond(pkg, opname, B, groups)
    nd = noise.to(DEV)
    kw = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False, save_root=None,
              pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN, measurement_mask=mask)
    if pass_robust:
        kw["robust"] = robust
    if tiling is not None:
        kw["tiling"] = tiling
    trace = []
    if fused:
        _no_generic(monkeypatch, sampler)
        out = sampler.p_sample_loop(noise_fn=lambda k, shape: nd[k], trace=trace, **kw)
    else:
        cond.hip_ok = lambda: False             # the conditioner declines the fused loop; its step (the kernels) stays
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, PATTERN, tuple(x_T.shape)) is None
        _replay_randn_like(monkeypatch, nd, 4)
        out = sampler.p_sample_loop(**kw)
    monkeypatch.undo()
    return out, cond, trace


@pytest.mark.parametrize("case", list(CHAINS))
def test_fused_chain_with_the_term_vs_the_oracles_loop(pkg, monkeypatch, model48, case):
    """Free-running against the oracle's p_sample_loop with the term: final image and pred_xstart within 10 x the oracle's own drift
    under a 1e-6 perturbation of x_T (`_free_running_bar`, floor 2e-5), loss 20 x that, phi 2e-6 -- the chain protocol of the other
    suites.  The drift staying below 1e-3 is asserted: no case is skipped to teacher forcing."""
    from test_tiled_gpu import TILING
    opname, robust, masked, rule, groups, tiled, seed = CHAINS[case]
    ref, (x_T, y, noise, mask) = oracle_chain(case)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert, _ = oracle_chain(case, bump)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    assert bar is not None, (case, drift)
    out, cond, trace = fused_chain(pkg, monkeypatch, model48, opname, x_T, y, noise, mask, robust, rule, groups,
                                   dict(TILING, window="hann") if tiled else None)
    B = x_T.shape[0]
    a, b = trace[-1], ref[-1]
    e_img, e_x0 = float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max())
    want = np.asarray(b["loss"], dtype=np.float64).reshape(-1)
    e_loss = float((np.abs(a["loss"].cpu().numpy().reshape(-1) - want) / want).max())
    e_phi = max(float((a["phi"][:, off:off + n].cpu() - b["phi"][name].reshape(B, -1)[:, :n]).abs().max())
                for name, (off, n) in cond.operator._slots().items())
    v = cond.robust_values()
    print(f"ROBUSTCHAIN {case}: oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
          f"phi {e_phi:.2e}; sigma {v['scale'].tolist()} mean omega {float(v['weight'].mean()):.3f}")
    assert e_img < bar and e_x0 < bar and e_loss < 20.0 * bar and e_phi < 2e-6, (case, e_img, e_x0, e_loss, e_phi, bar)
    assert bool(torch.isfinite(v["scale"]).all()) and float(v["weight"].min()) < 1.0 and float(v["weight"].max()) <= 1.0


def test_chunks_one_tile_and_robust_none_bit_for_bit(pkg, monkeypatch, model48):
    """B = 3 walked as [2, 1] is the one pass, `robust_values()` included row by row; one tile covering the canvas is the untiled chain;
    `robust=None` is a call without the keyword."""
    op, rb = "underwater_physical_revised", dict(loss="tukey")
    x_T, y, noise, mask = chain_inputs(3, 4, 611)
    for m in (None, mask):
        whole, cw, _ = fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, m, rb, sizes=[3])
        chunked, cc, _ = fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, m, rb, sizes=[2, 1])
        _same_bits(chunked, whole, f"robust: one pass vs chunks of [2, 1] (mask {m is not None})")
        vw, vc = cw.robust_values(), cc.robust_values()
        for k in ("scale", "n_valid", "weight"):
            assert vc[k].shape[0] == 3 and torch.equal(vc[k], vw[k]), k
        assert len(set(vc["scale"].tolist())) == 3 and bool(torch.isfinite(vc["scale"]).all())
    free, c0, _ = fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, None, None, sizes=[3])
    assert not torch.equal(free[0], whole[0]) and c0.robust_values() is None                     # the term matters
    _same_bits(fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, None, None, sizes=[3], pass_robust=False)[0], free,
               "robust=None vs no keyword")
    x1, y1, n1, _ = chain_inputs(1, 4, 612)
    one = fused_chain(pkg, monkeypatch, model48, op, x1, y1, n1, None, rb)[0]
    tiled = fused_chain(pkg, monkeypatch, model48, op, x1, y1, n1, None, rb, tiling=dict(tile=(CH, CW), stride=(CH, CW), window="uniform"))[0]
    _same_bits(tiled, one, "robust: one 16 x 24 tile vs the untiled fused chain")


def test_fused_chain_with_the_term_equals_the_generic_loop(pkg, monkeypatch, model48):
    """Osmosis, B = 2 with a mask: both loops at tests/test_mask_gpu.py's fused-versus-generic bars (image and pred_xstart 1e-4, loss
    rtol 1e-5, phi 1e-6); the generic loop takes the kernels' step through `conditioning`."""
    op, rb = "underwater_physical_revised", dict(loss="tukey")
    x_T, y, noise, mask = chain_inputs(2, 4, 621)
    f, cf, _ = fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, mask, rb)
    g, cg, _ = fused_chain(pkg, monkeypatch, model48, op, x_T, y, noise, mask, rb, fused=False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"ROBUSTGENERIC: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6 and np.allclose(f[2], g[2], rtol=1e-5)
    assert torch.allclose(cf.robust_values()["scale"], cg.robust_values()["scale"], rtol=1e-4)


def test_torch_route_agrees_with_the_kernels(pkg):
    """`_loss_autograd` (what `_generic_loop` and foreign operators use) with the term: the same M_eff by torch.sort -- loss and
    sigma against `loss_grad_x0` on the same inputs (loss 3e-5 relative, the masked kernels' bar)."""
    B, H, W = 2, 36, 34
    x0, y = inputs(B, H, W, H, W, 631)
    y, _ = with_outliers(y, 632)
    cond = gcond(pkg, "underwater_physical_revised", B, None, "mean", "sgd", 5, None, "norm", "depth")
    cond.set_measurement_mask(make_masks("uniform", B, H, W, 633), batch=B, device=DEV)
    cond.set_robust(loss="cauchy", per_pixel=True)
    sep, _, _ = cond._loss_autograd(x0.to(DEV), y.to(DEV))
    vt = {k: v.cpu().clone() for k, v in cond.robust_values().items()}
    _, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=True)
    vk = cond.robust_values()
    assert np.allclose(sep, loss.cpu().numpy(), rtol=3e-5)
    assert torch.allclose(vt["scale"], vk["scale"].cpu(), rtol=1e-6) and torch.equal(vt["n_valid"], vk["n_valid"].cpu())
    assert float((vt["weight"] - vk["weight"].cpu()).abs().max()) < 1e-5


# ------------------------------------------------------------------------------------------------------------ the driver
def driver_cfg(robust=None):
    op_cfg = dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised")
    cfg = {"measurement": {"operator": op_cfg, "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    if robust is not None:
        cfg["measurement"]["robust"] = robust
    return cfg


def test_restore_image_with_the_term(pkg, monkeypatch, model48, tmp_path):
    """`restore_image` on the 3-index low-noise sub-chain: `robust_weight` in [0, 1] with the photo's shape, `robust_scale` finite and
    >= sigma_min, `_robust.png` written; the argument wins over the config; without the key no result key and no file; chunked
    batches give every image its own."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    photo = (torch.rand(1, 3, 256, 256, generator=torch.Generator().manual_seed(701)) * 1.2 - 0.6)
    photo, _ = with_outliers(photo, 702)
    photo = photo.to(DEV)
    sub = dict(index_range=(2, 0), x_scale=0.05, noise_seed=7)
    res = sampling.restore_image(model48, photo, driver_cfg(dict(loss="tukey")), **sub)[-1]
    w, s = res["robust_weight"], res["robust_scale"]
    assert tuple(w.shape) == (3, 256, 256) and float(w.min()) >= 0.0 and float(w.max()) <= 1.0 and float(w.min()) < 1.0
    assert math.isfinite(s) and s >= float(np.float32(RO.SIGMA_MIN))
    paths = sampling.save_outputs(res, photo, str(tmp_path), "photo")
    assert paths["robust"].endswith("photo_robust.png") and os.path.getsize(paths["robust"]) > 0
    by_arg = sampling.restore_image(model48, photo, driver_cfg(dict(loss="huber")), robust=dict(loss="tukey"), **sub)[-1]
    assert torch.equal(by_arg["sample"], res["sample"]) and torch.equal(by_arg["robust_weight"], w)
    free = sampling.restore_image(model48, photo, driver_cfg(), **sub)[-1]
    assert "robust_weight" not in free and "robust_scale" not in free and not torch.equal(free["sample"], res["sample"])
    assert "robust" not in sampling.save_outputs(free, photo, str(tmp_path / "free"), "photo")
    with pytest.raises(ValueError, match="unknown key"):
        sampling.restore_image(model48, photo, driver_cfg(dict(loss="tukey", k=4.0)), **sub)
    photos = [photo.cpu(), photo.cpu().flip(-1).contiguous()]
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: [1] * B_))
    two = sampling.restore_images(model48, photos, driver_cfg(), device=DEV, batch_size=2, robust=dict(loss="tukey"), **sub)
    assert all(tuple(two[i]["robust_weight"].shape) == (3, 256, 256) and math.isfinite(two[i]["robust_scale"]) for i in (0, 1))
    assert not torch.equal(two[0]["robust_weight"], two[1]["robust_weight"])
    assert abs(two[0]["robust_scale"] - s) <= 1e-4 * s


def test_ps_chain_with_the_term_fused_vs_the_generic_loop(pkg, monkeypatch, model36):
    """`ps` 3 -> 6 with the term: fused against `_generic_loop`, whose step is pure autograd (`grad_and_value`, the torch route's
    M_eff) over the HIP UNet.  Bar: the one tests/test_mask_gpu.py holds its masked `ps` chain to on this network,
    min(5 x measured, 10 x drift_1e-6) of the unmasked pair."""
    from test_mask_gpu import GOLD, MEASURED_RGB
    _, gd, M, CM = pkg
    gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
    bar = min(5.0 * MEASURED_RGB["rg.ddpm.c36"], 10.0 * float(gold["rg.ddpm.c36.drift_1e-6"]))
    x_T, y, noise, mask = chain_inputs(1, 3, 641)
    noise = noise.to(DEV)
    sampler = make_sampler(gd, "ddpm")

    def make_cond():
        return CM.PosteriorSampling(M.get_operator("noise", device=DEV, batch_size=1), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    kw = dict(model=model36, x_start=x_T.to(DEV), measurement=y.to(DEV), record=False, save_root=None, pretrain_model="imagenet",
              rgb_guidance=True, sample_pattern=PATTERN, measurement_mask=mask)
    _no_generic(monkeypatch, sampler)
    cf = make_cond()
    f = sampler.p_sample_loop(measurement_cond_fn=cf.conditioning, noise_fn=lambda k, shape: noise[k], robust=dict(loss="huber"), **kw)
    plain = sampler.p_sample_loop(measurement_cond_fn=make_cond().conditioning, noise_fn=lambda k, shape: noise[k], **kw)
    monkeypatch.undo()
    monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cg = make_cond()
    assert sampler._fast_path_ok(model36, cg.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is None
    _replay_randn_like(monkeypatch, noise, 3)
    g = sampler.p_sample_loop(measurement_cond_fn=cg.conditioning, robust=dict(loss="huber"), **kw)
    monkeypatch.undo()
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    print(f"ROBUSTPSCHAIN: fused vs generic {e:.3e} (bar {bar:.3e}); with vs without the term {float((f - plain).abs().max()):.2e}")
    assert bool(torch.isfinite(f).all()) and e <= bar and not torch.equal(f, plain)
    assert torch.allclose(cf.robust_values()["scale"], cg.robust_values()["scale"], rtol=1e-4)
