"""Blind deblurring on the GPU (operator `blind_blur`, include/osmosis_blind.h): the tap-gradient kernel and the projected step
against the float64 oracle of tests/blind_oracle.py, the data term `loss_grad_x0` with its inner loop, the recovery of a known kernel
when the image is known, the fused sampler loop against `_generic_loop` and against the oracle's chain, and `restore_image`.

Tap-gradient bar (derived from the header's order, not tuned): part[b][q][t] is an fp32 chain of one fma per pixel of a tile, at
most N = min(32, H) min(32, W) long; the partials are then added in fp64.  So per tap |err| <= (N + 2) 2^-24 sum |r| |x| (the + 2:
the (1 + u)^n - 1 <= n u / (1 - n u) slack, as tests/test_psf_gpu.py has it).  Worst |err| / bound measured: see the README.

Kernel-estimate bar: 5 x the distance between the float64 oracle and the SAME oracle with its image side (A, loss, r, c) in float32
on the CPU -- the definition's own sensitivity to fp32 arithmetic.  Both numbers are printed and recorded in the README."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import blind_oracle as BO
from oracle import diffusion_ref as D
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U24 = 2.0 ** -24
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")
H0, W0 = 16, 24
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)
# tests/test_rgb_gpu.py MEASURED of the identity 'ps' chains, as tests/test_psf_gpu.py copies them (the fused-vs-generic bar:
# min(5 x measured, 10 x the recorded drift_1e-6 of tests/golden/loop_rgb.npz))
MEASURED_RGB = {"rg.ddpm.c36": 5.960e-07, "rg.ddim.c36": 7.153e-07, "rg.ddpm.c36.m2": 1.162e-06}


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


# ------------------------------------------------------------------------------------------------------------ 1: the tap gradient
def _sparse15():
    from osmosis_diffusion_code_amd.guided_diffusion.measurements import motion_kernel
    iy, ix = np.nonzero(motion_kernel(15, 0.5, 7))
    return (iy - 7).astype(np.int32), (ix - 7).astype(np.int32), 15, 15


def _dense(kh, kw):
    dy, dx = np.repeat(np.arange(kh) - kh // 2, kw).astype(np.int32), np.tile(np.arange(kw) - kw // 2, kh).astype(np.int32)
    return dy, dx, kh, kw


# case -> (H, W, taps)
TAP_CASES = {"tiles9": (36, 34, lambda: _dense(9, 9)),           # two tiles per axis, ragged tails
             "asym3x7": (20, 27, lambda: _dense(3, 7)),
             "both_mirrors": (8, 6, lambda: _dense(5, 5)),       # smaller than a tile, both mirrors reach
             "wide9": (40, 72, lambda: _dense(9, 9)),
             "dense61": (64, 64, lambda: _dense(61, 61)),        # the LDS-capacity case, T = 3721 > 256 lanes
             "sparse15": (36, 34, _sparse15)}                    # a list that is not dense
_TAPREF = {}


def tap_reference(case):
    """Inputs and the float64 c of a case, once: x [2,4,H,W], r [2,3,H,W]; c and the magnitude sum |r| |x| per tap."""
    if case not in _TAPREF:
        H, W, taps = TAP_CASES[case]
        dy, dx, kh, kw = taps()
        g = torch.Generator().manual_seed(17)
        x, r = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
        x64, r64 = x[:, 0:3].double(), r.double()
        sel = (torch.from_numpy(dy.astype(np.int64)) + kh // 2) * kw + torch.from_numpy(dx.astype(np.int64)) + kw // 2
        c = BO.tap_corr(r64, x64, kh, kw).reshape(2, -1)[:, sel]
        mag = BO.tap_corr(r64.abs(), x64.abs(), kh, kw).reshape(2, -1)[:, sel]
        _TAPREF[case] = dict(H=H, W=W, dy=dy, dx=dx, R=(kh // 2, kw // 2), x=x, r=r, c=c, mag=mag)
    return _TAPREF[case]


def run_tap_grad(ref, x, r, B=None):
    """osm_psf_tap_grad into a NaN-filled workspace -> part [B, nparts, T] (device)."""
    from osmosis_diffusion_code_amd import ops
    B = x.shape[0] if B is None else B
    C, H, W = x.shape[1], ref["H"], ref["W"]
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    nparts = ops.tap_grad_nparts(3, H, W)
    part = torch.full((B, nparts, dy.numel()), float("nan"), device=DEV)
    ops.psf_tap_grad(x, r, dy, dx, *ref["R"], B, 3, C * H * W, 3 * H * W, H, W, part)
    return part


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", list(TAP_CASES))
def test_tap_gradient_vs_float64_under_the_derived_bound(pkg, case, C):
    ref = tap_reference(case)
    H, W = ref["H"], ref["W"]
    x, r = ref["x"][:, 0:C].contiguous().to(DEV), ref["r"].to(DEV)
    part = run_tap_grad(ref, x, r)
    assert bool(torch.isfinite(part).all()), "a partial was not written"
    c = part.double().sum(dim=1).cpu()
    N = min(32, H) * min(32, W)
    bound = (N + 2) * U24 * ref["mag"]
    ratio = float(((c - ref["c"]).abs() / bound.clamp_min(1e-300)).max())
    print(f"BLINDTAP {case} C={C}: worst |err| / bound {ratio:.3f} (max |err| {float((c - ref['c']).abs().max()):.2e}, T {c.shape[1]})")
    assert ratio <= 1.0, (case, ratio)
    # a repeat, and the batch as two calls of one image: the same bits
    assert torch.equal(run_tap_grad(ref, x, r), part)
    for b in range(2):
        assert torch.equal(run_tap_grad(ref, x[b:b + 1].contiguous(), r[b:b + 1].contiguous())[0], part[b])


@pytest.mark.parametrize("case", list(TAP_CASES))
def test_tap_gradient_is_exact_on_small_integers(pkg, case):
    """The derived bound is a worst case (about 0.5 absolute per tap at 64 x 64), under which one mis-reflected pixel could hide.
    With x and r integers in [-3, 3] every product and every partial sum of a tile (at most 1024 x 9 < 2^24) is exact in fp32
    whatever the order, so each PARTIAL must equal the float64 sum over its tile bit for bit: a single wrong pixel shows."""
    ref = tap_reference(case)
    H, W = ref["H"], ref["W"]
    g = torch.Generator().manual_seed(23)
    x = torch.randint(-3, 4, (2, 4, H, W), generator=g).float()
    r = torch.randint(-3, 4, (2, 3, H, W), generator=g).float()
    part = run_tap_grad(ref, x.to(DEV), r.to(DEV)).cpu().double()
    kh, kw = 2 * ref["R"][0] + 1, 2 * ref["R"][1] + 1
    sel = (torch.from_numpy(ref["dy"].astype(np.int64)) + kh // 2) * kw + torch.from_numpy(ref["dx"].astype(np.int64)) + kw // 2
    nty, ntx = -(-H // 32), -(-W // 32)
    for p in range(3):
        for ty in range(nty):
            for tx in range(ntx):
                rt = torch.zeros(2, 1, H, W, dtype=torch.float64)
                rt[:, 0, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = r[:, p, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32].double()
                want = BO.tap_corr(rt, x[:, p:p + 1].double(), kh, kw).reshape(2, -1)[:, sel]
                assert torch.equal(part[:, p * nty * ntx + ty * ntx + tx], want), (case, p, ty, tx)


@pytest.mark.parametrize("case", ["tiles9", "both_mirrors", "sparse15"])
def test_linearity_identity_against_psf_apply(pkg, case):
    """<r, A(w) x> = sum_t w[t] c[t], both sides from the kernels, within the two derived bounds."""
    from osmosis_diffusion_code_amd import ops
    ref = tap_reference(case)
    H, W, T = ref["H"], ref["W"], len(ref["dy"])
    x, r = ref["x"].to(DEV), ref["r"].to(DEV)
    w = torch.rand(T, generator=torch.Generator().manual_seed(3)) - 0.3
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    Ax = torch.empty(2, 3, H, W, device=DEV)
    ops.psf_apply(x, Ax, dy, dx, w.to(DEV), *ref["R"], 2, 3, 4 * H * W, 3 * H * W, H, W)
    lhs = (ref["r"].double() * Ax.cpu().double()).sum(dim=(1, 2, 3))
    c = run_tap_grad(ref, x, r).double().sum(dim=1).cpu()
    rhs = c @ w.double()
    N = min(32, H) * min(32, W)
    mag = ref["mag"] @ w.double().abs()                                  # sum |r| |w| |x|
    bound = ((T + 2) + (N + 2)) * U24 * mag
    print(f"BLINDTAP identity {case}: |lhs - rhs| / bound {float(((lhs - rhs).abs() / bound).max()):.3f}")
    assert bool(((lhs - rhs).abs() <= bound).all())


def test_a_tap_beyond_the_radius_is_skipped_and_bad_arguments_launch_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    ref = dict(tap_reference("tiles9"))
    x, r = ref["x"].to(DEV), ref["r"].to(DEV)
    full = run_tap_grad(ref, x, r)
    ref["R"] = (4, 2)                                                    # the list's |dx| reaches 4
    cut = run_tap_grad(ref, x, r)
    out = torch.from_numpy(np.abs(ref["dx"]) > 2)
    assert float(cut[:, :, out].abs().max()) == 0.0 and not bool(torch.signbit(cut[:, :, out]).any())
    assert torch.equal(cut[:, :, ~out], full[:, :, ~out])
    H, W = ref["H"], ref["W"]
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    part = torch.full((2, 12, 81), float("nan"), device=DEV)
    lib, p = _lib.load(), _lib.ptr
    good = [p(x), p(r), p(dy), p(dx), 81, 4, 4, 2, 3, 4 * H * W, 3 * H * W, H, W, p(part), None]
    for pos, val in ((0, None), (13, None), (4, 0), (5, 33), (5, H), (6, W), (9, 10), (10, 10)):
        args = list(good)
        args[pos] = val
        assert lib.osm_psf_tap_grad(*args) != 0 and lib.osm_last_error().decode().startswith("osm_psf_tap_grad")
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all())
    with pytest.raises(_lib.OsmosisHipError, match="smaller"):
        ops.psf_tap_grad(x, r, dy, dx, 4, 4, 3, 3, 4 * H * W, 3 * H * W, H, W, part)
    assert lib.osm_psf_tap_grad(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(part, full)


# ------------------------------------------------------------------------------------------------------------ 2: the step
def _step_case(T, B, nparts, seed):
    rng = np.random.default_rng(seed)
    w = rng.random(T).astype(np.float32)
    w /= w.sum()
    part = rng.standard_normal((B, nparts, T)).astype(np.float32)
    loss = (rng.random(B) + 0.5).astype(np.float32)
    return w, part, loss


def _c_of(part):
    c = np.zeros((part.shape[0], part.shape[2]))
    for q in range(part.shape[1]):                                       # ascending, as the header states
        c = c + part[:, q].astype(np.float64)
    return c


def run_step(w, part, loss, hw3, eta, l1):
    from osmosis_diffusion_code_amd import ops
    wd = torch.from_numpy(w.copy()).to(DEV)
    ops.psf_tap_step(wd, torch.from_numpy(part).to(DEV), torch.from_numpy(loss).to(DEV), part.shape[0], part.shape[1], hw3, eta, l1)
    return wd.cpu().numpy()


@pytest.mark.parametrize("T,B,nparts", [(25, 2, 3), (81, 1, 12), (3721, 2, 12), (4225, 1, 3), (1024, 3, 7)])
def test_step_vs_the_numpy_step(pkg, T, B, nparts):
    """At most 1 fp32 ulp per tap (the final division's rounding), exact where u = 0; l1 > 0 so that some taps clamp."""
    w, part, loss = _step_case(T, B, nparts, T)
    hw3 = 3 * 36 * 34
    eta = 40.0                                                           # large enough for the step to reach the clamp
    l1 = 0.05 / T
    want, u, S = BO.step(w, _c_of(part), loss, hw3, eta, l1)
    got = run_step(w, part, loss, hw3, eta, l1)
    assert S > 0 and (u == 0).any() and (u > 0).any() and not np.array_equal(want, w)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-30))).astype(np.float64)
    print(f"BLINDSTEP T={T} B={B}: worst {ulps.max():.2f} ulp, {int((u == 0).sum())} of {T} taps clamped, sum {got.astype(np.float64).sum():.9f}")
    assert ulps.max() <= 1.0
    assert np.all(got[u == 0] == 0.0)
    assert abs(float(got.astype(np.float64).sum()) - 1.0) <= 1e-6 and (got >= 0).all()


def test_step_guards_leave_the_estimate_untouched(pkg):
    w, part, loss = _step_case(81, 2, 12, 5)
    hw3 = 3 * 36 * 34
    assert np.array_equal(run_step(w, part, loss, hw3, 0.1, 1e9), w)                    # every u clamped to 0
    bad = loss.copy()
    bad[1] = np.nan
    assert np.array_equal(run_step(w, part, bad, hw3, 0.1, 0.0), w)
    bad[1] = np.inf
    assert np.array_equal(run_step(w, part, bad, hw3, 0.1, 0.0), w)
    pbad = part.copy()
    pbad[0, 3, 7] = np.nan
    assert np.array_equal(run_step(w, pbad, loss, hw3, 0.1, 0.0), w)
    assert not np.array_equal(run_step(w, part, loss, hw3, 0.1, 0.0), w)                # (and a good step moves it)


# ------------------------------------------------------------------------------------------------------------ 3: the data term
def blind_cond(pkg, B=1, third_party=False, **okw):
    _, _, M, CM = pkg
    kw = dict(kernel_size=9, n_iter=3, eta=0.5, init_sigma=1.5)
    kw.update(okw)
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    return cls(M.get_operator("blind_blur", device=DEV, batch_size=B, **kw), M.get_noise("gaussian", sigma=0.0), scale="0.3")


def term_inputs(B, C, H, W, masked, seed=21):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    mask = None
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g)
        mask[1] = (torch.rand(1, 1, H, W, generator=g) > 0.4).float()
    return x0, y, mask


def kernel_bar(x0, y, mask, w0, k, n_iter, eta, l1=0.0):
    """(float64 oracle result, 5 x its distance to the float32 evaluation of the same oracle, that distance)."""
    r64 = BO.inner_loop(x0, y, mask, w0, k, k, n_iter, eta, l1)
    r32 = BO.inner_loop(x0, y, mask, w0, k, k, n_iter, eta, l1, dtype=torch.float32)
    d = float(np.abs(r64["w"].astype(np.float64) - r32["w"].astype(np.float64)).max())
    return r64, 5.0 * d, d


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
def test_data_term_with_three_inner_iterations_vs_the_oracle(pkg, monkeypatch, masked, C):
    """B = 2 at 36 x 34, k = 9, n_iter = 3: loss (2e-6 relative) and x0-gradient (2e-7 + 1e-5 max |want|) at the identity term's bars
    of tests/test_psf_gpu.py, the kernel after three steps under `kernel_bar`; the C call against the single launches, a repeat from
    reset(), and `learn: False` against psf_blur with the init kernel, bit for bit."""
    _, _, M, CM = pkg
    B, H, W = 2, 36, 34
    x0, y, mask = term_inputs(B, C, H, W, masked)
    cond = blind_cond(pkg, B)
    op = cond.operator
    if masked:
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    w0 = op.host_taps()[2]
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g, loss, w = g.clone(), loss.clone(), op.taps(DEV)[2].clone()
    ref, bar, d = kernel_bar(x0, y, mask, w0, 9, 3, 0.5)
    for b in range(B):
        el = abs(float(loss[b]) - float(ref["loss"][b])) / float(ref["loss"][b])
        eg = float((g[b, 0:3].cpu().double() - ref["g"][b, 0:3]).abs().max())
        assert el <= 2e-6 and eg <= 2e-7 + 1e-5 * float(ref["g"][b, 0:3].abs().max()), (b, el, eg)
    if C == 4:
        assert float(g[:, 3].abs().max()) == 0.0
    ew = float(np.abs(w.cpu().numpy().astype(np.float64) - ref["w"].astype(np.float64)).max())
    moved = float(np.abs(ref["w"] - w0).max())
    print(f"BLINDTERM masked={masked} C={C}: kernel vs float64 oracle {ew:.3e}; oracle float64 vs float32 {d:.3e} (bar {bar:.3e}); moved {moved:.2e}")
    assert moved > 1e-4 and ew <= bar
    assert np.array_equal(op.kernel2d().reshape(-1), w.cpu().numpy().astype(np.float64))
    # a repeat from reset(): the same bits, in the same tensors
    live = op.taps(DEV)[2]
    op.reset()
    assert np.array_equal(live.cpu().numpy(), w0)
    g2, loss2 = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    assert op.taps(DEV)[2] is live and torch.equal(g2, g) and torch.equal(loss2, loss) and torch.equal(live, w)
    # the single launches
    op.reset()
    monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1")
    g3, loss3 = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    monkeypatch.undo()
    assert torch.equal(g3, g) and torch.equal(loss3, loss) and torch.equal(live, w)
    # learn: False is psf_blur with the init kernel
    fixed = blind_cond(pkg, B, learn=False)
    plain = CM.PosteriorSampling(M.get_operator("psf_blur", device=DEV, kernel=M.blind_init_kernel(9, "gaussian", 1.5), normalize=False),
                                 M.get_noise("gaussian", sigma=0.0), scale="0.3")
    for c in (fixed, plain):
        if masked:
            c.set_measurement_mask(mask, batch=B, device=DEV)
    gf, lf = fixed.loss_grad_x0(x0.to(DEV), y.to(DEV))
    gp, lp = plain.loss_grad_x0(x0.to(DEV), y.to(DEV))
    assert torch.equal(gf, gp) and torch.equal(lf, lp)
    assert np.array_equal(fixed.operator.kernel2d(), M.blind_init_kernel(9, "gaussian", 1.5))


def test_a_fully_masked_member_changes_nothing_in_the_kernel(pkg):
    B, H, W = 3, 36, 34
    x0, y, mask = term_inputs(B, 3, H, W, True)
    mask[2] = 0.0
    three, two = blind_cond(pkg, 3), blind_cond(pkg, 2)
    three.set_measurement_mask(mask, batch=3, device=DEV)
    two.set_measurement_mask(mask[:2], batch=2, device=DEV)
    g3, l3 = three.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g2, l2 = two.loss_grad_x0(x0[:2].to(DEV), y[:2].to(DEV))
    assert torch.equal(three.operator.taps(DEV)[2], two.operator.taps(DEV)[2])
    assert torch.equal(g3[:2], g2) and torch.equal(l3[:2], l2) and float(l3[2]) == 0.0 and float(g3[2].abs().max()) == 0.0


def test_opcheck_of_ps_blind_loss_grad(pkg):
    x0, y, mask = term_inputs(2, 4, 20, 27, True)
    cond = blind_cond(pkg, 2, kernel_size=5, n_iter=2)
    dy, dx, w = cond.operator.taps(DEV)
    args = (x0.to(DEV), y.to(DEV), mask.to(DEV), dy, dx, w.clone(), 2, 2, 2, 0.5, 0.0)
    torch.library.opcheck(torch.ops.osmosis.ps_blind_loss_grad.default, args)
    torch.library.opcheck(torch.ops.osmosis.ps_blind_loss_grad.default, args[:2] + (None,) + args[3:])
    wl = w.clone()
    loss, g = torch.ops.osmosis.ps_blind_loss_grad(x0.to(DEV), y.to(DEV), mask.to(DEV), dy, dx, wl, 2, 2, 2, 0.5, 0.0)
    cond.set_measurement_mask(mask, batch=2, device=DEV)
    g2, loss2 = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    assert torch.equal(g, g2) and torch.equal(loss, loss2) and torch.equal(wl, w) and not torch.equal(wl, torch.from_numpy(cond.operator.host_taps()[2]).to(DEV))


def test_kernel2d_reads_the_stepped_weights_of_an_operator_built_on_an_index_less_device(pkg):
    """`get_operator(device="cuda")` (what the reference driver passes): the data term steps the weights made for the tensors'
    device, cuda:0, and `kernel2d()` / `reset()` must find them there."""
    _, _, M, CM = pkg
    x0, y, _ = term_inputs(2, 3, 36, 34, False)
    ref = blind_cond(pkg, 2)
    ref.loss_grad_x0(x0.to(DEV), y.to(DEV))
    for device in ("cuda", torch.device("cuda")):
        op = M.get_operator("blind_blur", device=device, batch_size=2, kernel_size=9, n_iter=3, eta=0.5, init_sigma=1.5)
        init = op.kernel2d()
        cond = CM.PosteriorSampling(op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
        cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
        assert float(np.abs(op.kernel2d() - init).max()) > 1e-4 and np.array_equal(op.kernel2d(), ref.operator.kernel2d())
        assert np.array_equal(op.reset().kernel2d(), init)


# ------------------------------------------------------------------------------------------------------------ 4: recovery
def test_recovery_of_a_motion_kernel_when_the_image_is_known(pkg):
    """The convex problem of tests/test_blind_cpu.py on the GPU: final loss <= 0.25 x the first, final l1 distance to the true kernel
    <= 0.5 x the init's, and the final weights against the float64 oracle's under `kernel_bar`."""
    x, y, kstar, w0 = BO.recovery_problem()
    one = blind_cond(pkg, 1, kernel_size=7, n_iter=1, eta=1.0)
    _, first = one.loss_grad_x0(x.float().to(DEV), y.float().to(DEV))
    first = float(first[0])
    cond = blind_cond(pkg, 1, kernel_size=7, n_iter=200, eta=1.0)
    cond.loss_grad_x0(x.float().to(DEV), y.float().to(DEV))
    w = cond.operator.kernel2d()
    probe = blind_cond(pkg, 1, kernel_size=7, init=w, learn=False)       # the loss AT the final weights
    final = float(probe.loss_grad_x0(x.float().to(DEV), y.float().to(DEV))[1][0])
    d0, d1 = np.abs(w0.astype(np.float64) - kstar.reshape(-1)).sum(), np.abs(w - kstar).sum()
    ref, bar, d = kernel_bar(x.float(), y.float(), None, w0, 7, 200, 1.0)
    ew = float(np.abs(w.reshape(-1) - ref["w"].astype(np.float64)).max())
    print(f"BLINDRECOVERY gpu: loss {first:.3f} -> {final:.3f} ({final / first:.3f}), l1 distance {d0:.3f} -> {d1:.3f}; "
          f"kernel vs float64 oracle {ew:.3e}; oracle float64 vs float32 {d:.3e} (bar {bar:.3e})")
    assert final <= 0.25 * first and d1 <= 0.5 * d0
    assert ew <= bar


# ------------------------------------------------------------------------------------------------------------ 5: the chains
def make_model(unet, kw):
    cfg = U.UNetConfig.from_create_model_kwargs(**kw)
    m = unet.create_model(**kw)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    m.conv_mode = "f32"
    return m


@pytest.fixture(scope="module")
def model36(pkg):
    return make_model(pkg[0], RGB_KW)


@pytest.fixture(scope="module")
def model48(pkg):
    return make_model(pkg[0], TINY_KW)


def make_sampler(gd, name="ddpm", **kw):
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    args.update(kw)
    return gd.get_sampler(name)(**args)


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _replay_p_sample_draws(monkeypatch, noise):
    state, orig = {"k": 0}, torch.randn_like

    def replay(t, **kw):
        k = state["k"]
        state["k"] += 1
        return noise[k // 2].clone() if k % 2 == 0 else orig(t, **kw)
    monkeypatch.setattr(torch, "randn_like", replay)


CHAIN_OKW = dict(kernel_size=5, n_iter=2, eta=0.5, init_sigma=1.0)


def chain_inputs(B, C, n, seed=31):
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H0, W0, generator=g)
    y = torch.rand(B, 3, H0, W0, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, H0, W0, generator=g)
    mask = torch.rand(B, 3, H0, W0, generator=g) * (torch.rand(B, 1, H0, W0, generator=g) > 0.3).float()
    mask[:, :, 4:9, 6:13] = 0.0
    return x_T, y, noise, mask


_ORACLE = {}


def oracle_chain():
    """The oracle's DDPM chain on the tiny 3 -> 6 network (once): the final image and kernel, its drift under a 1e-6 perturbation
    of x_T, and the kernel's distance to the same chain with the data term's image side in float32."""
    if not _ORACLE:
        cfg = U.UNetConfig.from_create_model_kwargs(**RGB_KW)
        sd = U.seeded_state_dict(cfg, 1234)
        tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
        x_T, y, noise, _ = chain_inputs(1, 3, 10)
        from osmosis_diffusion_code_amd.guided_diffusion.measurements import blind_init_kernel
        w0 = blind_init_kernel(5, "gaussian", 1.0).reshape(-1).astype(np.float32)

        def net(x, t):
            return U.unet_forward(sd, cfg, x, t)

        def run(x_start):
            return BO.ps_chain(net, tb, x_start, y, list(noise), w0, 5, 5, 2, 0.5, 0.0, 0.3)
        img, w = run(x_T)
        bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
        pimg, pw = run(x_T + bump)
        # the chain's data term evaluated in float32: teacher-forced on the float64 chain's pred_xstart is not needed -- the whole
        # chain is re-run with `inner_loop(dtype=float32)`
        orig = BO.inner_loop
        try:
            BO.inner_loop = lambda *a, **k: orig(*a, **dict(k, dtype=torch.float32))
            _, w32 = run(x_T)
        finally:
            BO.inner_loop = orig
        _ORACLE.update(img=img, w=w, w0=w0, tb=tb, drift=float((pimg - img).abs().max()),
                       d_kernel=float(np.abs(w.astype(np.float64) - w32.astype(np.float64)).max()),
                       d_kernel_drift=float(np.abs(w.astype(np.float64) - pw.astype(np.float64)).max()))
    return _ORACLE


def _free_running_bar(drift):
    """tests/test_physgroup_gpu.py's rule: 10 x the oracle's own drift under a 1e-6 perturbation of x_T, floor 2e-5."""
    assert drift <= 1e-4, drift
    return max(2e-5, 10.0 * drift)


# case -> (sampler, sampler kwargs, pattern changes, network, masked, the tests/test_rgb_gpu.py chain whose bar applies)
CHAIN_CASES = {"ddpm": ("ddpm", {}, {}, "c36", False, "rg.ddpm.c36"),
               "ddim.clip": ("ddim", dict(clip_denoised=True), {}, "c36", False, "rg.ddim.c36"),
               "m2": ("ddpm", {}, dict(local_M=2, s_start=0.5, s_end=0.0), "c36", False, "rg.ddpm.c36.m2"),
               "masked": ("ddpm", {}, {}, "c36", True, "rg.ddpm.c36"),
               "ddpm.c48": ("ddpm", {}, {}, "c48", False, None)}


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_blind_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """The fused loop against `_generic_loop` on the same injected draws at the fused-vs-generic bars of tests/test_rgb_gpu.py (as
    tests/test_psf_gpu.py takes them; 1e-4 for 4 -> 8), and the two routes' final kernels under 5 x the oracle chain's float64 /
    float32 kernel distance."""
    _, gd, M, CM = pkg
    sname, skw, pat_kw, net, masked, ref_tag = CHAIN_CASES[tag]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    kbar = 5.0 * oracle_chain()["d_kernel"]
    pat = dict(PATTERN, **pat_kw)
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, sampler.num_timesteps))
    x_T, y, noise, mask = chain_inputs(1, C, n)
    x_T, y, noise = x_T.to(DEV), y.to(DEV), noise.to(DEV)
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=True,
              sample_pattern=pat, measurement_mask=mask if masked else None)
    cond = blind_cond(pkg, **CHAIN_OKW)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, pat, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    kf = cond.operator.kernel2d()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = blind_cond(pkg, third_party=C == 4, **CHAIN_OKW)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, pat, tuple(x_T.shape)) is None
    _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    kg = cond.operator.kernel2d()
    e, ek = float((f.cpu() - g.detach().cpu()).abs().max()), float(np.abs(kf - kg).max())
    moved = float(max(r["grad"].abs().max() for r in trace))
    kmoved = float(np.abs(kf.reshape(-1) - cond.operator.host_taps()[2]).max())
    print(f"BLINDCHAIN {tag}: fused vs generic image {e:.3e} (bar {bar:.3e}), kernel {ek:.3e} (bar {kbar:.3e}); largest guidance "
          f"gradient {moved:.2e}, the kernel moved {kmoved:.2e}")
    assert moved > 0.0 and kmoved > 1e-4
    assert e <= bar and ek <= kbar
    assert abs(kf.sum() - 1.0) < 1e-6 and (kf >= 0).all()


def test_fused_blind_chain_vs_the_oracle_chain(pkg, monkeypatch, model36):
    """One 10-index DDPM chain, free-running against the oracle's driver with the same weights, x_T, measurement and noise, under
    10 x the oracle's own drift for a 1e-6 perturbation of x_T -- the image's drift for the image, the kernel's for the kernel."""
    _, gd, M, CM = pkg
    o = oracle_chain()
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(o["tb"].timestep_map)
    x_T, y, noise, _ = chain_inputs(1, 3, 10)
    nd = noise.to(DEV)
    cond = blind_cond(pkg, **CHAIN_OKW)
    _no_generic(monkeypatch, sampler)
    f = sampler.p_sample_loop(model=model36, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k])
    bar, kbar = _free_running_bar(o["drift"]), 10.0 * o["d_kernel_drift"]           # the same rule for the kernel: 10 x ITS drift
    e = float((f.cpu() - o["img"]).abs().max())
    ek = float(np.abs(cond.operator.kernel2d().reshape(-1) - o["w"].astype(np.float64)).max())
    print(f"BLINDCHAIN oracle: image {e:.3e} (oracle drift_1e-6 {o['drift']:.2e}, bar {bar:.2e}); kernel {ek:.3e} (oracle float64 vs "
          f"float32 {o['d_kernel']:.3e}, under the perturbation {o['d_kernel_drift']:.3e}, bar {kbar:.3e})")
    assert e <= bar and ek <= kbar


def test_batch_of_three_walked_as_two_and_one_equals_one_pass(pkg, monkeypatch, model36):
    """The PSF couples the batch: every chunk's forward, ONE data term over the three images, every chunk's backward (after a
    re-forward).  Image and kernel agree with the one-pass chain bit for bit."""
    _, gd, M, CM = pkg
    x_T, y, noise, mask = chain_inputs(3, 3, 10, seed=32)
    x_T, y, noise = x_T.to(DEV), y.to(DEV), noise.to(DEV)
    calls = []

    def run():
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        cond = blind_cond(pkg, 3, **CHAIN_OKW)
        orig = cond.loss_grad_x0

        def counted(x0, *a, **k):
            calls.append(x0.shape[0])
            return orig(x0, *a, **k)
        cond.loss_grad_x0 = counted
        img = sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                    noise_fn=lambda k, shape: noise[k], measurement_mask=mask, index_range=(9, 5))
        return img, cond.operator.kernel2d()
    whole, kw = run()
    assert bool(torch.isfinite(whole).all()) and calls == [3] * 5
    seen = []

    def two_one(B, cap):
        seen.append(B)
        return [2, 1]
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(two_one))
    del calls[:]
    chunked, kc = run()
    monkeypatch.undo()
    assert seen == [3] and calls == [3] * 5                              # still ONE data term per sub-step, over the whole batch
    assert torch.equal(chunked, whole) and np.array_equal(kc, kw)


def test_poisson_raises_and_tiling_keeps_refusing(pkg, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    x_T, y, _, _ = chain_inputs(1, 3, 10)
    kw = dict(model=model36, x_start=x_T.to(DEV), measurement=y.to(DEV), record=False, save_root=None, pretrain_model="imagenet",
              rgb_guidance=True, sample_pattern=PATTERN)
    poisson = CM.PosteriorSampling(M.get_operator("blind_blur", device=DEV, **CHAIN_OKW), M.get_noise("poisson", rate=1.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="poisson"):
        sampler.p_sample_loop(measurement_cond_fn=poisson.conditioning, **kw)
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(measurement_cond_fn=blind_cond(pkg, **CHAIN_OKW).conditioning, tiling=dict(tile=16, stride=8), **kw)


# ------------------------------------------------------------------------------------------------------------ 6: the driver
def test_restore_image_learns_a_kernel_resets_it_per_global_iteration_and_writes_it(pkg, monkeypatch, model48, tmp_path):
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    resets = []
    orig = M.BlindBlurOperator.reset
    monkeypatch.setattr(M.BlindBlurOperator, "reset", lambda self: (resets.append(self.kernel2d()), orig(self))[1])
    g = torch.Generator().manual_seed(41)
    ref = (torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV)
    cfg = {"measurement": {"operator": dict(name="blind_blur", simulate_with=dict(name="motion_blur", kernel_size=5, intensity=0.5), **CHAIN_OKW),
                           "noise": {"name": "gaussian", "sigma": 0.0}},
           "conditioning": {"method": "ps", "params": dict(scale="0.3")},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="4"),
           "sample_pattern": dict(PATTERN, global_N=2), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": True}
    res = sampling.restore_image(model48, ref, cfg, noise_seed=7, index_range=(3, 1))
    assert len(res) == 2 and len(resets) == 2
    init = M.blind_init_kernel(5, "gaussian", 1.0).astype(np.float32).astype(np.float64)
    assert np.array_equal(resets[0], init) and not np.array_equal(resets[1], init)       # the second reset found a learnt kernel
    blurred = M.get_operator("motion_blur", device=DEV, kernel_size=5, intensity=0.5).forward(ref).cpu()
    for r in res:
        k = r["kernel"]
        assert k.dtype == torch.float32 and k.shape == (5, 5) and abs(float(k.double().sum()) - 1.0) <= 1e-6 and float(k.min()) >= 0.0
        assert torch.equal(r["measurement"], blurred) and bool(torch.isfinite(r["sample"]).all())
    assert torch.equal(res[0]["kernel"], res[1]["kernel"]) and torch.equal(res[0]["sample"], res[1]["sample"])   # same seed, same start
    assert not np.array_equal(res[0]["kernel"].double().numpy(), init)
    # an index-less device, as the reference driver passes it: the learnt kernel, not the init, comes back
    named = sampling.restore_image(model48, ref, dict(cfg, sample_pattern=dict(PATTERN)), device="cuda", noise_seed=7, index_range=(3, 1))
    assert torch.equal(named[-1]["kernel"], res[-1]["kernel"])
    paths = sampling.save_outputs(res[-1], ref.cpu(), str(tmp_path), "photo", save_grids=False)
    assert paths["kernel"].endswith("photo_kernel.png") and os.path.exists(paths["kernel"])
    from PIL import Image
    pic = np.asarray(Image.open(paths["kernel"]))
    assert pic.shape == (125, 125) and pic.max() == 255
    # simulate: False takes the photo as it is (it must have the network's grid)
    with pytest.raises(ValueError, match="simulate"):
        bad = dict(cfg, measurement=dict(cfg["measurement"], operator=dict(name="blind_blur", simulate=False, **CHAIN_OKW)))
        sampling.restore_image(model48, ref, bad, noise_seed=7)
