"""Motion-blur and arbitrary-PSF measurement operators on the GPU: osm_psf_apply (forward and adjoint) against the float64 product
of the SAME fp32 taps and inputs -- F.conv2d on the reflect-padded input and its vector-Jacobian product --, the `osmosis::psf_apply`
operator, the 'ps' data term through an operator, and the fused sampler loop against `_generic_loop`.  The reference has no such
operators: the oracle is torch on the CPU in float64.

Kernel bar (derived, not tuned): an output element is the sum of N products, each added with one rounding (an fma, or a plain add
where the adjoint joins its mirror sums), so whatever the order |err| <= (N + 2) 2^-24 sum |w| |x| per element (the + 2: the standard
(1 + u)^n - 1 <= n u / (1 - n u) slack): N = T for the forward, at most 9 T for the adjoint (3 x 3 pre-images per tap at a corner).

Worst |err| / bound measured (forward / adjoint, over C in {3, 4}): see the PSF lines of the README.
"""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U24 = 2.0 ** -24
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")                   # the tiny 3 -> 6 network
H0, W0 = 16, 24            # the chains' grid (tests/test_linop_gpu.py: the tiny networks attend over (H / 4)(W / 4) tokens)
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)


def _delta():
    k = np.zeros((5, 7))
    k[2 + 2, 3 - 3] = 1.0                                           # one tap (dy = 2, dx = -3)
    return k


def _dense(kh, kw, seed, zeros=()):
    k = np.random.default_rng(seed).standard_normal((kh, kw))
    for z in zeros:
        k[z] = 0.0
    return k


# case -> (operator name, its kwargs, H, W)
CASES = {"delta": ("psf_blur", lambda: dict(kernel=_delta(), normalize=False), 20, 27),          # sign and flip convention
         "asym3x7": ("psf_blur", lambda: dict(kernel=_dense(3, 7, 1, [(0, 2), (2, 5)]), normalize=False), 20, 27),   # kh != kw, width no multiple of 4
         "both_mirrors": ("psf_blur", lambda: dict(kernel=_dense(9, 9, 2), normalize=False), 8, 6),  # smaller than a tile, R = W - 2
         "tiles": ("motion_blur", lambda: dict(kernel_size=9, intensity=0.5), 40, 72),           # halos across seams, all four edges
         "motion61": ("motion_blur", lambda: dict(), 64, 96),                                    # the default trajectory
         "dense61": ("psf_blur", lambda: dict(kernel=_dense(61, 61, 3), normalize=False), 64, 64),   # the largest halo: LDS capacity
         "motion9.chain": ("motion_blur", lambda: dict(kernel_size=9, intensity=0.5), H0, W0)}
KERNEL_CASES = [c for c in CASES if not c.endswith(".chain")]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


def make_op(M, case, B=1):
    name, kw, H, W = CASES[case]
    return M.get_operator(name, device=DEV, batch_size=B, **kw()), H, W


def kernel64(op):
    """The float64 [2 Ry + 1, 2 Rx + 1] kernel of the operator's fp32 taps."""
    dy, dx, w = op.host_taps()
    Ry, Rx = op.radius()
    k = np.zeros((2 * Ry + 1, 2 * Rx + 1))
    k[dy + Ry, dx + Rx] = w.astype(np.float64)
    return torch.from_numpy(k)


def conv_reflect(x, k):
    kh, kw = k.shape
    P = x.shape[1]
    return F.conv2d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), k.expand(P, 1, kh, kw).contiguous(), groups=P)


def conv_reflect_vjp(v, k):
    x = torch.zeros_like(v).requires_grad_(True)
    g, = torch.autograd.grad(conv_reflect(x, k), x, v)
    return g


def apply_kernel(op, x, C_out, adjoint, R=None):
    """osm_psf_apply on the colour planes of x [B,C_in,H,W] into a NaN-filled [B,C_out,H,W] (planes beyond 2: zero_planes)."""
    from osmosis_diffusion_code_amd import ops
    B, C_in, H, W = x.shape
    Ry, Rx = op.radius() if R is None else R
    out = torch.full((B, C_out, H, W), float("nan"), device=DEV)
    ops.psf_apply(x, out, *op.taps(DEV), Ry, Rx, B, 3, C_in * H * W, C_out * H * W, H, W, adjoint=adjoint, zero_planes=C_out - 3)
    return out


_REF = {}


def reference(M, case):
    """Inputs and the float64 products of a case, computed once: x [2,4,H,W], v [2,3,H,W]; A x, A^T v and the same on |x|, |v|, |w|."""
    if case not in _REF:
        op, H, W = make_op(M, case)
        g = torch.Generator().manual_seed(11)
        x, v = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
        k = kernel64(op)
        x64, v64 = x[:, 0:3].double(), v.double()
        _REF[case] = dict(op=op, H=H, W=W, x=x, v=v, T=len(op.host_taps()[2]), Ax=conv_reflect(x64, k), Atv=conv_reflect_vjp(v64, k),
                          mag_f=conv_reflect(x64.abs(), k.abs()), mag_a=conv_reflect_vjp(v64.abs(), k.abs()))
    return _REF[case]


def check(got, want, bound, what):
    assert bool(torch.isfinite(got).all()), f"{what}: an output element was not written"
    err = (got[:, 0:3].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"PSF {what}: worst |err| / bound {ratio:.3f} (max |err| {float(err.max()):.2e})")
    assert ratio <= 1.0, (what, ratio)
    if got.shape[1] > 3:
        assert float(got[:, 3:].abs().max()) == 0.0 and not bool(torch.signbit(got[:, 3:]).any())      # the zero planes: exactly +0


# ------------------------------------------------------------------------------------------------------------ 1: the kernel
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_forward_and_adjoint_vs_float64_product(pkg, case, C):
    _, _, M, _ = pkg
    ref = reference(M, case)
    op, T = ref["op"], ref["T"]
    x, v = ref["x"][:, 0:C].contiguous(), ref["v"]
    xd, vd = x.to(DEV), v.to(DEV)
    bf, ba = (T + 2) * U24 * ref["mag_f"], (9 * T + 2) * U24 * ref["mag_a"]
    Ax = apply_kernel(op, xd, 3, False).cpu()                   # reads the colour planes of [B,C,HW]
    Atv = apply_kernel(op, vd, C, True).cpu()                   # writes [B,C,HW], the depth plane as +0
    check(Ax, ref["Ax"], bf, f"{case} C={C} forward")
    check(Atv, ref["Atv"], ba, f"{case} C={C} adjoint")
    if case == "delta":                                         # out[i, j] = x[refl(i + 2), refl(j - 3)], bit for bit
        H, W = ref["H"], ref["W"]
        rows = [i + 2 if i + 2 < H else 2 * (H - 1) - (i + 2) for i in range(H)]
        cols = [abs(j - 3) for j in range(W)]
        assert torch.equal(Ax, x[:, 0:3][:, :, rows][:, :, :, cols])
    # <A x, v> = <x, A^T v>, in float64 from the kernel's fp32 outputs, under the bound the two element bounds give
    x64, v64 = x[:, 0:3].double(), v.double()
    lhs, rhs = float((Ax.double() * v64).sum()), float((x64 * Atv[:, 0:3].double()).sum())
    allow = float((bf * v64.abs()).sum() + (ba * x64.abs()).sum())
    print(f"PSF {case} C={C} adjoint identity: |<Ax,v> - <x,Atv>| / bound {abs(lhs - rhs) / allow:.3f}")
    assert abs(lhs - rhs) <= allow
    # bit-reproducible, and a B = 2 call is two B = 1 calls
    assert torch.equal(apply_kernel(op, xd, 3, False).cpu(), Ax) and torch.equal(apply_kernel(op, vd, C, True).cpu(), Atv)
    for b in range(2):
        assert torch.equal(apply_kernel(op, xd[b:b + 1].contiguous(), 3, False).cpu()[0], Ax[b]), b
        assert torch.equal(apply_kernel(op, vd[b:b + 1].contiguous(), C, True).cpu()[0], Atv[b]), b


def test_unstaged_and_staged_tiles_give_the_same_bits(pkg):
    """A workgroup stages its (32 + 2 Ry) x (32 + 2 Rx) window in LDS while (32 + 2 Ry) ((32 + 2 Rx) | 1) <= 96 * 97 floats, and reads
    global memory beyond.  The radius is the caller's statement (taps beyond it are skipped, a larger one only widens the halo), so the
    `tiles` taps (reach 4) are run at the stated radii 4 (staged), 32 (the last staged size: 96 x 97), 33 (the first unstaged: 98 x 99)
    and 39 = H - 1: the same fmas in the same order, the same bits."""
    _, _, M, _ = pkg
    ref = reference(M, "tiles")
    op = ref["op"]
    assert max(op.radius()) <= 4 and (32 + 64) * ((32 + 64) | 1) <= 96 * 97 < (32 + 66) * ((32 + 66) | 1)
    xd, vd = ref["x"].to(DEV), ref["v"].to(DEV)
    for adjoint, src in ((False, xd), (True, vd)):
        base = apply_kernel(op, src, 4, adjoint)
        for R in (32, 33, 39):
            assert torch.equal(apply_kernel(op, src, 4, adjoint, R=(R, R)), base), (adjoint, R)
        assert torch.equal(apply_kernel(op, src, 4, adjoint, R=(39, 4)), base) and torch.equal(apply_kernel(op, src, 4, adjoint, R=(4, 39)), base)


def test_a_tap_beyond_the_stated_radius_is_skipped(pkg):
    _, _, M, _ = pkg
    ref = reference(M, "asym3x7")
    op = ref["op"]                                              # reach (1, 3)
    dy, dx, w = op.host_taps()
    keep = np.abs(dx) <= 2
    inner = M.get_operator("psf_blur", device=DEV, normalize=False, kernel=kernel64(op).numpy()[:, 1:-1])
    assert inner.radius() == (1, 2) and np.array_equal(inner.host_taps()[2], w[keep])
    xd = ref["x"].to(DEV)
    for adjoint in (False, True):
        assert torch.equal(apply_kernel(op, xd, 3, adjoint, R=(1, 2)), apply_kernel(inner, xd, 3, adjoint))


def test_bad_arguments_return_a_status_and_launch_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    _, _, M, _ = pkg
    op, H, W = make_op(M, "asym3x7")
    dy, dx, w = op.taps(DEV)
    x = torch.randn(1, 3, H, W, device=DEV)
    out = torch.full((1, 3, H, W), float("nan"), device=DEV)
    lib = _lib.load()
    p = _lib.ptr
    good = [p(x), p(out), p(dy), p(dx), p(w), w.shape[0], 1, 3, 1, 3, 3 * H * W, 3 * H * W, H, W, 0, 0, None]
    for pos, val in ((0, None), (2, None), (5, 0), (6, H), (7, W), (14, 2)):     # null pointer, T < 1, R >= the image side, a bad flag
        args = list(good)
        args[pos] = val
        assert lib.osm_psf_apply(*args) != 0 and lib.osm_last_error().decode().startswith("osm_psf_apply")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.OsmosisHipError, match="smaller"):
        ops.psf_apply(x, out, dy, dx, w, 1, 3, 2, 3, 3 * H * W, 3 * H * W, H, W)
    with pytest.raises(_lib.OsmosisHipError, match="Ry"):
        ops.psf_apply(x, out, dy, dx, w, H, 3, 1, 3, 3 * H * W, 3 * H * W, H, W)
    assert lib.osm_psf_apply(*good) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ 2: the operator
def test_opcheck_and_autograd_of_psf_apply(pkg):
    _, _, M, _ = pkg
    for case in ("asym3x7", "both_mirrors", "tiles"):
        op, H, W = make_op(M, case)
        t, (Ry, Rx) = op.taps(DEV), op.radius()
        g = torch.Generator().manual_seed(12)
        x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        torch.library.opcheck(torch.ops.osmosis.psf_apply.default, (x, *t, Ry, Rx, False))
        torch.library.opcheck(torch.ops.osmosis.psf_apply.default, (x.clone().requires_grad_(True), *t, Ry, Rx, False))
        torch.library.opcheck(torch.ops.osmosis.psf_apply.default, (x.clone().requires_grad_(True), *t, Ry, Rx, True))
        xr = x.clone().requires_grad_(True)
        y = op.forward(xr)
        assert y.shape == (2, 3, H, W) and torch.equal(y.detach(), apply_kernel(op, x, 3, False))
        cot = torch.randn(2, 3, H, W, generator=g).to(DEV)
        gx, = torch.autograd.grad(y, xr, cot)
        assert torch.equal(gx, op.transpose(cot)) and torch.equal(gx, apply_kernel(op, cot, 3, True))      # the adjoint launch, bit for bit
        # ... and the backward of the adjoint is the forward
        cr = cot.clone().requires_grad_(True)
        gc, = torch.autograd.grad(op.transpose(cr), cr, x)
        assert torch.equal(gc, y.detach())
        assert op.ortho_project(x).shape == x.shape
    with pytest.raises(ValueError, match="reflection"):
        make_op(M, "motion61")[0].forward(torch.zeros(1, 3, 16, 24, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 3: the data term
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", ["tiles", "both_mirrors"])
def test_ps_data_term_through_a_psf_vs_float64_autograd(pkg, case, masked, C):
    """loss[b] = ||M (y - A x0[b, 0:3])|| and its x0-gradient against float64 autograd on the CPU, at the bars
    tests/test_linop_gpu.py and tests/test_mask_gpu.py hold the 'ps' term to: loss 2e-6 relative, gradient 2e-7 + 1e-5 max |want|;
    the depth channel's gradient exactly 0; a fully masked image has loss 0 and gradient 0."""
    _, _, M, CM = pkg
    B = 3
    op, H, W = make_op(M, case, B)
    g = torch.Generator().manual_seed(21)
    x0 = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
    mask = torch.ones(B, 3, H, W)
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g)
        mask[1] = (torch.rand(1, 1, H, W, generator=g) > 0.4).float()
        mask[2] = 0.0                                                           # image 2: masked out entirely
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    gk, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    gk, loss = gk.cpu().double(), loss.cpu().double()
    assert gk.shape == (B, C, H, W) and bool(torch.isfinite(gk).all()) and bool(torch.isfinite(loss).all())
    x64 = x0.double().requires_grad_(True)
    r = mask.double() * (y.double() - conv_reflect(x64[:, 0:3], kernel64(op)))
    L = (r ** 2).sum(dim=(1, 2, 3)).sqrt()
    live = range(2) if masked else range(B)
    want, = torch.autograd.grad(sum(L[b] for b in live), x64)
    L = L.detach()
    for b in live:
        el, eg = abs(float(loss[b]) - float(L[b])) / float(L[b]), float((gk[b, 0:3] - want[b, 0:3]).abs().max())
        print(f"PSFTERM {case} masked={masked} C={C} image {b}: loss rel {el:.2e}, grad abs {eg:.2e} (max |want| {float(want[b, 0:3].abs().max()):.2e})")
        assert el <= 2e-6, (b, float(loss[b]), float(L[b]))
        assert eg <= 2e-7 + 1e-5 * float(want[b, 0:3].abs().max()), (b, eg)
    if C == 4:
        assert float(gk[:, 3].abs().max()) == 0.0
    if masked:
        assert float(loss[2]) == 0.0 and float(gk[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 4: the chains
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
    """torch.randn_like for `_generic_loop` on the rgb-guidance branch: per call p_sample draws first, then q_sample on the
    measurement (unused by `ps`): the even draws replay `noise`."""
    state, orig = {"k": 0}, torch.randn_like

    def replay(t, **kw):
        k = state["k"]
        state["k"] += 1
        return noise[k // 2].clone() if k % 2 == 0 else orig(t, **kw)
    monkeypatch.setattr(torch, "randn_like", replay)


CHAIN = "motion9.chain"


def ps_cond(pkg, B=1, noiser=None, third_party=False):
    _, _, M, CM = pkg
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    return cls(make_op(M, CHAIN, B)[0], noiser or M.get_noise("gaussian", sigma=0.0), scale="0.3")


# case -> (sampler, sampler kwargs, branch, pattern changes, network, masked, the tests/test_rgb_gpu.py chain whose bar applies)
CHAIN_CASES = {"ddpm": ("ddpm", {}, "rg", {}, "c36", False, "rg.ddpm.c36"),
               "ddim.clip": ("ddim", dict(clip_denoised=True), "rg", {}, "c36", False, "rg.ddim.c36"),
               "m2": ("ddpm", {}, "rg", dict(local_M=2, s_start=0.5, s_end=0.0), "c36", False, "rg.ddpm.c36.m2"),
               "mean_only": ("ddpm", {}, "mo", {}, "c36", False, "mo.ddpm.c36"),
               "masked": ("ddpm", {}, "rg", {}, "c36", True, "rg.ddpm.c36"),
               "ddpm.c48": ("ddpm", {}, "rg", {}, "c48", False, None)}
# tests/test_rgb_gpu.py MEASURED of those chains, as tests/test_linop_gpu.py copies them (the bar: min(5 x measured, 10 x the
# recorded drift_1e-6 of tests/golden/loop_rgb.npz))
MEASURED_RGB = {"rg.ddpm.c36": 5.960e-07, "rg.ddim.c36": 7.153e-07, "mo.ddpm.c36": 5.960e-07, "rg.ddpm.c36.m2": 1.162e-06}


def chain_inputs(B, C, n, seed=31):
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H0, W0, generator=g)
    y = torch.rand(B, 3, H0, W0, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, H0, W0, generator=g)
    mask = torch.rand(B, 3, H0, W0, generator=g) * (torch.rand(B, 1, H0, W0, generator=g) > 0.3).float()
    mask[:, :, 4:9, 6:13] = 0.0                                      # a hole on the measurement's grid
    return x_T.to(DEV), y.to(DEV), noise.to(DEV), mask


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_motion_blur_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """The fused loop against `_generic_loop` (autograd through `operator.forward` = osmosis::psf_apply and the HIP UNet) on the same
    injected draws, at exactly the bars of tests/test_linop_gpu.py: the fused-vs-generic bar of the identity 'ps' chain of the same
    sampler / branch on the tiny 3 -> 6 network (min(5 x its measured deviation, 10 x its recorded drift_1e-6)), 1e-4 for 4 -> 8.
    Measured deviations: see the PSF lines of the README."""
    _, gd, M, CM = pkg
    sname, skw, branch, pat_kw, net, masked, ref_tag = CHAIN_CASES[tag]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    pat = dict(PATTERN, **pat_kw)
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, sampler.num_timesteps))
    x_T, y, noise, mask = chain_inputs(1, C, n)
    rg = branch == "rg"
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=rg,
              sample_pattern=pat, measurement_mask=mask if masked else None)
    cond = ps_cond(pkg)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = ps_cond(pkg, third_party=C == 4)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is None
    if rg:
        _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    moved = float(max(r["grad"].abs().max() for r in trace))
    print(f"PSFCHAIN {tag}: fused vs generic {e:.3e} (bar {bar:.3e}); largest guidance gradient {moved:.2e}")
    assert moved > 0.0
    assert e <= bar


def test_psf_operators_stay_fused_and_poisson_goes_generic(pkg, monkeypatch, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    x_T, y, noise, _ = chain_inputs(1, 3, 10)
    cond = ps_cond(pkg)
    assert sampler._fast_path_ok(model36, cond.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is cond
    poisson = ps_cond(pkg, noiser=M.get_noise("poisson", rate=1.0))
    assert sampler._fast_path_ok(model36, poisson.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is None
    # a user's PSF takes the fused loop end to end
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    user = CM.PosteriorSampling(M.get_operator("psf_blur", device=DEV, kernel=[[0.0, 1.0, 2.0], [0.5, 3.0, 0.0], [0.0, 0.25, 1.0]]),
                                M.get_noise("gaussian", sigma=0.0), scale="0.3")
    assert sampler._fast_path_ok(model36, user.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is user
    for c in (cond, user):
        img = sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=c.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                    index_range=(9, 6))
        assert img.shape == (1, 3, H0, W0) and bool(torch.isfinite(img).all())
    # tiling keeps refusing the 'ps' branch
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              tiling=dict(tile=16, stride=8))


def test_batch_of_three_walked_in_chunks_equals_one_pass(pkg, monkeypatch, model36):
    """B = 3 with a mask: the one-pass chain, the walk OSM_MAX_BATCH=2 forces and a [2, 1] walk agree bit for bit."""
    _, gd, M, CM = pkg
    x_T, y, noise, mask = chain_inputs(3, 3, 10, seed=32)

    def run():
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        cond = ps_cond(pkg, 3)
        return sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                     save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                     noise_fn=lambda k, shape: noise[k], measurement_mask=mask, index_range=(9, 5))
    whole = run()
    assert bool(torch.isfinite(whole).all())
    monkeypatch.setenv("OSM_MAX_BATCH", "2")
    capped = run()
    monkeypatch.undo()
    assert torch.equal(capped, whole)
    seen = []

    def two_one(B, cap):
        seen.append(B)
        return [2, 1]
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(two_one))
    chunked = run()
    monkeypatch.undo()
    assert seen == [3] and torch.equal(chunked, whole)


# ------------------------------------------------------------------------------------------------------------ 5: the driver
def test_restore_image_simulates_the_measurement_or_takes_it_as_it_is(pkg, monkeypatch, model36):
    """`restore_image` with `motion_blur`: y = noiser(A ref) by default; `simulate: False` takes ref as the measurement, which then
    must have the network's grid (a PSF's measurement has the image's size)."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(41)
    ref = (torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV)

    def cfg(**okw):
        return {"measurement": {"operator": dict(name="motion_blur", kernel_size=9, intensity=0.5, **okw), "noise": {"name": "gaussian", "sigma": 0.0}},
                "conditioning": {"method": "ps", "params": dict(scale="0.3")},
                "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                                  model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                                  timestep_respacing="4"),
                "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "imagenet"},
                "manual_seed": 0, "rgb_guidance": True}
    res = sampling.restore_image(model36, ref, cfg(), noise_seed=7)[-1]
    op = M.get_operator("motion_blur", device=DEV, kernel_size=9, intensity=0.5)
    blurred = op.forward(ref).cpu()
    assert res["sample"].shape == (1, 3, H0, W0) and bool(torch.isfinite(res["sample"]).all())
    assert torch.equal(res["measurement"], blurred) and not torch.equal(blurred, ref.cpu())
    # the measurement itself, on the network's 256 x 256 grid
    y = (torch.rand(1, 3, 256, 256, generator=g) * 1.6 - 0.8).to(DEV)
    own = sampling.restore_image(model36, y, cfg(simulate=False), noise_seed=7)[-1]
    assert own["sample"].shape == (1, 3, 256, 256) and bool(torch.isfinite(own["sample"]).all())
    assert torch.equal(own["measurement"], y.cpu())
    with pytest.raises(ValueError, match="simulate"):
        sampling.restore_image(model36, ref, cfg(simulate=False), noise_seed=7)
