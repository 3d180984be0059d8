"""Blur and super-resolution measurement operators on the GPU: osm_linop_apply (forward and adjoint) against the float64 dense
product of the SAME fp32 tables and inputs, the `osmosis::linop_apply` operator, the 'ps' data term through an operator, and the
fused sampler loop against `_generic_loop`.  The reference has no such operators: the oracle is torch on the CPU in float64.

Kernel bar (derived, not tuned): an output is Kw fused multiply-adds (horizontal) then Kh (vertical) in fp32, each rounding once, so
|err| <= (Kh + Kw + 2) 2^-24 sum |wt_h| |wt_w| |x| per element (the + 2: the standard (1 + u)^n - 1 <= n u / (1 - n u) slack).
"""
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U24 = 2.0 ** -24
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")                   # the tiny 3 -> 6 network
H0, W0 = 16, 24            # the chains' grid (see CASES)
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)
CASES = {"blur9": ("gaussian_blur", dict(kernel_size=9, intensity=1.5), 24, 36),          # reflection at all four edges
         "blur13": ("gaussian_blur", dict(kernel_size=13, intensity=3.0), 16, 16),        # band close to the image size
         "bicubic4": ("super_resolution", dict(scale_factor=4), 24, 36),                  # 6 x 9: output width no multiple of 4
         "bicubic3": ("super_resolution", dict(scale_factor=3), 21, 27),                  # odd sizes, unaligned rows
         "box2": ("super_resolution", dict(scale_factor=2, method="box"), 16, 20),
         "blur61": ("gaussian_blur", dict(kernel_size=61, intensity=3.0), 256, 256),      # the LDS-capacity case
         # x 8 on 320 x 40 -> 40 x 5: the first row tile (output rows 0..31) spans 268 input rows, more than the kernel's 256-row LDS
         # buffer, so it takes the unstaged path (every lane sums straight from global memory; output width 5: its one-column
         # tail), the second (rows 32..39, 76 input rows) the staged one -- both in one output
         "bicubic8": ("super_resolution", dict(scale_factor=8), 320, 40),
         # the chains' grid: the tiny networks attend over (H / 4)(W / 4) tokens, which the engine needs a multiple of 4 (24 x 36 gives
         # 54), so the chains run on the 16 x 24 grid of tests/test_mask_gpu.py (4 x 6 after super-resolution x 4)
         "blur9.chain": ("gaussian_blur", dict(kernel_size=9, intensity=1.5), H0, W0),
         "bicubic4.chain": ("super_resolution", dict(scale_factor=4), H0, W0)}
KERNEL_CASES = [c for c in CASES if not c.endswith(".chain")]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


def make_op(M, case, B=1):
    name, kw, H, W = CASES[case]
    return M.get_operator(name, device=DEV, batch_size=B, **kw), H, W


def dense64(M, tabs, n_h, n_w):
    sh, wh, sw, ww = tabs
    return (torch.from_numpy(M.band_to_dense(sh, wh, n_h).astype(np.float64)), torch.from_numpy(M.band_to_dense(sw, ww, n_w).astype(np.float64)))


def apply_kernel(tabs_dev, x, C_in, C_out, Hin, Win, B=None):
    """osm_linop_apply on the colour planes of x [B,C_in,Hin,Win] into a NaN-filled [B,C_out,Hout,Wout] (planes beyond 2: zero_planes)."""
    from osmosis_diffusion_code_amd import ops
    B = x.shape[0] if B is None else B
    Hout, Wout = tabs_dev[1].shape[0], tabs_dev[3].shape[0]
    out = torch.full((B, C_out, Hout, Wout), float("nan"), device=DEV)
    ops.linop_apply(x, out, *tabs_dev, B, 3, C_in * Hin * Win, C_out * Hout * Wout, Hin, Win, zero_planes=C_out - 3)
    return out


def check_against_dense(M, tabs_host, tabs_dev, x, C_out, Hin, Win, what):
    """-> (kernel output, per-element bound); asserts the worst |err| / bound <= 1 and that every element was written."""
    got = apply_kernel(tabs_dev, x.to(DEV), x.shape[1], C_out, Hin, Win).cpu()
    assert bool(torch.isfinite(got).all()), f"{what}: an output element was not written"
    Rh, Rw = dense64(M, tabs_host, Hin, Win)
    x64 = x[:, 0:3].double()
    want = torch.einsum("ia,bpac,jc->bpij", Rh, x64, Rw)
    mag = torch.einsum("ia,bpac,jc->bpij", Rh.abs(), x64.abs(), Rw.abs())
    bound = (tabs_host[1].shape[1] + tabs_host[3].shape[1] + 2) * U24 * mag
    err = (got[:, 0:3].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"LINOP {what}: worst |err| / bound {ratio:.3f} (max |err| {float(err.max()):.2e})")
    assert ratio <= 1.0, (what, ratio)
    if C_out > 3:
        assert float(got[:, 3:].abs().max()) == 0.0 and not bool(torch.signbit(got[:, 3:]).any())      # the zero planes: exactly 0
    return got, bound


# ------------------------------------------------------------------------------------------------------------ 1: the kernel
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", KERNEL_CASES)
def test_forward_and_adjoint_vs_float64_dense_product(pkg, case, C):
    _, _, M, _ = pkg
    op, H, W = make_op(M, case)
    h, w = op.out_shape(H, W)
    host, dev = op.host_tables(H, W), op.tables(H, W, DEV)
    g = torch.Generator().manual_seed(11)
    B = 2
    x = torch.randn(B, C, H, W, generator=g)
    v = torch.randn(B, 3, h, w, generator=g)
    Ax, bf = check_against_dense(M, host["fwd"], dev["fwd"], x, 3, H, W, f"{case} C={C} forward")
    Atv, ba = check_against_dense(M, host["adj"], dev["adj"], v, C, h, w, f"{case} C={C} adjoint")
    assert Ax.shape == (B, 3, h, w) and Atv.shape == (B, C, H, W)
    # <A x, v> = <x, A^T v>, in float64 from the kernel's fp32 outputs, under the bound the two element bounds give
    lhs = float((Ax.double() * v.double()).sum())
    rhs = float((x[:, 0:3].double() * Atv[:, 0:3].double()).sum())
    allow = float((bf * v.double().abs()).sum() + (ba * x[:, 0:3].double().abs()).sum())
    rel = abs(lhs - rhs) / (float(Ax.double().norm()) * float(v.double().norm()))
    print(f"LINOP {case} C={C} adjoint identity: |<Ax,v> - <x,Atv>| / (|Ax| |v|) = {rel:.2e}, / bound {abs(lhs - rhs) / allow:.3f}")
    assert abs(lhs - rhs) <= allow
    # bit-reproducible, and a B = 2 call is two B = 1 calls
    xd = x.to(DEV)
    again = apply_kernel(dev["fwd"], xd, C, 3, H, W).cpu()
    assert torch.equal(again, Ax)
    for b in range(B):
        one = apply_kernel(dev["fwd"], xd[b:b + 1].contiguous(), C, 3, H, W).cpu()
        assert torch.equal(one[0], Ax[b]), b
        one = apply_kernel(dev["adj"], v[b:b + 1].to(DEV), 3, C, h, w).cpu()
        assert torch.equal(one[0], Atv[b]), b


def test_unstaged_and_staged_tiles_give_the_same_bits(pkg):
    """The x 8 case's first row tile spans 268 input rows (unstaged: sums taken straight from global memory); the same output rows
    24..31 asked for through a table of rows 24..39 alone span 148 (staged through LDS).  Same fmas in the same order: same bits."""
    _, _, M, _ = pkg
    op, H, W = make_op(M, "bicubic8")
    sh, wh, sw, ww = op.tables(H, W, DEV)["fwd"]
    host_sh, host_wh = op.host_tables(H, W)["fwd"][:2]
    K = host_wh.shape[1]
    assert min(int(host_sh[:32].max()) + K, H) - int(host_sh[:32].min()) > 256       # tile 0 of the full table: unstaged
    assert min(int(host_sh[24:].max()) + K, H) - int(host_sh[24:].min()) <= 256      # the 16-row table: staged
    x = torch.randn(2, 4, H, W, generator=torch.Generator().manual_seed(13)).to(DEV)
    full = apply_kernel((sh, wh, sw, ww), x, 4, 3, H, W)
    part = apply_kernel((sh[24:].contiguous(), wh[24:].contiguous(), sw, ww), x, 4, 3, H, W)
    assert full.shape == (2, 3, 40, 5) and part.shape == (2, 3, 16, 5)
    assert torch.equal(full[:, :, 24:], part)


def test_box_on_a_constant_image_is_exact(pkg):
    _, _, M, _ = pkg
    op, H, W = make_op(M, "box2")
    x = torch.full((2, 4, H, W), 0.37)
    out = apply_kernel(op.tables(H, W, DEV)["fwd"], x.to(DEV), 4, 3, H, W).cpu()
    assert torch.equal(out, torch.full((2, 3, H // 2, W // 2), 0.37))


def test_bad_arguments_return_a_status_and_launch_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    _, _, M, _ = pkg
    op, H, W = make_op(M, "bicubic4")
    sh, wh, sw, ww = op.tables(H, W, DEV)["fwd"]
    x = torch.randn(1, 3, H, W, device=DEV)
    out = torch.full((1, 3, 6, 9), float("nan"), device=DEV)
    lib = _lib.load()
    p = _lib.ptr
    good = [p(x), p(out), p(sh), p(wh), p(sw), p(ww), 1, 3, 3 * H * W, 3 * 54, H, W, 6, 9, wh.shape[1], ww.shape[1], 0, None]
    for pos, val in ((0, None), (2, None), (12, 0), (14, 0), (15, 0)):          # null pointer, Hout < 1, K < 1
        args = list(good)
        args[pos] = val
        assert lib.osm_linop_apply(*args) != 0 and lib.osm_last_error().decode().startswith("osm_linop_apply")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.OsmosisHipError, match="smaller"):
        ops.linop_apply(x, out, sh, wh, sw, ww, 2, 3, 3 * H * W, 3 * 54, H, W)
    assert lib.osm_linop_apply(*good) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------------------ 2: the operator
def test_opcheck_and_autograd_of_linop_apply(pkg):
    _, _, M, _ = pkg
    for case in ("blur9", "bicubic4"):
        op, H, W = make_op(M, case)
        h, w = op.out_shape(H, W)
        t = op.tables(H, W, DEV)
        g = torch.Generator().manual_seed(12)
        x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        torch.library.opcheck(torch.ops.osmosis.linop_apply.default, (x, *t["fwd"], h, w, *t["adj"]))
        torch.library.opcheck(torch.ops.osmosis.linop_apply.default, (x.clone().requires_grad_(True), *t["fwd"], h, w, *t["adj"]))
        torch.library.opcheck(torch.ops.osmosis.linop_apply.default, (x, *t["fwd"], h, w))          # forward only
        xr = x.clone().requires_grad_(True)
        y = op.forward(xr)
        assert y.shape == (2, 3, h, w) and torch.equal(y.detach(), apply_kernel(t["fwd"], x, 3, 3, H, W))
        cot = torch.randn(2, 3, h, w, generator=g).to(DEV)
        gx, = torch.autograd.grad(y, xr, cot)
        assert torch.equal(gx, op.transpose(cot))                                                    # bit for bit
        assert op.ortho_project(x).shape == x.shape
    from osmosis_diffusion_code_amd._lib import OsmosisHipError
    y = torch.ops.osmosis.linop_apply(xr, *t["fwd"], h, w)
    with pytest.raises(OsmosisHipError, match="transposed tables"):
        y.sum().backward()


# ------------------------------------------------------------------------------------------------------------ 3: the data term
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", ["blur9", "bicubic4", "box2"])
def test_ps_data_term_through_an_operator_vs_float64_autograd(pkg, case, masked, C):
    """loss[b] = ||M (y - A x0[b, 0:3])|| and its x0-gradient against float64 autograd on the CPU, at the bars
    tests/test_mask_gpu.py::test_masked_ps_loss_grad_vs_float64 holds the identity 'ps' term to: loss 2e-6 relative, gradient
    2e-7 + 1e-5 max |want|; the depth channel's gradient exactly 0; a fully masked image has loss 0 and gradient 0."""
    _, _, M, CM = pkg
    B = 3
    op, H, W = make_op(M, case, B)
    h, w = op.out_shape(H, W)
    g = torch.Generator().manual_seed(21)
    x0 = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
    mask = torch.ones(B, 3, h, w)
    if masked:
        mask = torch.rand(B, 3, h, w, generator=g)
        mask[1] = (torch.rand(1, 1, h, w, generator=g) > 0.4).float()          # image 1: the [1,1,h,w] broadcast form's values
        mask[2] = 0.0                                                           # image 2: masked out entirely
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    gk, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    gk, loss = gk.cpu().double(), loss.cpu().double()
    assert gk.shape == (B, C, H, W) and bool(torch.isfinite(gk).all()) and bool(torch.isfinite(loss).all())
    Rh, Rw = dense64(M, op.host_tables(H, W)["fwd"], H, W)
    x64 = x0.double().requires_grad_(True)
    r = mask.double() * (y.double() - torch.einsum("ia,bpac,jc->bpij", Rh, x64[:, 0:3], Rw))
    L = (r ** 2).sum(dim=(1, 2, 3)).sqrt()
    live = range(2) if masked else range(B)
    want, = torch.autograd.grad(sum(L[b] for b in live), x64)
    L = L.detach()
    for b in live:
        assert abs(float(loss[b]) - float(L[b])) <= 2e-6 * float(L[b]), (b, float(loss[b]), float(L[b]))
        e = float((gk[b, 0:3] - want[b, 0:3]).abs().max())
        assert e <= 2e-7 + 1e-5 * float(want[b, 0:3].abs().max()), (b, e)
    if C == 4:
        assert float(gk[:, 3].abs().max()) == 0.0
    if masked:
        assert float(loss[2]) == 0.0 and float(gk[2].abs().max()) == 0.0
        # the [1,1,h,w] broadcast form: every image under image 1's mask
        one = CM.get_conditioning_method("ps", make_op(M, case, B)[0], M.get_noise("gaussian", sigma=0.0), scale="0.3")
        one.set_measurement_mask(mask[1:2, 0:1], batch=B, device=DEV)
        g1, l1 = one.loss_grad_x0(x0.to(DEV), y.to(DEV))
        assert torch.equal(g1[1].cpu().double(), gk[1]) and float(l1[1]) == float(loss[1])


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


def ps_cond(pkg, case, B=1, noiser=None, third_party=False):
    _, _, M, CM = pkg
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    return cls(make_op(M, case, B)[0], noiser or M.get_noise("gaussian", sigma=0.0), scale="0.3")


CHAIN_OPS = {"blur": "blur9.chain", "sr4": "bicubic4.chain"}        # both on the 16 x 24 grid
# case -> (operator, sampler, sampler kwargs, branch, pattern changes, network, masked, the tests/test_rgb_gpu.py chain whose bar applies)
CHAIN_CASES = {"ddpm.blur": ("blur", "ddpm", {}, "rg", {}, "c36", False, "rg.ddpm.c36"),
               "ddpm.sr4": ("sr4", "ddpm", {}, "rg", {}, "c36", False, "rg.ddpm.c36"),
               "ddim.clip.blur": ("blur", "ddim", dict(clip_denoised=True), "rg", {}, "c36", False, "rg.ddim.c36"),
               "m2.sr4": ("sr4", "ddpm", {}, "rg", dict(local_M=2, s_start=0.5, s_end=0.0), "c36", False, "rg.ddpm.c36.m2"),
               "mean_only.blur": ("blur", "ddpm", {}, "mo", {}, "c36", False, "mo.ddpm.c36"),
               "masked.sr4": ("sr4", "ddpm", {}, "rg", {}, "c36", True, "rg.ddpm.c36"),
               "ddpm.sr4.c48": ("sr4", "ddpm", {}, "rg", {}, "c48", False, None)}
# tests/test_rgb_gpu.py MEASURED of those chains (its `chain_bar`: min(5 x measured, 10 x the recorded drift_1e-6))
MEASURED_RGB = {"rg.ddpm.c36": 5.960e-07, "rg.ddim.c36": 7.153e-07, "mo.ddpm.c36": 5.960e-07, "rg.ddpm.c36.m2": 1.162e-06}


def chain_inputs(pkg, case, B, C, n, seed=31):
    _, _, M, _ = pkg
    op, H, W = make_op(M, case)
    h, w = op.out_shape(H, W)
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H, W, generator=g)
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, H, W, generator=g)
    mask = torch.rand(B, 3, h, w, generator=g) * (torch.rand(B, 1, h, w, generator=g) > 0.3).float()
    mask[:, :, 1:3, 2:5] = 0.0                                       # a hole on the measurement's grid
    return x_T.to(DEV), y.to(DEV), noise.to(DEV), mask


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_operator_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """The fused loop against `_generic_loop` (autograd through `operator.forward` = osmosis::linop_apply and the HIP UNet) on the
    same injected draws.  Bar: the fused-vs-generic bar tests/test_rgb_gpu.py applies to the identity 'ps' chain of the same
    sampler / branch on the tiny 3 -> 6 network (`chain_bar`: min(5 x its measured deviation, 10 x its recorded drift_1e-6)), and
    the 1e-4 it applies to the 4 -> 4 / 4 -> 8 rgb-guidance chains for the 4 -> 8 network."""
    _, gd, M, CM = pkg
    opn, sname, skw, branch, pat_kw, net, masked, ref_tag = CHAIN_CASES[tag]
    case = CHAIN_OPS[opn]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    pat = dict(PATTERN, **pat_kw)
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, sampler.num_timesteps))
    x_T, y, noise, mask = chain_inputs(pkg, case, 1, C, n)
    rg = branch == "rg"
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=rg,
              sample_pattern=pat, measurement_mask=mask if masked else None)
    cond = ps_cond(pkg, case)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = ps_cond(pkg, case, third_party=C == 4)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is None
    if rg:
        _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    # the data term moves the chain (an unguided step would give another image)
    moved = float(max(r["grad"].abs().max() for r in trace))
    print(f"LINOPCHAIN {tag}: fused vs generic {e:.3e} (bar {bar:.3e}); largest guidance gradient {moved:.2e}")
    assert moved > 0.0
    assert e <= bar


def test_new_operators_stay_fused_and_poisson_goes_generic(pkg, monkeypatch, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    for case in CHAIN_OPS.values():
        cond = ps_cond(pkg, case)
        x_T, y, noise, _ = chain_inputs(pkg, case, 1, 3, 10)
        assert sampler._fast_path_ok(model36, cond.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is cond
        poisson = ps_cond(pkg, case, noiser=M.get_noise("poisson", rate=1.0))
        assert sampler._fast_path_ok(model36, poisson.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is None
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    img = sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                index_range=(9, 6))
    assert img.shape == (1, 3, H0, W0) and bool(torch.isfinite(img).all())
    # tiling keeps refusing the 'ps' branch
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              tiling=dict(tile=16, stride=8))
    # a mask must live on the measurement's grid
    with pytest.raises(ValueError, match="measurement.s grid"):
        sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              measurement_mask=torch.ones(1, 1, H0, W0))


def test_batch_of_three_walked_in_chunks_equals_one_pass(pkg, monkeypatch, model36):
    """B = 3 with a measurement-space mask: the one-pass chain, the walk OSM_MAX_BATCH=2 forces (as the existing chunking tests force
    it) and a [2, 1] walk (two engines) agree bit for bit."""
    _, gd, M, CM = pkg
    x_T, y, noise, mask = chain_inputs(pkg, "bicubic4.chain", 3, 3, 10, seed=32)

    def run():
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        cond = ps_cond(pkg, "bicubic4.chain", 3)
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
    """`restore_image` with `super_resolution`: y = noiser(A ref) by default; `simulate: False` takes ref as the measurement, whose
    shape must be the operator's grid for the network's image_size; the result carries the measurement at its own size
    (`save_outputs` beside a smaller measurement: tests/test_linop_cpu.py)."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(41)
    ref = (torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV)

    def cfg(**okw):
        return {"measurement": {"operator": dict(name="super_resolution", scale_factor=4, **okw), "noise": {"name": "gaussian", "sigma": 0.0}},
                "conditioning": {"method": "ps", "params": dict(scale="0.3")},
                "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                                  model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                                  timestep_respacing="4"),
                "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "imagenet"},
                "manual_seed": 0, "rgb_guidance": True}
    res = sampling.restore_image(model36, ref, cfg(), noise_seed=7)[-1]
    op = M.get_operator("super_resolution", device=DEV, scale_factor=4)
    assert res["sample"].shape == (1, 3, H0, W0) and bool(torch.isfinite(res["sample"]).all())
    assert res["measurement"].shape == (1, 3, H0 // 4, W0 // 4) and torch.equal(res["measurement"], op.forward(ref).cpu())
    # the measurement itself: the network's 256 x 256 grid -> 64 x 64
    y = (torch.rand(1, 3, 64, 64, generator=g) * 1.6 - 0.8).to(DEV)
    own = sampling.restore_image(model36, y, cfg(simulate=False), noise_seed=7)[-1]
    assert own["sample"].shape == (1, 3, 256, 256) and bool(torch.isfinite(own["sample"]).all())
    assert torch.equal(own["measurement"], y.cpu())
    with pytest.raises(ValueError, match="simulate"):
        sampling.restore_image(model36, ref, cfg(simulate=False), noise_seed=7)
