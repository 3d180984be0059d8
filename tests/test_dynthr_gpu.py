"""`dynamic_threshold: True` on the fused kernels: the on-device exact quantile of |x| (osm_quantile_abs) vs torch.quantile, the
thresholding backward (osm_dynthr_bwd) vs torch.autograd of the reference's `clip(x * quantile(|x|, 0.98), -1, 1)`
(util/img_utils.py:8-15), and the fused sampler chains vs the REAL reference's (tests/golden/loop_dynthr.npz,
tools/gen_dynthr_golden.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
REVISED = dict(
    operator=dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_a_eta="1e-5", phi_a_learn_flag=True,
                  phi_b="0.95, 0.8, 0.8", phi_b_eta="1e-5", phi_b_learn_flag=True, phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5",
                  phi_inf_learn_flag=True),
    cond=dict(loss_function="norm", loss_weight="depth", weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
              gradient_clip="True,0.005"),
    aux=dict(aux_loss={"avrg_loss": 0.5, "val_loss": 20}))
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20, start_guidance=1,
               stop_guidance=0)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


def make_model(unet, conv_mode=None):
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    m = unet.create_model(**TINY_KW)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    if conv_mode is not None:
        m.conv_mode = conv_mode
    return m


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _free_running_bar(drift):
    """As in test_sampler_gpu.py: tight for well-conditioned chains, the north-star 1e-3 for mildly amplifying ones, None (teacher-forced)
    for chains the reference itself cannot reproduce to 1e-3."""
    if drift <= 1e-4:
        return max(2e-5, 10.0 * drift)
    return 1e-3 if drift <= 1e-3 else None


def _sampler(gd, name, clip_denoised, dynamic_threshold=True):
    return gd.get_sampler(name)(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=dynamic_threshold,
                                clip_denoised=clip_denoised, rescale_timesteps=False)


def _osmosis_cond(M, CM, B=1):
    op = M.get_operator("underwater_physical_revised", device=DEV, batch_size=B, **REVISED["operator"])
    return CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **REVISED["cond"], **PATTERN, **REVISED["aux"])


# ------------------------------------------------------------------------------------------------------------ the select
SIZES = [1, 2, 5, 4096, 4 * 37 * 53, 262144, 8388608, 16777216]
KINDS = ["normal", "quantised", "equal", "zeros", "inf", "nan"]


def _input(kind, n, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, generator=g, device=DEV)
    if kind == "quantised":                        # heavy ties (a few dozen distinct |x|)
        x = torch.round(x * 4.0) / 4.0
    elif kind == "equal":
        x = torch.full((n,), -0.625, device=DEV)
    elif kind == "zeros":                          # +0 and -0 (one key) among quantised values
        x = torch.round(x * 2.0) / 2.0
        x = torch.where(torch.rand(n, generator=g, device=DEV) < 0.5, torch.where(x < 0, -0.0, 0.0), x)
    elif kind == "inf":
        x[::7] = float("inf")
        x[3::11] = -float("inf")
    elif kind == "nan":
        x[n // 2] = float("nan")
    return x.contiguous()


def _bits(t):
    return int(t.reshape(1).view(torch.int32).item())


@pytest.mark.parametrize("n", SIZES)
def test_select_matches_torch_quantile(pkg, n):
    """osm_quantile_abs vs torch.quantile(x.abs(), s) on the device: the two order statistics bit-equal to the stable sort's, q within
    1 ulp (NaN where torch's is NaN), and the indices those of the stable sort (among equal |x|, the (k - #smaller)-th by index)."""
    from osmosis_diffusion_code_amd import ops
    q = torch.empty(1, device=DEV)
    idx = torch.empty(2, device=DEV, dtype=torch.int32)
    ws = ops.quantile_workspace(n, DEV)
    for ki, kind in enumerate(KINDS):
        x = _input(kind, n, 100 + ki)
        a = x.abs()
        srt, order = torch.sort(a, stable=True)
        for s in (0.0, 0.5, 0.98, 1.0):
            ops.quantile_abs(x, s, q, idx, ws)
            want = torch.quantile(a, s)
            r = np.float32(s) * np.float32(n - 1)
            lo, hi = int(np.floor(r)), int(np.ceil(r))
            what = f"n={n} {kind} s={s}"
            if kind == "nan":
                assert torch.isnan(want) and torch.isnan(q).item(), what
                continue
            i0, i1 = (int(v) for v in idx.tolist())
            assert 0 <= i0 < n and 0 <= i1 < n, what
            assert _bits(a[i0]) == _bits(srt[lo]) and _bits(a[i1]) == _bits(srt[hi]), what
            assert (i0, i1) == (int(order[lo]), int(order[hi])), (what, i0, i1, int(order[lo]), int(order[hi]))
            if torch.isnan(want):
                assert torch.isnan(q).item(), what
            else:
                assert abs(_bits(q) - _bits(want)) <= 1, (what, float(q), float(want))


def test_select_refuses_what_torch_quantile_refuses(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    with pytest.raises(_lib.OsmosisHipError, match="too large"):
        ops.quantile_ws_bytes((1 << 24) + 1)
    x = torch.zeros(8, device=DEV)
    with pytest.raises(_lib.OsmosisHipError):
        ops.quantile_abs(x, 1.5, torch.empty(1, device=DEV), torch.empty(2, device=DEV, dtype=torch.int32), ops.quantile_workspace(8, DEV))


# ------------------------------------------------------------------------------------------------------------ the backward
def _autograd(x, w, s=0.98):
    xr = x.clone().requires_grad_(True)
    y = torch.clip(xr * torch.quantile(xr.abs(), s), -1.0, 1.0)
    (dx,) = torch.autograd.grad((y * w).sum(), xr)
    return y.detach(), dx


def _kernel_bwd(x, w, s=0.98):
    from osmosis_diffusion_code_amd import ops
    q, idx = torch.empty(1, device=DEV), torch.empty(2, device=DEV, dtype=torch.int32)
    ws = ops.quantile_workspace(x.numel(), DEV)
    ops.quantile_abs(x, s, q, idx, ws)
    g = w.clone()
    ops.dynthr_bwd(g, x, q, idx, ws, s)
    return g, q


@pytest.mark.parametrize("shape", [(2, 4, 16, 16), (1, 4, 256, 256), (3, 4, 37, 53)])
def test_backward_matches_autograd_tie_free(pkg, shape):
    """d/dx of clip(x * quantile(|x|, 0.98), -1, 1): q m g plus the rank-one term at the two order statistics (autograd differs from
    q m g at exactly those two elements)."""
    g = torch.Generator(device=DEV).manual_seed(5)
    x = 1.3 * torch.randn(*shape, generator=g, device=DEV)
    w = torch.randn(*shape, generator=g, device=DEV)
    _, want = _autograd(x, w)
    got, q = _kernel_bwd(x, w)
    m = ((x * q).abs() <= 1.0).float()
    assert int(((q * m * w) != want).sum()) == 2                   # the rank-one term lands on two elements
    err = float((got - want).abs().max()) / float(want.abs().max())
    print(shape, "backward max rel error", err)
    assert err < 2e-6


def test_backward_with_ties_matches_autograd_per_tied_group(pkg):
    """With ties the order statistic's element is a matter of sort order: compare sum_i sgn(x_i) g_i over each group of equal |x|
    (the rank-one term contributes sgn(x_i)^2 (1-w) S whichever member carries it) and every element outside the two selected groups."""
    g = torch.Generator(device=DEV).manual_seed(6)
    x = torch.round(4.0 * 1.3 * torch.randn(2, 4, 64, 64, generator=g, device=DEV)) / 4.0
    w = torch.randn(2, 4, 64, 64, generator=g, device=DEV)
    _, want = _autograd(x, w)
    got, q = _kernel_bwd(x, w)
    a, sg = x.abs().flatten(), torch.sign(x).flatten()
    keys, inv = torch.unique(a, return_inverse=True)
    gs = torch.zeros(keys.numel(), device=DEV, dtype=torch.float64).index_add_(0, inv, (sg * got.flatten()).double())
    ws = torch.zeros(keys.numel(), device=DEV, dtype=torch.float64).index_add_(0, inv, (sg * want.flatten()).double())
    scale = float(want.abs().max())
    assert float((gs - ws).abs().max()) / scale < 2e-6
    m = ((x * q).abs() <= 1.0).float()
    direct = (q * m * w).flatten()
    sel = (got.flatten() != direct) | (want.flatten() != direct)
    keep = ~torch.isin(inv, torch.unique(inv[sel]))
    assert torch.equal(got.flatten()[keep], want.flatten()[keep])


@pytest.mark.parametrize("tag", ["free", "ties"])
def test_forward_and_vjp_match_the_reference_vectors(pkg, tag):
    """The reference's own dynamic_thresholding (forward and VJP, torch-CPU) on the fixture's seeded tensors, through
    osmosis::posterior_dynthr (start_x: x0_raw = the network output) and osmosis::dynthr_bwd."""
    from osmosis_diffusion_code_amd import torch_ops  # noqa: F401  (registers osmosis::)
    g = np.load(os.path.join(GOLD, "loop_dynthr.npz"))
    x, w = (torch.from_numpy(g[f"px.{tag}.{k}"]).to(DEV) for k in ("x", "w"))
    coef = torch.tensor([0.0, -1.0, 0.5, 0.25, 0.0, 0.0, 1.0, 0.0], device=DEV)         # start_x row: x0 = out
    model_out = torch.cat([x, torch.zeros_like(x)], dim=1).contiguous()
    x0, mean, _lv, raw, q, idx = torch.ops.osmosis.posterior_dynthr(model_out, torch.zeros_like(x), coef, 1, 1, 0.98)
    assert torch.equal(raw, x)
    assert abs(_bits(q) - _bits(torch.from_numpy(g[f"px.{tag}.q"]))) <= 1
    assert float((x0.cpu() - torch.from_numpy(g[f"px.{tag}.y"])).abs().max()) <= 1e-6
    assert torch.equal(mean, 0.5 * x0)
    dx = torch.ops.osmosis.dynthr_bwd(w, raw, q, idx, 0.98).cpu()
    want = torch.from_numpy(g[f"px.{tag}.dx"])
    if tag == "free":
        assert float((dx - want).abs().max()) / float(want.abs().max()) < 2e-6
    else:
        xs = torch.from_numpy(g["px.ties.x"])
        _, inv = torch.unique(xs.abs().flatten(), return_inverse=True)
        n = int(inv.max()) + 1
        sd = torch.zeros(n, dtype=torch.float64).index_add_(0, inv, (torch.sign(xs).flatten() * dx.flatten()).double())
        sw = torch.zeros(n, dtype=torch.float64).index_add_(0, inv, (torch.sign(xs).flatten() * want.flatten()).double())
        assert float((sd - sw).abs().max()) / float(want.abs().max()) < 2e-6


def test_new_operators_opcheck(pkg):
    from osmosis_diffusion_code_amd import torch_ops  # noqa: F401
    g = torch.Generator(device=DEV).manual_seed(8)
    x = torch.randn(2, 4, 16, 16, generator=g, device=DEV)
    model_out = torch.randn(2, 8, 16, 16, generator=g, device=DEV)
    sampler = pkg[1].create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                                    model_var_type="learned_range", dynamic_threshold=True, clip_denoised=False,
                                    rescale_timesteps=False, timestep_respacing=1000)
    coef = torch.from_numpy(sampler.coef_table()[120].copy()).to(DEV)
    torch.library.opcheck(torch.ops.osmosis.quantile_abs.default, (x, 0.98))
    torch.library.opcheck(torch.ops.osmosis.posterior_dynthr.default, (model_out, x, coef, 0, 0, 0.98))
    _x0, _m, _lv, raw, q, idx = torch.ops.osmosis.posterior_dynthr(model_out, x, coef)
    torch.library.opcheck(torch.ops.osmosis.dynthr_bwd.default, (torch.randn_like(x), raw, q, idx, 0.98))


# ------------------------------------------------------------------------------------------------------------ the fused chains
@pytest.mark.parametrize("conv_mode", ["f32", "f16x3"])
@pytest.mark.parametrize("clip", [0, 1])
def test_fused_osmosis_loop_with_dynamic_threshold_matches_the_reference(pkg, monkeypatch, conv_mode, clip):
    """The Osmosis loop with `dynamic_threshold: True` (clip_denoised off / on) on the fused kernels -- osm_posterior_dynthr and
    osm_dynthr_bwd in place of the posterior and the clamp's backward -- vs the REAL reference: per-step pred_xstart, guidance gradient,
    loss and q, final image and phi."""
    unet, gd, M, CM = pkg
    g, base = np.load(os.path.join(GOLD, "loop_dynthr.npz")), np.load(os.path.join(GOLD, "loop_underwater_physical_revised.npz"))
    tag = f"osmosis.clip{clip}"
    model = make_model(unet, conv_mode)
    cond = _osmosis_cond(M, CM)
    sampler = _sampler(gd, "ddpm", bool(clip))
    _no_generic(monkeypatch, sampler)
    noise = torch.from_numpy(base["noise"]).to(DEV)
    bar = _free_running_bar(float(g[f"{tag}.drift_1e-6"]))
    assert bar is not None
    trace = []
    img, variables, loss, x0 = sampler.p_sample_loop(
        model=model, x_start=torch.from_numpy(base["x_T"]).to(DEV), measurement=torch.from_numpy(base["y"]).to(DEV),
        measurement_cond_fn=cond.conditioning, record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False,
        sample_pattern=PATTERN, noise_fn=lambda k, shape: noise[k], trace=trace)
    assert len(trace) == 10
    e_x0 = max(float((r["x0"].cpu() - torch.from_numpy(g[f"{tag}.x0"][k])).abs().max()) for k, r in enumerate(trace))
    e_g = max(float((r["grad"].cpu() - torch.from_numpy(g[f"{tag}.grad"][k])).abs().max()) / float(np.abs(g[f"{tag}.grad"][k]).max())
              for k, r in enumerate(trace))
    e_loss = max(abs(float(r["loss"][0]) - float(g[f"{tag}.loss"][k].reshape(-1)[0])) / float(g[f"{tag}.loss"][k].reshape(-1)[0])
                 for k, r in enumerate(trace))
    e_q = max(abs(float(r["q"][0]) - float(g[f"{tag}.q"][k])) / float(g[f"{tag}.q"][k]) for k, r in enumerate(trace))
    e_img = float((img.cpu() - torch.from_numpy(g[f"{tag}.final_img"])).abs().max())
    print(f"{tag} {conv_mode}: x0 {e_x0:.1e} grad(rel) {e_g:.1e} loss(rel) {e_loss:.1e} q(rel) {e_q:.1e} final img {e_img:.1e}")
    assert max(float(r["x0"].abs().max()) for r in trace) == 1.0            # the threshold clips
    assert e_x0 < 5e-5 and e_g < 5e-5 and e_loss < 1e-5 and e_q < 1e-5 and e_img < bar
    for n, v in variables.items():
        assert torch.allclose(v.cpu(), torch.from_numpy(g[f"{tag}.{n}"]), atol=2e-6), n


@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_fused_rgb_guidance_chain_with_dynamic_threshold_matches_the_reference(pkg, monkeypatch, name):
    unet, gd, M, CM = pkg
    g, ps = np.load(os.path.join(GOLD, "loop_dynthr.npz")), np.load(os.path.join(GOLD, "loop_ps.npz"))
    model = make_model(unet)
    cond = CM.get_conditioning_method("ps", M.get_operator("rgb_guidance", device=DEV, batch_size=1),
                                      M.get_noise("gaussian", sigma=0.05), scale="0.6,0.5,0.4,0.0")
    sampler = _sampler(gd, name, False)
    _no_generic(monkeypatch, sampler)
    draws = torch.from_numpy(ps[f"{name}.draws_x"]).to(DEV)
    bar = _free_running_bar(float(g[f"ps.{name}.drift_1e-6"]))
    assert bar is not None
    trace = []
    img = sampler.p_sample_loop(model=model, x_start=torch.from_numpy(ps[f"{name}.x_T"]).to(DEV),
                                measurement=torch.from_numpy(ps[f"{name}.y"]).to(DEV), measurement_cond_fn=cond.conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=True, sample_pattern=PATTERN,
                                noise_fn=lambda k, shape: draws[k], trace=trace)
    losses = [float(r["loss"][0]) for r in trace]
    qs = [float(r["q"][0]) for r in trace]
    assert np.allclose(losses, g[f"ps.{name}.loss"], rtol=1e-5), (losses, g[f"ps.{name}.loss"])
    assert np.allclose(qs, g[f"ps.{name}.q"], rtol=1e-5), (qs, g[f"ps.{name}.q"])
    err = float((img.cpu() - torch.from_numpy(g[f"ps.{name}.final_img"])).abs().max())
    print(f"ps.{name} dynamic_threshold: free-running chain max-abs error {err:.1e}, bar {bar:.1e}")
    assert err < bar


def _b2_inputs():
    gen = torch.Generator().manual_seed(44)
    x_T = 0.5 * torch.randn(2, 4, 32, 32, generator=gen)
    y = torch.rand(2, 3, 32, 32, generator=gen) * 1.6 - 0.8
    noise = torch.randn(10, 2, 4, 32, 32, generator=gen)
    return x_T.to(DEV), y.to(DEV), noise.to(DEV)


def _run_b2(pkg, monkeypatch, fused):
    unet, gd, M, CM = pkg
    model = make_model(unet, "f32")
    cond = _osmosis_cond(M, CM, B=2)
    sampler = _sampler(gd, "ddpm", False)
    x_T, y, noise = _b2_inputs()
    kw = dict(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False, save_root=None,
              pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN)
    if fused:
        _no_generic(monkeypatch, sampler)
        out = sampler.p_sample_loop(noise_fn=lambda k, shape: noise[k], **kw)
    else:
        monkeypatch.setenv("OSM_FUSED_DYNTHR", "0")
        draws = iter(noise)
        orig = torch.randn_like

        def replay(t, **k):                       # the step noise of the fused run; q_sample's draw is unused
            return next(draws).clone() if t.shape[1] == 4 else orig(t, **k)
        monkeypatch.setattr(torch, "randn_like", replay)
        out = sampler.p_sample_loop(**kw)
    monkeypatch.undo()
    return out


def test_batch_of_two_fused_equals_the_generic_loop(pkg, monkeypatch):
    """B = 2 (the quantile couples both images): the fused loop and `_generic_loop` (torch.quantile + autograd over the HIP UNet) with
    the same injected noise."""
    f_img, f_vars, f_loss, f_x0 = _run_b2(pkg, monkeypatch, True)
    g_img, g_vars, g_loss, g_x0 = _run_b2(pkg, monkeypatch, False)
    e_img = float((f_img.cpu() - g_img.detach().cpu()).abs().max())
    e_x0 = float((f_x0 - g_x0).abs().max())
    print(f"B=2 fused vs generic: img {e_img:.1e} x0 {e_x0:.1e}")
    assert e_img < 1e-4 and e_x0 < 1e-4
    assert np.allclose(f_loss, g_loss, rtol=1e-5)
    for n in f_vars:
        assert torch.allclose(f_vars[n].cpu(), g_vars[n].detach().cpu(), atol=1e-6), n


class _Generic(Exception):
    pass


def _routes_to_generic(pkg, monkeypatch, B):
    unet, gd, M, CM = pkg
    model = make_model(unet)
    cond = _osmosis_cond(M, CM, B=B)
    sampler = _sampler(gd, "ddpm", False)

    def generic(*a, **k):
        raise _Generic()
    monkeypatch.setattr(type(sampler), "_generic_loop", generic)
    x_T, y, _noise = _b2_inputs()
    try:
        sampler.p_sample_loop(model=model, x_start=x_T[:B], measurement=y[:B], measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: torch.zeros(shape, device=DEV), index_range=(9, 9))
    except _Generic:
        return True
    return False


def test_routing_of_dynamic_threshold_chains(pkg, monkeypatch):
    """One engine pass: fused.  A chunked batch (the quantile would span chunks) and OSM_FUSED_DYNTHR=0: `_generic_loop`."""
    assert not _routes_to_generic(pkg, monkeypatch, 1)
    monkeypatch.setenv("OSM_MAX_BATCH", "1")
    assert _routes_to_generic(pkg, monkeypatch, 2)
    monkeypatch.delenv("OSM_MAX_BATCH")
    assert not _routes_to_generic(pkg, monkeypatch, 2)
    monkeypatch.setenv("OSM_FUSED_DYNTHR", "0")
    assert _routes_to_generic(pkg, monkeypatch, 1)
