"""The PCGS inner alternation (`local_M > 1`: the step repeated `alternate_len` times at the same t inside [s_end, s_start],
gaussian_diffusion.py:225-309) on the fused loop: the sub-step noise of the library stream (counter word 2 = step | sub << 16), the
fused Osmosis and rgb-guidance chains vs the REAL reference (tests/golden/loop_pcgs.npz, tools/gen_pcgs_golden.py) and vs
`_generic_loop`, the trace / step counter / record bookkeeping, batches and chunks, routing."""
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
STREAM = 0x6f736d31                                  # "osm1": word 3 of the step-noise counter
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
COND = dict(loss_function="norm", loss_weight="depth", weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
            gradient_clip="True,0.005")
AUX = dict(aux_loss={"avrg_loss": 0.5, "val_loss": 20})
OPERATORS = {
    "revised": ("underwater_physical_revised",
                dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_a_eta="1e-5",
                     phi_a_learn_flag=True, phi_b="0.95, 0.8, 0.8", phi_b_eta="1e-5", phi_b_learn_flag=True,
                     phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True)),
    "haze": ("haze_physical",
             dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_ab_eta="1e-5", phi_ab_learn_flag=True,
                  phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True)),
}
WINDOWS = {"w62": (0.6, 0.2), "w50": (0.5, 0.0)}


def pattern(win, local_M):
    s_start, s_end = WINDOWS[win]
    return dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=local_M, s_start=s_start, s_end=s_end, n_iter=20,
                start_guidance=1, stop_guidance=0)


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


@pytest.fixture(scope="module")
def gold():
    return np.load(os.path.join(GOLD, "loop_pcgs.npz"))


def make_model(unet, conv_mode=None):
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    m = unet.create_model(**TINY_KW)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    if conv_mode is not None:
        m.conv_mode = conv_mode
    return m


def make_sampler(gd, name="ddpm"):
    return gd.get_sampler(name)(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False,
                                clip_denoised=False, rescale_timesteps=False)


def osmosis_cond(M, CM, op, pat, B=1):
    name, okw = OPERATORS[op]
    operator = M.get_operator(name, device=DEV, batch_size=B, **okw)
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **pat, **AUX)


def ps_cond(M, CM, B=1):
    return CM.get_conditioning_method("ps", M.get_operator("rgb_guidance", device=DEV, batch_size=B),
                                      M.get_noise("gaussian", sigma=0.05), scale="0.6,0.5,0.4,0.0")


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _free_running_bar(drift):
    """As in test_dynthr_gpu.py: tight for well-conditioned chains, the north-star 1e-3 for mildly amplifying ones, None
    (teacher-forced) for chains the reference itself cannot reproduce to 1e-3."""
    if drift <= 1e-4:
        return max(2e-5, 10.0 * drift)
    return 1e-3 if drift <= 1e-3 else None


def sub_steps(gd, pat, T=10):
    """[(idx, sub)] of a chain in call order."""
    return [(T - 1 - j, s) for j, (_, _, a) in enumerate(gd.pcgs_schedule(pat, T)) for s in range(a)]


# ------------------------------------------------------------------------------------------------------------ the sub-step noise
def philox_np(c, k):
    c, k = [int(v) for v in c], [int(v) for v in k]
    for _ in range(10):
        p0, p1 = 0xD2511F53 * c[0], 0xCD9E8D57 * c[2]
        c = [(p1 >> 32) ^ c[1] ^ k[0], p1 & 0xffffffff, (p0 >> 32) ^ c[3] ^ k[1], p0 & 0xffffffff]
        k = [(k[0] + 0x9E3779B9) & 0xffffffff, (k[1] + 0xBB67AE85) & 0xffffffff]
    return tuple(c)


def normal4_np(r):
    """The kernel's Box-Muller on one counter's four words: 24-bit uniforms centred in their cell and the angle, rounded to float32
    as the kernel forms them; log / sqrt / sin / cos in float64."""
    f = np.float32
    u = [f(w >> 8) * f(5.9604644775390625e-8) + f(2.98023223876953125e-8) for w in r]
    r0, r1 = np.sqrt(-2.0 * np.log(np.float64(u[0]))), np.sqrt(-2.0 * np.log(np.float64(u[2])))
    a0, a1 = (np.float64(f(6.283185307179586) * u[i]) for i in (1, 3))
    return np.array([r0 * np.cos(a0), r0 * np.sin(a0), r1 * np.cos(a1), r1 * np.sin(a1)])


def test_sub_zero_is_the_plain_stream_and_sub_follows_the_documented_counter(pkg):
    """osm_randn_sub / osm_guide_update_rng_sub at sub = 0 are bit-equal to osm_randn / osm_guide_update_rng; at sub != 0 the draws
    are Philox-4x32-10 at counter (element / 4, image, step | sub << 16, "osm1"), key = seed, restated in numpy."""
    from osmosis_diffusion_code_amd import ops
    B, H, W = 2, 16, 24
    HW, n = H * W, 4 * H * W
    seed = 0x0123456789ABCDEF
    a, b = torch.empty(B, n, device=DEV), torch.empty(B, n, device=DEV)
    ops.randn(a, B, n, seed, step_const=7, img0=3)
    ops.randn_sub(b, B, n, seed, step_const=7, sub=0, img0=3)
    assert torch.equal(a, b)
    step = torch.tensor([7], device=DEV, dtype=torch.int32)
    ops.randn_sub(b, B, n, seed, step=step, sub=0, img0=3)
    assert torch.equal(a, b)
    # the update kernel, with guidance and a stride-0 (shared) image index
    g = torch.Generator(device=DEV).manual_seed(3)
    mean, lv, gg, dxu = (torch.randn(B, 4, H, W, generator=g, device=DEV) for _ in range(4))
    lv = lv - 3.0
    coef = torch.tensor([0.9, 0.1, 0.5, 0.5, 0.0, 0.0, 1.0, 7.0], device=DEV)
    scale4 = torch.tensor([7.0, 7.0, 7.0, 0.9], device=DEV)
    outs = []
    for fn, extra in ((ops.guide_update_rng, {}), (ops.guide_update_rng_sub, {"sub": 0})):
        x_next, grad, used = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
        fn(mean, lv, gg, dxu, coef, scale4, 0.005, x_next, grad, used, B, HW, seed, step, step_offset=1, img0=5, img_stride=0, **extra)
        outs.append((x_next, grad, used))
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    # sub != 0: a few quads against the restatement
    k0, k1 = seed & 0xffffffff, seed >> 32
    for sub, st, img0 in ((1, 7, 0), (2, 7, 4), (5, 999, 1), (65535, 0, 2)):
        z = torch.empty(B, n, device=DEV)
        ops.randn_sub(z, B, n, seed, step_const=st, sub=sub, img0=img0)
        raw = torch.zeros(4 * HW, device=DEV, dtype=torch.int32)
        ops.philox_raw(raw, HW, img0 + 1, st | sub << 16, STREAM, k0, k1)
        raw = raw.view(HW, 4).cpu().numpy().astype(np.uint32)
        for q in (0, 1, 17, HW - 1):
            want = philox_np((q, img0 + 1, st | sub << 16, STREAM), (k0, k1))
            assert tuple(int(v) for v in raw[q]) == want
            got = z[1, 4 * q:4 * q + 4].cpu().double().numpy()
            assert np.allclose(got, normal4_np(want), rtol=1e-5, atol=1e-5), (sub, st, q, got, normal4_np(want))
        # the update kernel draws the same at the same (step, sub): step word = *step + step_offset
        used = torch.empty(B, 4, H, W, device=DEV)
        ops.guide_update_rng_sub(mean, lv, None, None, coef, None, -1.0, torch.empty_like(mean), None, used, B, HW, seed,
                                 torch.tensor([st - 1], device=DEV, dtype=torch.int32), step_offset=1, sub=sub, img0=img0)
        assert torch.equal(used.view(B, n), z)
        ops.randn_sub(a, B, n, seed, step_const=st, sub=0, img0=img0)
        assert not torch.equal(a, z)


def test_sub_argument_is_checked(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    z = torch.empty(1, 64, device=DEV)
    with pytest.raises(_lib.OsmosisHipError, match="sub"):
        ops.randn_sub(z, 1, 64, 1, step_const=3, sub=65536)
    with pytest.raises(_lib.OsmosisHipError, match="sub"):
        ops.randn_sub(z, 1, 64, 1, step_const=3, sub=-1)
    with pytest.raises(_lib.OsmosisHipError, match="step"):
        ops.randn_sub(z, 1, 64, 1, step_const=65536, sub=1)


@pytest.mark.parametrize("sub", [1, 2])
def test_sub_step_noise_moments_and_independence(pkg, sub):
    """N(0, 1) moments at sub = 1, 2; |corr| < 4 / sqrt(n) against sub = 0 of the same step, the same sub of the neighbouring steps and
    sub = 0 of the neighbouring steps."""
    from osmosis_diffusion_code_amd import ops
    n = 4 * 256 * 256
    seed, st = 4321, 500

    def draw(step, s):
        z = torch.empty(1, n, device=DEV)
        ops.randn_sub(z, 1, n, seed, step_const=step, sub=s, img0=0)
        return z[0].double()
    z = draw(st, sub)
    assert abs(float(z.mean())) < 4e-3 and abs(float(z.var()) - 1.0) < 6e-3
    assert abs(float((z ** 3).mean())) < 2e-2 and abs(float((z ** 4).mean()) - 3.0) < 5e-2
    assert torch.isfinite(z).all() and float(z.abs().max()) < 6.5
    bar = 4.0 / np.sqrt(n)
    for other in ((st, 0), (st - 1, sub), (st + 1, sub), (st - 1, 0), (st + 1, 0), (st, sub + 1)):
        c = float((z * draw(*other)).mean())
        assert abs(c) < bar, (other, c)


# ------------------------------------------------------------------------------------------------------------ the fused chains
def _osmosis_run(pkg, monkeypatch, tag, gold, conv_mode="f32", **kw):
    unet, gd, M, CM = pkg
    _, op, win = tag.split(".")
    pat = pattern(win, 3)
    model = make_model(unet, conv_mode)
    cond = osmosis_cond(M, CM, op, pat)
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    noise = torch.from_numpy(gold[f"{tag}.noise"]).to(DEV)
    trace = []
    out = sampler.p_sample_loop(
        model=model, x_start=torch.from_numpy(gold[f"{tag}.x_T"]).to(DEV), measurement=torch.from_numpy(gold[f"{tag}.y"]).to(DEV),
        measurement_cond_fn=cond.conditioning, record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False,
        sample_pattern=pat, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    return out, trace, cond, pat


@pytest.mark.parametrize("conv_mode", ["f32", "f16x3"])
@pytest.mark.parametrize("tag", ["osm.revised.w62", "osm.revised.w50", "osm.haze.w62"])
def test_fused_osmosis_pcgs_chain_matches_the_reference(pkg, monkeypatch, gold, conv_mode, tag):
    """The Osmosis loop with local_M = 3 on the fused kernels vs the REAL reference: per sub-step pred_xstart, guidance gradient, loss
    and phi (each sub-step runs its own n_iter = 20 phi steps), final image, pred_xstart and phi."""
    gd = pkg[1]
    (img, variables, loss, x0), trace, cond, pat = _osmosis_run(pkg, monkeypatch, tag, gold, conv_mode)
    n = len(gold[f"{tag}.loss"])
    assert len(trace) == n and [(r["idx"], r["sub"]) for r in trace] == sub_steps(gd, pat)
    bar = _free_running_bar(float(gold[f"{tag}.drift_1e-6"]))
    assert bar is not None
    slots = cond.operator._slots()
    e_x0 = e_g = e_loss = e_phi = 0.0
    for k, r in enumerate(trace):
        e_x0 = max(e_x0, float((r["x0"][..., ::2, ::2].cpu() - torch.from_numpy(gold[f"{tag}.x0_s2"][k])).abs().max()))
        want_g = gold[f"{tag}.grad_s2"][k]
        e_g = max(e_g, float((r["grad"][..., ::2, ::2].cpu() - torch.from_numpy(want_g)).abs().max()) / float(np.abs(want_g).max()))
        want_l = float(gold[f"{tag}.loss"][k].reshape(-1)[0])
        e_loss = max(e_loss, abs(float(r["loss"][0]) - want_l) / want_l)
        for name, (off, m) in slots.items():
            got = r["phi"][0, off:off + m].cpu().numpy()
            e_phi = max(e_phi, float(np.abs(got - gold[f"{tag}.phi.{name}"][k].reshape(-1)).max()))
    e_img = float((img.cpu() - torch.from_numpy(gold[f"{tag}.final_img"])).abs().max())
    e_fx0 = float((x0 - torch.from_numpy(gold[f"{tag}.final_x0"])).abs().max())
    print(f"{tag} {conv_mode}: x0 {e_x0:.1e} grad(rel) {e_g:.1e} loss(rel) {e_loss:.1e} phi {e_phi:.1e} final img {e_img:.1e} "
          f"x0 {e_fx0:.1e} (bar {bar:.1e})")
    assert e_x0 < 1e-4 and e_g < 1e-4 and e_loss < 2e-5 and e_phi < 2e-6
    assert e_img < bar and e_fx0 < bar
    assert np.allclose(loss, gold[f"{tag}.loss"][-1].reshape(-1), rtol=2e-5)
    for name, v in variables.items():
        assert torch.allclose(v.cpu(), torch.from_numpy(gold[f"{tag}.final.{name}"]), atol=2e-6), name


@pytest.mark.parametrize("name", ["ddpm", "ddim"])
def test_fused_rgb_guidance_pcgs_chain_matches_the_reference(pkg, monkeypatch, gold, name):
    """`ps` through DDPM.p_sample / DDIM.p_sample with local_M = 2 in [0, 0.5] (index 0 alternates: no noise there) vs the REAL
    reference: per sub-step loss, final image."""
    unet, gd, M, CM = pkg
    tag = f"ps.{name}"
    pat = pattern("w50", 2)
    model = make_model(unet)
    sampler = make_sampler(gd, name)
    _no_generic(monkeypatch, sampler)
    draws = torch.from_numpy(gold[f"{tag}.draws_x"]).to(DEV)
    bar = _free_running_bar(float(gold[f"{tag}.drift_1e-6"]))
    assert bar is not None
    trace = []
    img = sampler.p_sample_loop(model=model, x_start=torch.from_numpy(gold[f"{tag}.x_T"]).to(DEV),
                                measurement=torch.from_numpy(gold[f"{tag}.y"]).to(DEV), measurement_cond_fn=ps_cond(M, CM).conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=True, sample_pattern=pat,
                                noise_fn=lambda k, shape: draws[k], trace=trace)
    assert [(r["idx"], r["sub"]) for r in trace] == sub_steps(gd, pat) and len(trace) == len(gold[f"{tag}.loss"])
    losses = [float(r["loss"][0]) for r in trace]
    assert np.allclose(losses, gold[f"{tag}.loss"], rtol=1e-5), (losses, gold[f"{tag}.loss"])
    err = float((img.cpu() - torch.from_numpy(gold[f"{tag}.final_img"])).abs().max())
    print(f"{tag} local_M = 2: free-running chain max-abs error {err:.1e}, bar {bar:.1e}")
    assert err < bar


def _replay_randn_like(monkeypatch, noise):
    """torch.randn_like for `_generic_loop`: the 4-channel draws (step / p_sample noise) replay `noise`, the rest draw as usual."""
    draws, orig = iter(noise), torch.randn_like

    def replay(t, **k):
        return next(draws).clone() if t.shape[1] == 4 else orig(t, **k)
    monkeypatch.setattr(torch, "randn_like", replay)


@pytest.mark.parametrize("branch", ["osmosis", "ddpm", "ddim"])
def test_fused_equals_the_generic_loop(pkg, monkeypatch, gold, branch):
    """The fused chain and `_generic_loop` (OSM_FUSED_PCGS=0: autograd over the HIP UNet, the reference's control flow) on the same
    injected noise."""
    unet, gd, M, CM = pkg
    model = make_model(unet, "f32")
    tag = "osm.revised.w62" if branch == "osmosis" else f"ps.{branch}"
    pat = pattern("w62", 3) if branch == "osmosis" else pattern("w50", 2)
    noise = torch.from_numpy(gold[f"{tag}.noise" if branch == "osmosis" else f"{tag}.draws_x"]).to(DEV)
    x_T, y = torch.from_numpy(gold[f"{tag}.x_T"]).to(DEV), torch.from_numpy(gold[f"{tag}.y"]).to(DEV)

    def run(fused):
        sampler = make_sampler(gd, "ddpm" if branch == "osmosis" else branch)
        cond = osmosis_cond(M, CM, "revised", pat) if branch == "osmosis" else ps_cond(M, CM)
        kw = dict(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False, save_root=None,
                  pretrain_model="osmosis", rgb_guidance=branch != "osmosis", sample_pattern=pat)
        if fused:
            _no_generic(monkeypatch, sampler)
            out = sampler.p_sample_loop(noise_fn=lambda k, shape: noise[k], **kw)
        else:
            monkeypatch.setenv("OSM_FUSED_PCGS", "0")
            assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", branch != "osmosis", pat, tuple(x_T.shape)) is None
            _replay_randn_like(monkeypatch, noise)
            out = sampler.p_sample_loop(**kw)
        monkeypatch.undo()
        return out
    f, g = run(True), run(False)
    if branch != "osmosis":
        e = float((f.cpu() - g.detach().cpu()).abs().max())
        print(f"{branch}: fused vs generic img {e:.1e}")
        assert e < 1e-4
        return
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    print(f"osmosis: fused vs generic img {e_img:.1e} x0 {e_x0:.1e}")
    assert e_img < 1e-4 and e_x0 < 1e-4
    assert np.allclose(f[2], g[2], rtol=1e-5)
    for n in f[1]:
        assert torch.allclose(f[1][n].cpu(), g[1][n].detach().cpu(), atol=1e-6), n


@pytest.mark.parametrize("branch", ["osmosis", "ddpm"])
def test_aten_noise_draws_the_generic_loops_realisation(pkg, monkeypatch, gold, branch):
    """noise="aten" in the fused loop draws the reference's order per sub-step (Osmosis: q_sample, then the step noise; `ps`: p_sample,
    then q_sample) on torch's device generator: with the same torch.manual_seed it lands where `_generic_loop` lands."""
    unet, gd, M, CM = pkg
    model = make_model(unet, "f32")
    tag = "osm.revised.w62" if branch == "osmosis" else "ps.ddpm"
    pat = pattern("w62", 3) if branch == "osmosis" else pattern("w50", 2)
    x_T, y = torch.from_numpy(gold[f"{tag}.x_T"]).to(DEV), torch.from_numpy(gold[f"{tag}.y"]).to(DEV)

    def run(fused):
        sampler = make_sampler(gd, "ddpm")
        cond = osmosis_cond(M, CM, "revised", pat) if branch == "osmosis" else ps_cond(M, CM)
        kw = dict(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False, save_root=None,
                  pretrain_model="osmosis", rgb_guidance=branch != "osmosis", sample_pattern=pat)
        if fused:
            _no_generic(monkeypatch, sampler)
            kw["noise"] = "aten"
        else:
            monkeypatch.setenv("OSM_FUSED_PCGS", "0")
        torch.manual_seed(11)
        out = sampler.p_sample_loop(**kw)
        monkeypatch.undo()
        return out[0] if branch == "osmosis" else out
    f, g = run(True), run(False)
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    print(f"{branch}: aten fused vs generic img {e:.1e}")
    assert e < 1e-4


# ------------------------------------------------------------------------------------------------------------ bookkeeping
def test_trace_counter_and_records(pkg, monkeypatch, gold):
    """One trace record per sub-step (idx, sub); the device step counter stays at idx through the non-final sub-steps and ends where a
    local_M = 1 chain ends; the library stream gives every sub-step its own noise (counter word 2 = idx | sub << 16); `record`
    snapshots are taken once per index, after its last sub-step."""
    from osmosis_diffusion_code_amd import ops
    unet, gd, M, CM = pkg
    model = make_model(unet, "f32")
    tag = "osm.revised.w62"
    x_T, y = torch.from_numpy(gold[f"{tag}.x_T"]).to(DEV), torch.from_numpy(gold[f"{tag}.y"]).to(DEV)
    seed = 99

    def run(pat, **kw):
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        trace, records = [], []
        sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=osmosis_cond(M, CM, "revised", pat).conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat,
                              noise_seed=seed, trace=trace, record_out=records, record_every=1, **kw)
        monkeypatch.undo()
        return trace, records
    pat = pattern("w50", 3)
    trace, records = run(pat)
    assert [(r["idx"], r["sub"]) for r in trace] == sub_steps(gd, pat)
    steps = [int(r["step"].item()) for r in trace]
    alt = {idx: a for idx, (_, _, a) in zip(range(9, -1, -1), gd.pcgs_schedule(pat, 10))}
    assert steps == [r["idx"] - 1 if r["sub"] == alt[r["idx"]] - 1 else r["idx"] for r in trace]
    plain, _ = run(pattern("w50", 1))
    assert len(plain) == 10 and int(plain[-1]["step"].item()) == steps[-1] == -1
    short, _ = run(pat, index_range=(6, 3))
    assert [(r["idx"], r["sub"]) for r in short] == [s for s in sub_steps(gd, pat) if 3 <= s[0] <= 6]
    assert int(short[-1]["step"].item()) == 2
    # the noise of every sub-step is its own stream, none at index 0
    z = torch.empty(1, 4 * 16 * 16, device=DEV)
    for r in trace:
        if r["idx"] == 0:
            assert float(r["noise"].abs().max()) == 0.0
            continue
        ops.randn_sub(z, 1, z.shape[1], seed, step_const=r["idx"], sub=r["sub"], img0=0)
        assert torch.equal(r["noise"].reshape(1, -1), z), (r["idx"], r["sub"])
    # records: one per index, pred_xstart of its last sub-step
    assert [i for i, _ in records] == list(range(9, -1, -1))
    last = {r["idx"]: r for r in trace}
    for idx, x0 in records:
        assert torch.equal(x0, last[idx]["x0"].cpu()), idx


# ------------------------------------------------------------------------------------------------------------ batches and chunks
def _batch_inputs():
    gen = torch.Generator().manual_seed(45)
    return (0.5 * torch.randn(2, 4, 16, 16, generator=gen)).to(DEV), (torch.rand(2, 3, 16, 16, generator=gen) * 1.6 - 0.8).to(DEV)


def _lib_chain(pkg, monkeypatch, sl, **kw):
    unet, gd, M, CM = pkg
    pat = pattern("w62", 2)
    x_T, y = _batch_inputs()
    model = make_model(unet, "f32")
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    cond = osmosis_cond(M, CM, "revised", pat, B=sl.stop - sl.start)
    out = sampler.p_sample_loop(model=model, x_start=x_T[sl], measurement=y[sl], measurement_cond_fn=cond.conditioning, record=False,
                                save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat, noise_seed=5, **kw)
    monkeypatch.undo()
    return out


def test_batch_of_two_equals_two_single_images(pkg, monkeypatch):
    """B = 2 with local_M = 2 and the library stream equals two batch-1 chains (image_index0 = the image's index)."""
    both = _lib_chain(pkg, monkeypatch, slice(0, 2))
    for i in range(2):
        one = _lib_chain(pkg, monkeypatch, slice(i, i + 1), image_index0=i)
        assert float((both[0][i:i + 1] - one[0]).abs().max()) < 2e-5
        assert float((both[3][i:i + 1] - one[3]).abs().max()) < 2e-5
        assert np.allclose(both[2][i], one[2][0], rtol=1e-5)
        for n in both[1]:
            assert torch.allclose(both[1][n][i:i + 1], one[1][n], atol=1e-6), n


def test_chunked_walk_equals_one_pass(pkg, monkeypatch):
    """The same B = 2 chain walked in two chunks of one image (OSM_MAX_BATCH=1) equals the one-pass chain."""
    whole = _lib_chain(pkg, monkeypatch, slice(0, 2))
    os.environ["OSM_MAX_BATCH"] = "1"
    try:
        chunked = _lib_chain(pkg, monkeypatch, slice(0, 2))
    finally:
        os.environ.pop("OSM_MAX_BATCH", None)
    assert float((whole[0] - chunked[0]).abs().max()) < 2e-5
    assert float((whole[3] - chunked[3]).abs().max()) < 2e-5
    assert np.allclose(whole[2], chunked[2], rtol=1e-5)
    for n in whole[1]:
        assert torch.allclose(whole[1][n], chunked[1][n], atol=1e-6), n


# ------------------------------------------------------------------------------------------------------------ routing
def test_routing_of_pcgs_chains(pkg, monkeypatch):
    """local_M > 1 is fused on both branches; OSM_FUSED_PCGS=0 keeps such chains on `_generic_loop`; third-party objects route as
    before."""
    unet, gd, M, CM = pkg
    model = make_model(unet)
    shape = (1, 4, 16, 16)
    pat_o, pat_p = pattern("w62", 3), pattern("w50", 2)
    co, cp = osmosis_cond(M, CM, "revised", pat_o), ps_cond(M, CM)
    s_o, s_p = make_sampler(gd), make_sampler(gd, "ddim")
    assert s_o._fast_path_ok(model, co.conditioning, "osmosis", False, pat_o, shape) is co
    assert s_p._fast_path_ok(model, cp.conditioning, "osmosis", True, pat_p, shape) is cp
    assert make_sampler(gd)._fast_path_ok(model, cp.conditioning, "osmosis", True, pat_p, shape) is cp
    monkeypatch.setenv("OSM_FUSED_PCGS", "0")
    assert s_o._fast_path_ok(model, co.conditioning, "osmosis", False, pat_o, shape) is None
    assert s_p._fast_path_ok(model, cp.conditioning, "osmosis", True, pat_p, shape) is None
    assert s_o._fast_path_ok(model, co.conditioning, "osmosis", False, pattern("w62", 1), shape) is co   # (local_M = 1: unchanged)
    monkeypatch.delenv("OSM_FUSED_PCGS")

    class ThirdPartyPS(type(cp)):
        pass
    tp = ThirdPartyPS(cp.operator, cp.noiser, scale="0.6,0.5,0.4,0.0")
    assert s_p._fast_path_ok(model, tp.conditioning, "osmosis", True, pat_p, shape) is None
    assert s_o._fast_path_ok(model, lambda **kw: None, "osmosis", False, pat_o, shape) is None


def test_opcheck_with_sub(pkg):
    from osmosis_diffusion_code_amd import torch_ops  # noqa: F401  (registers osmosis::)
    g = torch.Generator(device=DEV).manual_seed(8)
    mean, lv, gx0, dxu = (torch.randn(2, 4, 16, 16, generator=g, device=DEV) for _ in range(4))
    coef = torch.tensor([0.9, 0.1, 0.5, 0.5, 0.0, 0.0, 1.0, 7.0], device=DEV)
    scale4 = torch.tensor([7.0, 7.0, 7.0, 0.9], device=DEV)
    step = torch.tensor([120], device=DEV, dtype=torch.int32)
    a = torch.ops.osmosis.guide_update_rng(mean, lv, gx0, dxu, coef, scale4, 0.005, 77, step, 0, 0, 1)
    b = torch.ops.osmosis.guide_update_rng(mean, lv, gx0, dxu, coef, scale4, 0.005, 77, step, 0, 0, 1, 0)
    c = torch.ops.osmosis.guide_update_rng(mean, lv, gx0, dxu, coef, scale4, 0.005, 77, step, 0, 0, 1, 2)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    assert torch.equal(a[1], c[1]) and not torch.equal(a[2], c[2])
    torch.library.opcheck(torch.ops.osmosis.guide_update_rng.default, (mean, lv, gx0, dxu, coef, scale4, 0.005, 77, step, 0, 0, 1, 2))
