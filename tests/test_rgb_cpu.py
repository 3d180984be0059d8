"""The 3-channel (RGB) model family, CPU side: the oracle on the fixture's tiny 3 -> 6 / 3 -> 3 networks vs the REAL reference
(tests/golden/loop_rgb.npz, tools/gen_rgb_golden.py), the routing table of `_fast_path_ok`, the record=True error, and the
coefficient tables (which do not depend on the channel count)."""
import dataclasses
import os

import numpy as np
import pytest
import torch

from oracle import unet_ref as U

GOLD = os.path.join(os.path.dirname(__file__), "golden")
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
NETS = {"c36": dict(TINY_KW, pretrain_model="imagenet", learn_sigma=True),
        "c33": dict(TINY_KW, pretrain_model="imagenet", learn_sigma=False)}


def gold():
    return dict(np.load(os.path.join(GOLD, "loop_rgb.npz")))


@pytest.mark.parametrize("net,cout", [("c36", 6), ("c33", 3)])
def test_oracle_rgb_unet_matches_the_reference(net, cout):
    """oracle/unet_ref.py on the tiny 3 -> 6 / 3 -> 3 networks reproduces the reference's y and dx (the bars of
    test_oracle_vs_golden.py::test_tiny_unet_forward_and_input_grad): ties the oracle to the reference for the full-size GPU test."""
    g = gold()
    cfg = U.UNetConfig.from_create_model_kwargs(**NETS[net])
    assert (cfg.in_channels, cfg.out_channels) == (3, cout)
    sd = U.seeded_state_dict(cfg, 1234)
    assert sum(v.numel() for v in sd.values()) == int(g[f"unet.{net}.n_params"])
    chk = float(sum(v.double().abs().sum() for v in sd.values()))
    assert abs(chk - float(g[f"unet.{net}.weight_abs_sum"])) < 1e-6 * chk
    x = torch.from_numpy(g[f"unet.{net}.x"]).requires_grad_(True)
    y = U.unet_forward(sd, cfg, x, torch.from_numpy(g[f"unet.{net}.t"]))
    (dx,) = torch.autograd.grad((y[:, :3] ** 2).sum(), x)
    ry, rdx = torch.from_numpy(g[f"unet.{net}.y"]), torch.from_numpy(g[f"unet.{net}.dx"])
    assert y.shape == (2, cout, 32, 32)
    assert torch.allclose(y, ry, atol=1e-5), (y - ry).abs().max()
    assert torch.allclose(dx, rdx, atol=1e-5 * float(rdx.abs().max()) + 1e-6)


def test_fixture_chains_are_contractive():
    """What makes free-running comparisons possible: the reference's own final image moves by a few 1e-6 under a 1e-6 perturbation of
    x_T on every recorded chain (so no chain needed its per-call inputs recorded)."""
    g = gold()
    chains = [str(c) for c in g["chains"]]
    assert len(chains) == 13 and {c.split(".")[0] for c in chains} == {"rg", "mo"}
    for c in chains:
        assert 0 < float(g[f"{c}.drift_1e-6"]) < 2e-5, c
        assert f"{c}.x_in" not in g
        assert np.isfinite(g[f"{c}.final_img"]).all() and g[f"{c}.final_img"].shape == (1, 3, 16, 16)
        assert len(g[f"{c}.loss"]) == (16 if c.endswith(".m2") else 10)


def _model(cin, cout):
    from osmosis_diffusion_code_amd.guided_diffusion.unet import UNetModel
    return UNetModel(image_size=256, in_channels=cin, model_channels=32, out_channels=cout, num_res_blocks=1,
                     attention_resolutions=(2, 4), channel_mult=(1, 2, 2), num_heads=4, num_head_channels=16,
                     use_scale_shift_norm=True, resblock_updown=True)


def _sampler(name="ddpm", var="learned_range", **kw):
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type=var, dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    args.update(kw)
    return gd.get_sampler(name)(**args)


PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)


def _ps(scale="0.3", noiser="gaussian", op="noise"):
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    nz = M.get_noise("gaussian", sigma=0.0) if noiser == "gaussian" else M.get_noise("poisson", rate=1.0)
    return CM.get_conditioning_method("ps", M.get_operator(op, device="cpu", batch_size=1), nz, scale=scale)


# (in, out, branch, OSM_FUSED_RGB, scale, fused?)   branch: rg = rgb_guidance=True, mo = mean-only (pretrain_model != "osmosis")
ROUTES = [
    (3, 6, "rg", "1", "0.3", True), (3, 3, "rg", "1", "0.3", True), (3, 6, "mo", "1", "0.3", True), (3, 3, "mo", "1", "0.3", True),
    (3, 6, "rg", "0", "0.3", False), (3, 3, "rg", "0", "0.3", False), (3, 6, "mo", "0", "0.3", False), (3, 3, "mo", "0", "0.3", False),
    (3, 6, "rg", "1", "0.3,0.2,0.1", True), (3, 6, "rg", "1", "0.6,0.5,0.4,0.0", False),      # 1 or C scale entries
    (4, 8, "rg", "1", "0.6,0.5,0.4,0.0", True), (4, 8, "rg", "0", "0.6,0.5,0.4,0.0", True),    # the switch is for 3-channel chains
    (4, 8, "rg", "1", "0.3,0.2,0.1", False),
    (4, 4, "rg", "1", "0.3", True),                                                            # fixed variance, no variance half
    (4, 8, "mo", "1", "0.3", False), (4, 4, "mo", "1", "0.3", False),                          # 4-channel mean-only: generic
    (5, 10, "rg", "1", "0.3", False), (5, 5, "mo", "1", "0.3", False), (3, 4, "rg", "1", "0.3", False),
    (4, 6, "rg", "1", "0.3", False), (3, 9, "rg", "1", "0.3", False),
]


@pytest.mark.parametrize("cin,cout,branch,env,scale,fused", ROUTES)
def test_fast_path_routing_table(monkeypatch, cin, cout, branch, env, scale, fused):
    monkeypatch.setenv("OSM_FUSED_RGB", env)
    m = _model(cin, cout)
    cond = _ps(scale)
    s = _sampler("ddpm", "learned_range" if cout == 2 * cin else "fixed_small")
    got = s._fast_path_ok(m, cond.conditioning, "imagenet", branch == "rg", PATTERN, (1, cin, 16, 16))
    assert (got is cond) if fused else (got is None)


def test_fast_path_routing_other_conditions(monkeypatch):
    """The rest of the table: the Osmosis branch needs the 4 -> 8 network; a third-party noiser / an unguided end / an overridden
    step rule keep a 3-channel chain on `_generic_loop`; DDIM is fused on the rgb-guidance branch."""
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    monkeypatch.delenv("OSM_FUSED_RGB", raising=False)
    m36, m48, m44 = _model(3, 6), _model(4, 8), _model(4, 4)
    shape = (1, 3, 16, 16)
    s = _sampler()
    assert _sampler("ddim")._fast_path_ok(m36, _ps().conditioning, "imagenet", True, PATTERN, shape) is not None
    assert s._fast_path_ok(m36, _ps(noiser="poisson").conditioning, "imagenet", True, PATTERN, shape) is None
    assert s._fast_path_ok(m36, _ps().conditioning, "imagenet", False, dict(PATTERN, stop_guidance=0.3), shape) is None
    assert s._fast_path_ok(m36, _ps().conditioning, "imagenet", True, dict(PATTERN, stop_guidance=0.3), shape) is None
    assert s._fast_path_ok(m36, _ps().conditioning, "imagenet", False, dict(PATTERN, local_M=2, s_start=0.5, s_end=0.0), shape) is not None

    class Mine(gd.DDPM):
        def p_mean_variance(self, model, x, t):
            return super().p_mean_variance(model, x, t)
    mine = Mine(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    assert mine._fast_path_ok(m36, _ps().conditioning, "imagenet", False, PATTERN, shape) is None
    # the Osmosis configuration: 4 -> 8 only
    op = M.get_operator("underwater_physical_revised", device="cpu", batch_size=1, optimizer="sgd", depth_type="gamma",
                        value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8", phi_inf="0.14, 0.29, 0.49")
    osm = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), loss_function="norm", loss_weight="depth",
                                     weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
                                     gradient_clip="True,0.005", **PATTERN)
    assert s._fast_path_ok(m48, osm.conditioning, "osmosis", False, PATTERN, (1, 4, 16, 16)) is osm
    assert _sampler(var="fixed_small")._fast_path_ok(m44, osm.conditioning, "osmosis", False, PATTERN, (1, 4, 16, 16)) is None


@pytest.mark.parametrize("rgb_guidance", [True, False])
def test_record_true_on_a_three_channel_chain_raises_index_error(rgb_guidance):
    """The reference's record branch reads pred_xstart[:, 3] (gaussian_diffusion.py:319): IndexError on an RGB chain.  Raised before
    anything launches (the model lives on the CPU here: reaching the network would raise something else)."""
    m = _model(3, 6)
    cond = _ps()
    with pytest.raises(IndexError, match="depth channel"):
        _sampler().p_sample_loop(model=m, x_start=torch.zeros(1, 3, 16, 16), measurement=torch.zeros(1, 3, 16, 16),
                                 measurement_cond_fn=cond.conditioning, record=True, save_root=None, pretrain_model="imagenet",
                                 rgb_guidance=rgb_guidance, sample_pattern=PATTERN)


def test_ps_scale_vector_per_channel_count():
    cond = _ps("0.3")
    assert cond.scale4("cpu", 3).tolist() == pytest.approx([0.3] * 3) and cond.scale4("cpu").tolist() == pytest.approx([0.3] * 4)
    assert _ps("0.3,0.2,0.1").scale4("cpu", 3).tolist() == pytest.approx([0.3, 0.2, 0.1])
    assert _ps("0.3,0.2,0.1").hip_ok(3) and not _ps("0.3,0.2,0.1").hip_ok() and _ps("0.6,0.5,0.4,0.0").hip_ok()
    with pytest.raises(ValueError):
        _ps("0.3,0.2,0.1").scale4("cpu", 4)


def test_coefficient_tables_do_not_depend_on_the_channel_count():
    """`coef_table` / `ddim_table` are what they were: rows of the schedule (posterior coefficients, variance bounds, noise_on, t),
    pinned here against the sampler's own fp64 tables."""
    for var in ("learned_range", "fixed_small"):
        s = _sampler("ddim", var)
        tab, dtab = s.coef_table(), s.ddim_table(0.0)
        assert tab.shape == dtab.shape == (10, 8) and tab.dtype == dtab.dtype == np.float32
        assert np.array_equal(tab[:, 0], s.sqrt_recip_alphas_cumprod.astype(np.float32))
        assert np.array_equal(tab[:, 1], s.sqrt_recipm1_alphas_cumprod.astype(np.float32))
        assert np.array_equal(tab[:, 2], s.posterior_mean_coef1.astype(np.float32))
        assert np.array_equal(tab[:, 3], s.posterior_mean_coef2.astype(np.float32))
        assert tab[0, 6] == 0.0 and np.all(tab[1:, 6] == 1.0)
        assert np.array_equal(tab[:, 7], np.arange(0, 100, 10, dtype=np.float32))
        assert np.array_equal(dtab[:, 0], s.alphas_cumprod.astype(np.float32))
        assert np.array_equal(dtab[:, 1], s.alphas_cumprod_prev.astype(np.float32))
        assert dtab[0, 3] == 0.0 and np.all(dtab[1:, 3] == 1.0) and np.all(dtab[:, 2] == 0.0)
        assert np.array_equal(dtab[:, 7], tab[:, 7])


def test_header_declares_the_channel_generic_entry_points():
    from osmosis_diffusion_code_amd import _lib, torch_ops
    new = {"osm_posterior_c", "osm_posterior_dynthr_c", "osm_posterior_bwd_c", "osm_guide_update_c", "osm_guide_update_rng_c",
           "osm_ddim_update_c", "osm_ps_loss_grad_c"}
    assert new <= set(_lib.exports("osmosis_hip.h"))
    with open(os.path.join(os.path.dirname(GOLD), "..", "include", "osmosis_hip.h")) as f:
        hdr = f.read()
    for n in new:
        assert f"int {n}(" in hdr, n
    assert set(torch_ops.OPS_C) <= set(torch_ops.OPS)
    for name in torch_ops.OPS_C:
        assert getattr(torch.ops.osmosis, name).default is not None
