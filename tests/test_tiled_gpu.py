"""Tiled sampling on the HIP path.

Kernel level (no network): osm_tile_gather / osm_tile_blend against float64 restatements of the same fp32 inputs -- the plain
crop bit for bit, the weighted gather, the blend, the partition of unity, the adjoint identity, the single tile, determinism --
and torch.library.opcheck on the two operators.
Chain level (the tiny 4 -> 8 network in exact fp32, a 10-index respaced chain, injected noise, `_generic_loop` patched to raise;
the helpers and constants of tests/test_mask_gpu.py): a 24 x 36 canvas as six 16 x 16 tiles at stride (8, 12) against the oracle's
own loop around a tiled wrapper of the oracle's network, one tile against the untiled fused chain, chunked tile batches against
one pass, the library's noise stream, the options the tiled loop refuses, and `restore_image(tiling=)` end to end."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import diffusion_ref as D
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
# (C, Hc, Wc, th, tw, sy, sx): ragged 2 x 2 overlap; odd sizes, every vector tail, up to nine covering tiles; a single tile
GEOMETRIES = [(4, 40, 52, 32, 32, 24, 24), (8, 37, 45, 16, 20, 7, 9), (4, 16, 24, 16, 24, 16, 24)]
WINDOWS = ["uniform", "hann"]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


# ============================================================================================================ kernel level
def _case(gd, geo, window, seed=0):
    C, Hc, Wc, th, tw, sy, sx = geo
    origins, wy, wx, inv = gd.tile_grid(Hc, Wc, (th, tw), (sy, sx), window)
    g = torch.Generator().manual_seed(1000 * seed + Hc)
    canvas = torch.randn(C, Hc, Wc, generator=g)
    tiles = torch.randn(origins.shape[0], C, th, tw, generator=g)
    return canvas, tiles, origins, wy, wx, inv


def gather64(canvas, origins, th, tw, wy=None, wx=None, inv=None):
    """float64 restatement: the crop, times wy[y] wx[x] inv_norm[oy + y, ox + x] of the same fp32 weights."""
    out = []
    for oy, ox in origins.tolist():
        t = canvas[:, oy:oy + th, ox:ox + tw].double()
        if wy is not None:
            t = t * (wy.double()[:, None] * wx.double()[None, :] * inv.double()[oy:oy + th, ox:ox + tw])
        out.append(t)
    return torch.stack(out, 0)


def blend64(tiles, origins, Hc, Wc, wy=None, wx=None, inv=None):
    """float64 restatement and the per-pixel bound (k + 3) 2^-24 inv_norm sum_t |w_t v_t|, k = the number of covering tiles."""
    n, C, th, tw = tiles.shape
    w = torch.ones(th, tw, dtype=torch.float64) if wy is None else wy.double()[:, None] * wx.double()[None, :]
    total, mag, cover = torch.zeros(C, Hc, Wc, dtype=torch.float64), torch.zeros(C, Hc, Wc, dtype=torch.float64), torch.zeros(Hc, Wc)
    for t, (oy, ox) in enumerate(origins.tolist()):
        total[:, oy:oy + th, ox:ox + tw] += tiles[t].double() * w
        mag[:, oy:oy + th, ox:ox + tw] += (tiles[t].double() * w).abs()
        cover[oy:oy + th, ox:ox + tw] += 1
    scale = torch.ones(Hc, Wc, dtype=torch.float64) if inv is None else inv.double()
    return total * scale, (cover.double() + 3) * EPS * scale * mag, cover


def hip_gather(canvas, origins, th, tw, *weights):
    from osmosis_diffusion_code_amd import ops
    tiles = torch.full((origins.shape[0], canvas.shape[0], th, tw), float("nan"), device=DEV)
    ops.tile_gather(canvas.to(DEV), tiles, origins.to(DEV), *(w.to(DEV) for w in weights))
    return tiles.cpu()


def hip_blend(tiles, origins, Hc, Wc, *weights):
    from osmosis_diffusion_code_amd import ops
    canvas = torch.full((tiles.shape[1], Hc, Wc), float("nan"), device=DEV)
    ops.tile_blend(tiles.to(DEV), canvas, origins.to(DEV), *(w.to(DEV) for w in weights))
    return canvas.cpu()


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("geo", GEOMETRIES, ids=lambda g: "x".join(map(str, g)))
def test_tile_gather_and_blend_against_float64(pkg, geo, window):
    gd = pkg[1]
    C, Hc, Wc, th, tw, sy, sx = geo
    canvas, tiles, origins, wy, wx, inv = _case(gd, geo, window)
    n = origins.shape[0]
    # unweighted gather: the slices, bit for bit
    got = hip_gather(canvas, origins, th, tw)
    assert torch.equal(got, gather64(canvas, origins, th, tw).float())
    assert torch.equal(got, hip_gather(canvas, origins, th, tw))
    # weighted gather: relative error <= 4 x 2^-24 (three roundings: wy wx, its product with inv_norm, the product with the pixel)
    got_w = hip_gather(canvas, origins, th, tw, wy, wx, inv)
    want_w = gather64(canvas, origins, th, tw, wy, wx, inv)
    rel = float(((got_w.double() - want_w).abs() / want_w.abs().clamp_min(1e-300)).max())
    # blend, weighted and plain
    got_b = hip_blend(tiles, origins, Hc, Wc, wy, wx, inv)
    want_b, bound_b, cover = blend64(tiles, origins, Hc, Wc, wy, wx, inv)
    got_s = hip_blend(tiles, origins, Hc, Wc)
    want_s, bound_s, _ = blend64(tiles, origins, Hc, Wc)
    e_b = float(((got_b.double() - want_b).abs() / bound_b).max())
    e_s = float(((got_s.double() - want_s).abs() / bound_s).max())
    # partition of unity: the weighted blend of the plain crops is the canvas, within the blend's bound
    back = hip_blend(got, origins, Hc, Wc, wy, wx, inv)
    _, bound_u, _ = blend64(got, origins, Hc, Wc, wy, wx, inv)
    e_u = float(((back.double() - canvas.double()).abs() / bound_u).max())
    # adjoint identity <blend(T), G> = <T, gather_w(G)> in float64; bound: the two sides' bounds against their terms
    lhs = float((got_b.double() * canvas.double()).sum())
    rhs = float((tiles.double() * got_w.double()).sum())
    adj_bound = float((bound_b * canvas.double().abs()).sum()) + 4 * EPS * float((tiles.double() * want_w).abs().sum())
    lhs_s = float((got_s.double() * canvas.double()).sum())
    rhs_s = float((tiles.double() * got.double()).sum())
    adj_bound_s = float((bound_s * canvas.double().abs()).sum())
    print(f"TILEKERNEL {geo} {window}: n {n}, cover max {int(cover.max())}; weighted gather rel {rel / EPS:.2f} x 2^-24 (bar 4); blend "
          f"{e_b:.3f} / plain {e_s:.3f} / unity {e_u:.3f} of the bound; adjoint |lhs - rhs| {abs(lhs - rhs):.2e} (bar {adj_bound:.2e}), "
          f"plain {abs(lhs_s - rhs_s):.2e} (bar {adj_bound_s:.2e})")
    assert int(cover.min()) >= 1 and int(cover.max()) == {40: 4, 37: 9, 16: 1}[Hc]
    assert rel <= 4 * EPS
    assert e_b <= 1.0 and e_s <= 1.0 and e_u <= 1.0
    assert abs(lhs - rhs) <= adj_bound and abs(lhs_s - rhs_s) <= adj_bound_s
    # determinism: two runs, bit for bit
    assert torch.equal(got_w, hip_gather(canvas, origins, th, tw, wy, wx, inv))
    assert torch.equal(got_b, hip_blend(tiles, origins, Hc, Wc, wy, wx, inv)) and torch.equal(got_s, hip_blend(tiles, origins, Hc, Wc))
    if n == 1 and window == "uniform":           # a single tile with the uniform window: both directions are copies
        assert torch.equal(got_w[0], canvas) and torch.equal(got_b, tiles[0]) and torch.equal(got_s, tiles[0])


def test_gather_writes_zeros_for_an_origin_off_the_canvas_and_blend_for_an_uncovered_pixel(pkg):
    from osmosis_diffusion_code_amd import ops
    C, Hc, Wc, th, tw = 4, 24, 36, 16, 16
    big = torch.randn(C + 2, Hc, Wc, generator=torch.Generator().manual_seed(3)).to(DEV)
    canvas = big[1:C + 1]                         # (rows around the canvas exist: nothing here can leave the allocation)
    origins = torch.tensor([[8, 20], [9, 20], [8, 21], [-1, 0], [0, 0]], dtype=torch.int32, device=DEV)
    tiles = torch.full((5, C, th, tw), float("nan"), device=DEV)
    ops.tile_gather(canvas, tiles, origins)
    assert torch.equal(tiles[0], canvas[:, 8:24, 20:36]) and torch.equal(tiles[4], canvas[:, 0:16, 0:16])
    for t in (1, 2, 3):
        assert float(tiles[t].abs().max()) == 0.0, t
    out = torch.full((C, Hc, Wc), float("nan"), device=DEV)
    ops.tile_blend(tiles[4:5].contiguous(), out, origins[4:5].contiguous())
    assert torch.equal(out[:, :16, :16], tiles[4]) and float(out[:, 16:].abs().max()) == 0.0 and float(out[:, :, 16:].abs().max()) == 0.0


def test_opcheck_and_autograd_of_the_tile_operators(pkg):
    gd = pkg[1]
    from osmosis_diffusion_code_amd import torch_ops
    assert {"tile_gather", "tile_blend"} <= set(torch_ops.OPS)
    geo = GEOMETRIES[1]
    C, Hc, Wc, th, tw, sy, sx = geo
    canvas, tiles, origins, wy, wx, inv = (t.to(DEV) for t in _case(gd, geo, "hann", seed=2))
    for weights in ((), (wy, wx, inv)):
        c, t = canvas.clone().requires_grad_(True), tiles.clone().requires_grad_(True)
        torch.library.opcheck(torch.ops.osmosis.tile_gather.default, (c, origins, th, tw, *weights))
        torch.library.opcheck(torch.ops.osmosis.tile_blend.default, (t, origins, Hc, Wc, *weights))
        # each is the other's backward, with the same weights
        (gt,) = torch.autograd.grad((torch.ops.osmosis.tile_blend(t, origins, Hc, Wc, *weights) * canvas).sum(), t)
        assert torch.equal(gt, torch.ops.osmosis.tile_gather(canvas, origins, th, tw, *weights))
        (gc,) = torch.autograd.grad((torch.ops.osmosis.tile_gather(c, origins, th, tw, *weights) * tiles).sum(), c)
        assert torch.equal(gc, torch.ops.osmosis.tile_blend(tiles, origins, Hc, Wc, *weights))


# ============================================================================================================ chain level
# (helpers and constants of tests/test_mask_gpu.py)
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")
COND = dict(loss_function="norm", loss_weight="depth", weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
            gradient_clip="True,0.005")
AUX = {"avrg_loss": 0.5, "val_loss": 20}
OPERATORS = {
    "underwater_physical_revised": dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_a_eta="1e-5",
                                        phi_a_learn_flag=True, phi_b="0.95, 0.8, 0.8", phi_b_eta="1e-5", phi_b_learn_flag=True,
                                        phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True),
    "haze_physical": dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_ab_eta="1e-5", phi_ab_learn_flag=True,
                          phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True),
}
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)
T = 10
CANVAS = (24, 36)
TILING = dict(tile=(16, 16), stride=(8, 12))          # 2 x 3 = 6 tiles, x origins [0, 12, 20]: a ragged last overlap


class MaskedGuidance(D.OsmosisGuidance):
    """The oracle's guidance with the mask in the residual: diff = (y - (2 I - 1)) w M; the losses keep their normalisation."""
    mask = None

    def loss(self, x0, y):
        I = self.op.forward(x0)
        diff = (y - (2 * I - 1)) * self._weight(x0) * self.mask
        if self.loss_function == "norm":
            return torch.norm(diff.detach(), p=2, dim=[1, 2, 3]).numpy(), torch.linalg.norm(diff)
        mse = (diff ** 2).mean(dim=(1, 2, 3))
        return mse.detach().numpy(), mse.sum()


def make_model(unet, kw=TINY_KW):
    cfg = U.UNetConfig.from_create_model_kwargs(**kw)
    m = unet.create_model(**kw)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    m.conv_mode = "f32"
    return m


@pytest.fixture(scope="module")
def model48(pkg):
    return make_model(pkg[0])


def make_sampler(gd, name="ddpm", **kw):
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    args.update(kw)
    return gd.get_sampler(name)(**args)


def osmosis_cond(pkg, opname, pat, B=1):
    _, _, M, CM = pkg
    operator = M.get_operator(opname, device=DEV, batch_size=B, **OPERATORS[opname])
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **pat, aux_loss=AUX)


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _free_running_bar(drift):
    """As in test_mask_gpu.py / test_pcgs_gpu.py: tight for well-conditioned chains, the north-star 1e-3 for mildly amplifying
    ones, None (teacher-forced) for chains the oracle itself cannot reproduce to 1e-3."""
    if drift <= 1e-4:
        return max(2e-5, 10.0 * drift)
    return 1e-3 if drift <= 1e-3 else None


def chain_inputs(seed, hw=CANVAS, n=T):
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(1, 4, H, W, generator=g)
    y = torch.rand(1, 3, H, W, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, 1, 4, H, W, generator=g)
    mask = torch.rand(1, 3, H, W, generator=g) * (torch.rand(1, 1, H, W, generator=g) > 0.3).float()
    mask[:, :, 4:9, 6:15] = 0.0
    return x_T, y, noise, mask


def _same_bits(a, b, what):
    e = {"img": float((a[0] - b[0]).abs().max()), "x0": float((a[3] - b[3]).abs().max()),
         "loss": float(np.abs(np.asarray(a[2]) - np.asarray(b[2])).max()),
         "phi": max(float((a[1][n] - b[1][n]).abs().max()) for n in a[1])}
    print(f"TILEBITS {what}: max-abs differences {e}")
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and np.array_equal(a[2], b[2]), (what, e)
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), (what, n, e)


def _run(pkg, monkeypatch, model, x_T, y, injected, tiling, opname="underwater_physical_revised", mask=None, sampler_kw=None, **kw):
    gd = pkg[1]
    sampler = make_sampler(gd, **(sampler_kw or {}))
    _no_generic(monkeypatch, sampler)
    cond = osmosis_cond(pkg, opname, PATTERN)
    if injected is not None:
        nd = injected.to(DEV)
        kw["noise_fn"] = lambda k, shape: nd[k]
    out = sampler.p_sample_loop(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                                measurement_mask=mask, tiling=tiling, **kw)
    monkeypatch.undo()
    return out


# ------------------------------------------------------------------------------------------------------------ 1: one tile = the fused chain
@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip_denoised"])
def test_one_tile_covering_the_canvas_is_the_untiled_fused_chain_bit_for_bit(pkg, monkeypatch, model48, clip):
    x_T, y, noise, mask = chain_inputs(81, (16, 24))
    kw = dict(sampler_kw=dict(clip_denoised=clip), mask=mask if clip else None)
    plain = _run(pkg, monkeypatch, model48, x_T, y, noise, None, **kw)
    tiled = _run(pkg, monkeypatch, model48, x_T, y, noise, dict(tile=(16, 24), stride=(16, 24), window="uniform"), **kw)
    assert bool(torch.isfinite(plain[0]).all())
    _same_bits(tiled, plain, f"one 16 x 24 tile, uniform window, clip_denoised {clip}: tiled vs untiled fused chain")


# ------------------------------------------------------------------------------------------------------------ 2: against the oracle
def tiled_oracle_model(sd, cfg, origins, wy, wx, inv, th, tw):
    """The CPU restatement of the tiled network: crop, the oracle's network per tile, blend with the same fp32 wy, wx and
    inv_norm, in torch under autograd (so the oracle's guidance differentiates through the blend)."""
    w = wy[:, None] * wx[None, :]

    def model(x, t):
        Hc, Wc = x.shape[-2:]
        total = 0.0
        for oy, ox in origins.tolist():
            o = U.unet_forward(sd, cfg, x[:, :, oy:oy + th, ox:ox + tw], t)
            total = total + F.pad(o * w, (ox, Wc - ox - tw, oy, Hc - oy - th))
        return total * inv
    return model


def _oracle_chain(gd, opname, window, cfg, sd, tb, x_T, y, noise, mask):
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    rop = D.PhysOperator(opname, batch_size=1, depth_type="gamma", value="1.4,1.4,1", **okw)
    if mask is None:
        rg = D.OsmosisGuidance(rop, n_iter=20, scale=COND["scale"], gradient_clip=COND["gradient_clip"], aux=AUX)
    else:
        rg = MaskedGuidance(rop, n_iter=20, scale=COND["scale"], gradient_clip=COND["gradient_clip"], aux=AUX)
        rg.mask = mask
    th, tw = TILING["tile"]
    origins, wy, wx, inv = gd.tile_grid(*x_T.shape[-2:], TILING["tile"], TILING["stride"], window)
    trace = []
    D.p_sample_loop(tiled_oracle_model(sd, cfg, origins, wy, wx, inv, th, tw), tb, x_T, y, rg, PATTERN, [noise[k] for k in range(T)], trace)
    return trace


@pytest.mark.parametrize("opname,window,masked", [("underwater_physical_revised", "hann", False),
                                                  ("underwater_physical_revised", "uniform", False),
                                                  ("haze_physical", "hann", False), ("haze_physical", "uniform", False),
                                                  ("underwater_physical_revised", "hann", True)])
def test_tiled_fused_chain_vs_the_tiled_oracle(pkg, monkeypatch, model48, opname, window, masked):
    """The tiled fused chain (24 x 36 canvas, six 16 x 16 tiles) against the oracle's own loop around a tiled wrapper of the
    oracle's network, same weights, x_T, measurement and noise.  Protocol and bars of
    test_mask_gpu.py::test_fused_masked_osmosis_chain_vs_the_masked_oracle: the bar comes from the oracle's own drift under a 1e-6
    perturbation of x_T (`_free_running_bar`); where the oracle cannot reproduce itself to 1e-3, teacher-forced per index from the
    oracle's x_in and phi at 1e-3 / 2e-5 / 2e-6."""
    _, gd, _, _ = pkg
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    x_T, y, noise, mask = chain_inputs(91)
    mask = mask if masked else None
    tiling = dict(TILING, window=window)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ref = _oracle_chain(gd, opname, window, cfg, sd, tb, x_T, y, noise, mask)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert = _oracle_chain(gd, opname, window, cfg, sd, tb, x_T + bump, y, noise, mask)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(tb.timestep_map)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)
    tag = f"{opname} {window}{' masked' if masked else ''}"

    def hip(x_start, index_range=None, phi0=None, k0=0):
        cond = osmosis_cond(pkg, opname, PATTERN)
        if phi0 is not None:
            for name, (off, m) in cond.operator._slots().items():
                cond.operator.phi[0, off:off + m] = phi0[name].reshape(-1)[:m].to(DEV)
        trace = []
        kw = {} if index_range is None else {"index_range": index_range}
        sampler.p_sample_loop(model=model48, x_start=x_start.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k0 + k], trace=trace, measurement_mask=mask, tiling=tiling, **kw)
        return trace, cond

    def errs(a, b, slots):
        e_phi = max(float((a["phi"][0, off:off + m].cpu() - b["phi"][n].reshape(-1)[:m]).abs().max()) for n, (off, m) in slots.items())
        return (float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max()),
                abs(float(a["loss"][0]) - float(np.asarray(b["loss"]).reshape(-1)[0])) / float(np.asarray(b["loss"]).reshape(-1)[0]), e_phi)
    if bar is not None:
        trace, cond = hip(x_T)
        assert len(trace) == T and tuple(trace[0]["model_out"].shape) == (1, 8, *CANVAS)
        slots = cond.operator._slots()
        e_img, e_x0, e_loss, e_phi = (max(v) for v in zip(*(errs(a, b, slots) for a, b in zip(trace, ref))))
        f_img, f_x0, f_loss, f_phi = errs(trace[-1], ref[-1], slots)
        msg = (f"TILECHAIN {tag}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
               f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}; worst over the chain: x_out {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
               f"phi {e_phi:.2e}")
        print(msg)
        assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
        return
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(T):
        idx = T - 1 - k
        trace, cond = hip(ref[k]["x_in"], (idx, idx), None if k == 0 else ref[k - 1]["phi"], k0=k)
        worst = [max(w, e) for w, e in zip(worst, errs(trace[0], ref[k], cond.operator._slots()))]
    msg = (f"TILECHAIN {tag}: oracle drift_1e-6 {drift:.2e} > 1e-3, teacher-forced per index: x_out {worst[0]:.2e} x0 {worst[1]:.2e} "
           f"loss(rel) {worst[2]:.2e} phi {worst[3]:.2e}")
    print(msg)
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 2e-5 and worst[3] < 2e-6, msg


# ------------------------------------------------------------------------------------------------------------ 3: chunked tile batches
@pytest.mark.parametrize("hw,tiling,cap,sizes", [(CANVAS, dict(TILING, window="hann"), 4, [3, 3]),
                                                 ((16, 48), dict(tile=16, stride=8, window="hann"), 3, [2, 2, 1])])
def test_tiles_walked_in_chunks_equal_one_pass(pkg, monkeypatch, model48, hw, tiling, cap, sizes):
    gd = pkg[1]
    x_T, y, noise, mask = chain_inputs(92, hw)
    n = gd.tile_grid(*hw, tiling["tile"], tiling["stride"], tiling["window"])[0].shape[0]
    whole = _run(pkg, monkeypatch, model48, x_T, y, noise, tiling, mask=mask)
    assert bool(torch.isfinite(whole[0]).all())
    os.environ["OSM_MAX_BATCH"] = str(cap)
    try:
        assert gd.GaussianDiffusion.chunk_sizes(n, model48.images_in_flight(n, 16, 16)) == sizes
        chunked = _run(pkg, monkeypatch, model48, x_T, y, noise, tiling, mask=mask)
    finally:
        os.environ.pop("OSM_MAX_BATCH", None)
    _same_bits(whole, chunked, f"{n} tiles in one pass vs chunks {sizes}")


# ------------------------------------------------------------------------------------------------------------ 4: the library's noise
def test_library_noise_belongs_to_the_canvas_and_repeats(pkg, monkeypatch, model48):
    x_T, y, _, _ = chain_inputs(93)
    tiling = dict(TILING, window="hann")
    runs, traces = [], []
    for _ in range(2):
        trace = []
        runs.append(_run(pkg, monkeypatch, model48, x_T, y, None, tiling, noise="library", noise_seed=11, trace=trace))
        traces.append(trace)
    _same_bits(runs[0], runs[1], "noise='library', noise_seed=11, twice")
    assert len(traces[0]) == T and all(tuple(r["noise"].shape) == (1, 4, *CANVAS) for r in traces[0])
    assert all(torch.equal(a["noise"], b["noise"]) for a, b in zip(*traces)) and float(traces[0][0]["noise"].std()) > 0.5
    other = _run(pkg, monkeypatch, model48, x_T, y, None, tiling, noise="library", noise_seed=12)
    assert not torch.equal(other[0], runs[0][0])
    aten = _run(pkg, monkeypatch, model48, x_T, y, None, tiling, noise="aten")
    assert bool(torch.isfinite(aten[0]).all()) and tuple(aten[0].shape) == (1, 4, *CANVAS)


# ------------------------------------------------------------------------------------------------------------ 5: what is refused
def test_unsupported_options_raise_and_never_reach_the_generic_loop(pkg, monkeypatch, model48):
    unet, gd, M, CM = pkg
    x_T, y, noise, _ = chain_inputs(94)
    tiling = dict(TILING, window="hann")
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    monkeypatch.setattr(gd.GaussianDiffusion, "_fused_loop", lambda *a, **k: 1 / 0)

    def loop(sampler=None, cond=None, model=model48, x=x_T, yy=y, pat=PATTERN, **kw):
        sampler = sampler or make_sampler(gd)
        cond = cond or osmosis_cond(pkg, "underwater_physical_revised", pat)
        call = dict(model=model, x_start=x.to(DEV), measurement=yy.to(DEV), measurement_cond_fn=cond.conditioning, record=False,
                    save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat, tiling=tiling)
        call.update(kw)
        return sampler.p_sample_loop(**call)
    ps = CM.PosteriorSampling(M.get_operator("noise", device=DEV, batch_size=1), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="rgb_guidance"):
        loop(cond=ps, rgb_guidance=True)
    with pytest.raises(NotImplementedError, match="mean-only"):
        loop(cond=ps, pretrain_model="imagenet")
    with pytest.raises(NotImplementedError, match="ddim"):
        loop(sampler=make_sampler(gd, "ddim"))
    with pytest.raises(NotImplementedError, match="dynamic_threshold"):
        loop(sampler=make_sampler(gd, dynamic_threshold=True))
    with pytest.raises(NotImplementedError, match="one canvas"):
        loop(cond=osmosis_cond(pkg, "underwater_physical_revised", PATTERN, B=2), x=x_T.repeat(2, 1, 1, 1), yy=y.repeat(2, 1, 1, 1))
    with pytest.raises(NotImplementedError, match="4 -> 8"):
        loop(model=make_model(unet, RGB_KW), x=x_T[:, :3])
    declined = osmosis_cond(pkg, "underwater_physical_revised", PATTERN)
    declined.hip_ok = lambda: False               # (a third-party operator / auxiliary loss: no fused step)
    with pytest.raises(NotImplementedError, match="no fused step"):
        loop(cond=declined)
    pat2 = dict(PATTERN, local_M=2, s_start=0.6, s_end=0.2)
    monkeypatch.setenv("OSM_FUSED_PCGS", "0")
    with pytest.raises(NotImplementedError, match="no fused step"):
        loop(pat=pat2)
    monkeypatch.delenv("OSM_FUSED_PCGS")
    with pytest.raises(ValueError, match="does not fit"):
        loop(tiling=dict(tile=32, stride=8))
    monkeypatch.undo()
    # the same sub-step pattern runs tiled once the fused path is allowed: PCGS sub-steps fall out of the structure
    n = sum(a for _, _, a in gd.pcgs_schedule(pat2, T))
    assert n > T
    x2, y2, noise2, _ = chain_inputs(95, n=n)
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    nd, trace = noise2.to(DEV), []
    cond = osmosis_cond(pkg, "underwater_physical_revised", pat2)
    out = sampler.p_sample_loop(model=model48, x_start=x2.to(DEV), measurement=y2.to(DEV), measurement_cond_fn=cond.conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat2,
                                tiling=tiling, noise_fn=lambda k, shape: nd[k], trace=trace)
    assert len(trace) == n and bool(torch.isfinite(out[0]).all()) and max(r["sub"] for r in trace) == 1


# ------------------------------------------------------------------------------------------------------------ 6: restore_image
def test_restore_image_tiled_end_to_end_with_the_full_resolution_path(pkg, monkeypatch, model48, tmp_path):
    """A synthetic 50 x 75 photo -> `fit_transform` (a 24 x 36 grid) and `transform_mask` -> `restore_image(tiling=)` / the config
    key -> `reconstruct_full_resolution` with the canvas's Geometry -> `save_outputs`."""
    from PIL import Image

    from osmosis_diffusion_code_amd import sampling
    from osmosis_diffusion_code_amd.osmosis_utils import data as DT
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    monkeypatch.setattr(gd.GaussianDiffusion, "_fused_loop", lambda *a, **k: 1 / 0)
    rng = np.random.default_rng(96)
    pic = Image.fromarray((50 + 150 * rng.random((50, 75, 3))).astype(np.uint8), mode="RGB")
    img, geo = DT.fit_transform(size=24, multiple=4)(pic)
    assert (geo.h, geo.w) == CANVAS and tuple(img.shape) == (3, *CANVAS)
    valid = np.ones((50, 75), dtype=np.float32)
    valid[10:20, 30:50] = 0.0
    mask = DT.transform_mask(valid, size=24, geometry=geo)
    assert tuple(mask.shape) == (1, 1, *CANVAS)
    ref = img.unsqueeze(0).to(DEV)
    cfg = {"measurement": {"operator": dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised"),
                           "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    tiling = dict(TILING, window="hann")
    by_arg = sampling.restore_image(model48, ref, cfg, noise_seed=7, mask=mask, tiling=tiling)[-1]
    by_cfg = sampling.restore_image(model48, ref, dict(cfg, tiling={"tile": [16, 16], "stride": [8, 12], "window": "hann"}), noise_seed=7,
                                    mask=mask)[-1]
    via_images = sampling.restore_images(model48, [ref], cfg, noise_seed=7, masks=[mask], tiling=tiling, originals=[DT.to_tensor(pic)],
                                         geometries=[geo])[0]
    x0 = by_arg["pred_xstart"]
    assert tuple(x0.shape) == (1, 4, *CANVAS) and bool(torch.isfinite(x0).all()) and bool(torch.isfinite(by_arg["sample"]).all())
    assert torch.equal(x0, by_cfg["pred_xstart"]) and torch.equal(by_arg["sample"], by_cfg["sample"])
    assert torch.equal(x0, via_images["pred_xstart"])
    for r in (by_arg, by_cfg, via_images):
        t = r["tiling"]
        assert t["tile"] == (16, 16) and t["stride"] == (8, 12) and t["window"] == "hann"
        assert t["origins"].tolist() == [[0, 0], [0, 12], [0, 20], [8, 0], [8, 12], [8, 20]]
    assert tuple(by_arg["mask"].shape) == (1, 3, *CANVAS)
    with pytest.raises(ValueError, match="unknown key"):
        sampling.restore_image(model48, ref, dict(cfg, tiling={"tile": 16, "overlap": 4}), noise_seed=7)
    full = sampling.reconstruct_full_resolution(by_arg, DT.to_tensor(pic), geo, cfg["measurement"]["operator"])
    assert tuple(full["rgb_recon_full"].shape) == (3, geo.Hc, geo.Wc) and bool(torch.isfinite(full["rgb_recon_full"]).all())
    assert torch.equal(full["rgb_recon_full"], via_images["full_res"]["rgb_recon_full"])
    paths = sampling.save_outputs(by_arg, ref, str(tmp_path), "photo", full_res=full)
    assert {"rgb", "depth_color", "mask", "recon_full", "depth_full"} <= set(paths) and all(os.path.getsize(p) > 0 for p in paths.values())
    monkeypatch.undo()
    plain = sampling.restore_image(model48, img[:, :16, :24].unsqueeze(0).contiguous().to(DEV), cfg, noise_seed=7)[-1]      # (untiled: `_fused_loop`)
    assert "tiling" not in plain
