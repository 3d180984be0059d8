"""Tiled sampling, host side: the tile grid (origins, windows, blend normalisation), the errors a bad tiling raises before
anything launches, and the C ABI entries osm_tile_gather / osm_tile_blend (declared, exported, bound, validating).  No GPU."""
import os
import re

import numpy as np
import pytest
import torch

from osmosis_diffusion_code_amd import _lib, sampling
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L,t,s,want", [(52, 32, 24, [0, 20]), (40, 32, 24, [0, 8]), (48, 16, 8, [0, 8, 16, 24, 32]), (16, 16, 8, [0])])
def test_tile_origins_per_axis(L, t, s, want):
    assert gd.tile_origins(L, t, s) == want
    assert gd.tile_origins(L, t, s) == list(range(0, L - t, s)) + [L - t]


def test_tile_grid_enumerates_row_major_in_y_x_order():
    origins, wy, wx, inv = sampling.tile_grid(40, 52, 32, 24, "uniform")
    assert origins.dtype == torch.int32 and origins.tolist() == [[0, 0], [0, 20], [8, 0], [8, 20]]
    assert wy.dtype == wx.dtype == inv.dtype == torch.float32 and wy.shape == (32,) and wx.shape == (32,) and inv.shape == (40, 52)
    assert sampling.tile_grid is gd.tile_grid
    origins, wy, wx, inv = gd.tile_grid(24, 36, (16, 16), (8, 12), "hann")
    assert origins.tolist() == [[0, 0], [0, 12], [0, 20], [8, 0], [8, 12], [8, 20]]
    origins, wy, wx, inv = gd.tile_grid(16, 24, (16, 24), (16, 24), "uniform")
    assert origins.tolist() == [[0, 0]] and bool((inv == 1).all()) and bool((wy == 1).all()) and bool((wx == 1).all())


@pytest.mark.parametrize("window", ["uniform", "hann"])
@pytest.mark.parametrize("Hc,Wc,tile,stride", [(40, 52, (32, 32), (24, 24)), (37, 45, (16, 20), (7, 9)), (16, 24, (16, 24), (16, 24)),
                                               (512, 768, (256, 256), (128, 128))])
def test_blend_weights_sum_to_one(Hc, Wc, tile, stride, window):
    """inv_norm * sum over the covering tiles of the fp32 windows' float64 product = 1 within the one fp32 rounding of inv_norm;
    every pixel is covered."""
    origins, wy, wx, inv = gd.tile_grid(Hc, Wc, tile, stride, window)
    total = np.zeros((Hc, Wc))
    cover = np.zeros((Hc, Wc), dtype=int)
    w = np.outer(wy.double().numpy(), wx.double().numpy())
    for oy, ox in origins.tolist():
        total[oy:oy + tile[0], ox:ox + tile[1]] += w
        cover[oy:oy + tile[0], ox:ox + tile[1]] += 1
    assert cover.min() >= 1 and bool(torch.isfinite(inv).all()) and float(inv.min()) > 0
    assert np.abs(inv.double().numpy() * total - 1.0).max() <= 2.0 ** -24 + 1e-12
    if window == "uniform":
        assert np.array_equal(inv.numpy(), (1.0 / cover).astype(np.float32))


@pytest.mark.parametrize("t", [4, 16, 20, 32, 256])
def test_hann_window_is_strictly_positive_and_symmetric(t):
    w = gd.tile_window(t, "hann")
    assert w.dtype == np.float64 and w.min() > 0 and w.max() <= 1.0
    assert np.allclose(w, np.sin(np.pi * (np.arange(t) + 0.5) / t) ** 2, rtol=0, atol=0) and np.allclose(w, w[::-1], atol=1e-15)
    assert float(torch.from_numpy(w).float().min()) > 0          # still positive once cast for the kernels
    assert np.array_equal(gd.tile_window(t, "uniform"), np.ones(t))


def test_bad_tilings_raise_value_errors():
    with pytest.raises(ValueError, match="does not fit"):
        gd.tile_origins(15, 16, 8)
    with pytest.raises(ValueError, match="does not fit"):
        gd.tile_grid(24, 36, (32, 16), 8, "hann")
    for s in (0, 17, -1):
        with pytest.raises(ValueError, match="stride"):
            gd.tile_origins(48, 16, s)
    with pytest.raises(ValueError, match="stride"):
        gd.tile_grid(24, 36, 16, (8, 17), "uniform")
    with pytest.raises(ValueError, match="window"):
        gd.tile_grid(24, 36, 16, 8, "gauss")
    with pytest.raises(ValueError, match="window"):
        gd.parse_tiling(dict(tile=16, stride=8, window="box"))
    with pytest.raises(ValueError, match="unknown key"):
        gd.parse_tiling(dict(tile=16, strid=8))
    with pytest.raises(ValueError, match="tile"):
        gd.parse_tiling(dict(stride=8))
    with pytest.raises(ValueError, match="pair"):
        gd.parse_tiling(dict(tile=(16, 16, 16)))
    with pytest.raises(ValueError, match="integer"):
        gd.parse_tiling(dict(tile=16.5))
    with pytest.raises(ValueError, match="mapping"):
        gd.parse_tiling(16)
    assert gd.parse_tiling(dict(tile=16)) == (16, 16, 8, 8, "hann")
    assert gd.parse_tiling(dict(tile=[16, 32], stride=[8, 12], window="uniform")) == (16, 32, 8, 12, "uniform")


def _loop(tiling, x=None, y=None, model=None, sampler_kw=None, **kw):
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    name = (sampler_kw or {}).pop("name", "ddpm") if sampler_kw else "ddpm"
    args.update(sampler_kw or {})
    sampler = gd.get_sampler(name)(**args)
    x = torch.zeros(1, 4, 24, 36) if x is None else x
    y = torch.zeros(1, 3, *x.shape[2:]) if y is None else y
    call = dict(model=model, x_start=x, measurement=y, measurement_cond_fn=None, record=False, save_root=None,
                pretrain_model="osmosis", rgb_guidance=False, sample_pattern=None, tiling=tiling)
    call.update(kw)
    return sampler.p_sample_loop(**call)


def test_the_loop_rejects_a_bad_tiling_before_anything_launches():
    from osmosis_diffusion_code_amd.guided_diffusion import unet
    kw = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
              num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
              pretrain_model="osmosis")
    model = unet.create_model(**kw)               # on the CPU: any launch would raise "no CPU fallback"
    for tiling, msg in [(dict(tile=32, stride=8), "does not fit"), (dict(tile=16, stride=0), "stride"), (dict(tile=16, stride=17), "stride"),
                        (dict(tile=16, stride=8, window="box"), "window"), (dict(tile=16, stride=8, overlap=4), "unknown key"),
                        (dict(tile=(16, 18), stride=8), "divisible by 4"), (dict(tile=(6, 16), stride=4), "divisible by 4")]:
        with pytest.raises(ValueError, match=msg):
            _loop(tiling, model=model)
    # what the tiled loop does not carry raises NotImplementedError naming the option -- never the generic loop
    for kwargs, msg in [(dict(rgb_guidance=True), "rgb_guidance"), (dict(pretrain_model="imagenet"), "mean-only"),
                        (dict(sampler_kw=dict(name="ddim")), "ddim"), (dict(sampler_kw=dict(dynamic_threshold=True)), "dynamic_threshold"),
                        (dict(x=torch.zeros(2, 4, 24, 36)), "one canvas"), (dict(model=torch.nn.Identity()), "4 -> 8")]:
        kwargs.setdefault("model", model)
        with pytest.raises(NotImplementedError, match=msg):
            _loop(dict(tile=16, stride=8), **kwargs)


def test_restore_image_rejects_a_bad_tiling_from_argument_and_config_first():
    ref = torch.zeros(1, 3, 24, 36)
    for bad, msg in [({"tile": 16, "strides": 8}, "unknown key"), ({"tile": 32}, "does not fit"), ({"tile": 16, "window": "box"}, "window")]:
        with pytest.raises(ValueError, match=msg):
            sampling.restore_image(None, ref, {}, tiling=bad)
        with pytest.raises(ValueError, match=msg):
            sampling.restore_image(None, ref, {"tiling": bad})
        with pytest.raises(ValueError, match=msg):
            sampling.restore_images(None, [ref], {}, tiling=bad)


def test_tile_entries_are_exported_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "osmosis_hip.h")).read()
    for name in ("osm_tile_gather", "osm_tile_blend"):
        first, second = ("canvas", "tiles") if name.endswith("gather") else ("tiles", "canvas")
        assert re.search(rf"\bint\s+{name}\s*\(\s*const\s+float\s*\*\s*{first}\s*,\s*float\s*\*\s*{second}\s*,\s*const\s+int\s*\*\s*origins\s*,"
                         r"\s*const\s+float\s*\*\s*wy\s*,\s*const\s+float\s*\*\s*wx\s*,\s*const\s+float\s*\*\s*inv_norm\s*,\s*int\s+n\s*,"
                         r"\s*int\s+C\s*,\s*int\s+Hc\s*,\s*int\s+Wc\s*,\s*int\s+th\s*,\s*int\s+tw\s*,\s*void\s*\*\s*stream\s*\)", hdr), name
        assert name in _lib.exports("osmosis_hip.h") and len(_lib.SIGS[name]) == 13
    assert "tile.hip" in open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "Makefile")).read()


@pytest.mark.parametrize("name", ["osm_tile_gather", "osm_tile_blend"])
def test_tile_entries_validate_their_arguments_without_a_gpu(name):
    lib = _lib.load()
    fn = getattr(lib, name)
    P = 4096                                    # never dereferenced: validation fails first
    good = dict(n=4, C=4, Hc=40, Wc=52, th=32, tw=32)

    def call(a=P, b=P, org=P, wy=None, wx=None, inv=None, **dims):
        d = dict(good, **dims)
        return fn(a, b, org, wy, wx, inv, d["n"], d["C"], d["Hc"], d["Wc"], d["th"], d["tw"], None)
    assert call(a=None) != 0 and b"null pointer" in lib.osm_last_error()
    assert call(b=None) != 0 and b"null pointer" in lib.osm_last_error()
    assert call(org=None) != 0 and b"null pointer" in lib.osm_last_error()
    for ws in [dict(wy=P), dict(wx=P), dict(inv=P), dict(wy=P, wx=P), dict(wy=P, inv=P), dict(wx=P, inv=P)]:
        assert call(**ws) != 0 and b"together" in lib.osm_last_error(), ws
    for dims, msg in [(dict(n=0), b"tile count"), (dict(C=0), b"channel count"), (dict(Hc=0), b"canvas"), (dict(Wc=-1), b"canvas"),
                      (dict(th=41), b"does not fit"), (dict(tw=53), b"does not fit"), (dict(th=0), b"does not fit"),
                      (dict(C=1 << 20, Hc=1 << 10, Wc=1 << 10, th=8, tw=8), b"canvas")]:
        assert call(**dims) != 0, dims
        assert msg in lib.osm_last_error() and name.encode() in lib.osm_last_error(), (dims, lib.osm_last_error())


def test_tile_operators_are_registered_and_have_no_cpu_path():
    from osmosis_diffusion_code_amd import ops, torch_ops
    assert {"tile_gather", "tile_blend"} <= set(torch_ops.OPS)
    assert str(torch.ops.osmosis.tile_gather.default._schema) == (
        "osmosis::tile_gather(Tensor canvas, Tensor origins, SymInt th, SymInt tw, Tensor? wy=None, Tensor? wx=None, "
        "Tensor? inv_norm=None) -> Tensor")
    assert str(torch.ops.osmosis.tile_blend.default._schema) == (
        "osmosis::tile_blend(Tensor tiles, Tensor origins, SymInt Hc, SymInt Wc, Tensor? wy=None, Tensor? wx=None, "
        "Tensor? inv_norm=None) -> Tensor")
    z = torch.zeros
    org = torch.zeros(1, 2, dtype=torch.int32)
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.osmosis.tile_gather(z(4, 16, 24), org, 16, 24)
    with pytest.raises(_lib.OsmosisHipError, match="no CPU fallback"):
        ops.tile_gather(z(4, 16, 24), z(1, 4, 16, 24), org)
    with pytest.raises(_lib.OsmosisHipError, match="no CPU fallback"):
        ops.tile_blend(z(1, 4, 16, 24), z(4, 16, 24), org)
    with pytest.raises(_lib.OsmosisHipError, match="together"):
        ops.tile_blend(z(1, 4, 16, 24), z(4, 16, 24), org, wy=z(16))
    with pytest.raises(_lib.OsmosisHipError, match="origins"):
        ops.tile_gather(z(4, 16, 24), z(2, 4, 16, 24), org)
    from torch._subclasses.fake_tensor import FakeTensorMode
    with FakeTensorMode():
        e = lambda *s, **k: torch.empty(*s, device="cuda", **k)
        tiles = torch.ops.osmosis.tile_gather(e(8, 37, 45), e(20, 2, dtype=torch.int32), 16, 20, e(16), e(20), e(37, 45))
        assert tiles.shape == (20, 8, 16, 20)
        assert torch.ops.osmosis.tile_blend(tiles, e(20, 2, dtype=torch.int32), 37, 45).shape == (8, 37, 45)
