"""The driver's plumbing of the data-term options on real chains: `restore_images(batch_size=2)` against `batch_size=1`, image by image,
key set and values, with several options at once.  The protocol of the other driver tests: the 48-channel seeded network, the
3-index low-noise sub-chain (`index_range=(2, 0), x_scale=0.05, noise_seed=7`) on 256 x 256 photos, `_generic_loop` patched to fail.

No bar is chosen here.  Between a batch of two and an image alone the network's rounding depends on the engine's batch, and the tests of
each option already hold that comparison to a bar; those are applied key by key:
    sample, pred_xstart                               2e-5            tests/test_physlin_gpu.py (batched driver test)
    depth_scale, depth_shift, depth_loss_final        1e-4 relative   tests/test_depthprior_gpu.py (`restore_images(batch_size=2, depths=)`)
    robust_scale                                      1e-4 relative   tests/test_robust_gpu.py (driver test, chunked batch)
    gain_nodes                                        1e-4            tests/test_gain_gpu.py (driver test, chunked batch)
What is the caller's own data handed through (`mask`, `depth_prior`, `depth_confidence`, `depth_align`, `measurement`) is equal bit for
bit.  The keys derived per pixel from the above (`robust_weight`, `gain_field`, `flat_fielded`, `depth_metric`, `phi_metric`) have no bar
of their own anywhere: their differences are printed with the rest and they must be finite where both are."""
import math

import pytest
import torch
from test_mask_gpu import AUX, COND, OPERATORS, PATTERN, model48, pkg  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUB = dict(index_range=(2, 0), x_scale=0.05, noise_seed=7)
DIFFUSION = dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type="learned_range",
                 dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False, timestep_respacing="10")
EXACT = ("mask", "depth_prior", "depth_confidence", "depth_align", "measurement", "kernel")
ABSOLUTE = {"sample": 2e-5, "pred_xstart": 2e-5, "gain_nodes": 1e-4}
RELATIVE = {"depth_scale": 1e-4, "depth_shift": 1e-4, "depth_loss_final": 1e-4, "robust_scale": 1e-4}
PRINTED = ("robust_weight", "gain_field", "flat_fielded", "depth_metric", "phi_metric")
DEPTH_KEYS = {"depth_prior", "depth_confidence", "depth_scale", "depth_shift", "depth_loss_final", "depth_align", "depth_metric", "phi_metric"}


def photos_and_masks(seed, n=3):
    g = torch.Generator().manual_seed(seed)
    photos = [(torch.rand(1, 3, 256, 256, generator=g) * 1.2 - 0.6).to(DEV) for _ in range(n)]
    masks = [(torch.rand(1, 1, 256, 256, generator=g) > 0.1).to(torch.float32) for _ in range(n)]
    for i, m in enumerate(masks):
        m[..., 30 + 10 * i:90, 100:180] = 0.0
    return photos, masks


def range_maps(seed, n=3):
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 256), torch.linspace(0, 1, 256), indexing="ij")
    zs = [(1.0 + (2.0 + i) * yy + 0.5 * xx + 0.05 * torch.randn(256, 256, generator=g))[None, None] for i in range(n)]
    for z in zs:
        z[..., 40:90, 100:180] = float("nan")                         # a hole in the range map
    return zs


def osmosis_cfg(operator, **measurement):
    return {"measurement": dict(operator=dict(OPERATORS[operator], name=operator), noise={"name": "clean"}, **measurement),
            "conditioning": {"method": "osmosis", "params": dict(COND)}, "diffusion": dict(DIFFUSION),
            "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
            "manual_seed": 0, "rgb_guidance": False}


def case(name):
    """(config, photos, keyword arguments of `restore_images`) of a case."""
    photos, masks = photos_and_masks({"a": 811, "b": 821, "c": 831}[name])
    if name == "a":         # revised underwater operator: mask + depths (the second photo without a map) + robust
        zs = range_maps(812)
        return (osmosis_cfg("underwater_physical_revised", depth=dict(weight=2.0, align="affine", loss="norm")), photos,
                dict(masks=masks, depths=[zs[0], None, zs[2]], robust=dict(loss="tukey")))
    if name == "b":         # haze operator: mask + depths + gain field
        return (osmosis_cfg("haze_physical", depth=dict(weight=2.0, align="scale", loss="mse")), photos,
                dict(masks=masks, depths=range_maps(822), gain=dict(grid=[5, 5], eta=0.05)))
    cfg = {"measurement": {"operator": {"name": "noise"}, "noise": {"name": "gaussian", "sigma": 0.0}, "robust": dict(loss="huber")},
           "conditioning": {"method": "ps", "params": dict(scale="0.3")}, "diffusion": dict(DIFFUSION, solver="ddim"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": True}
    return cfg, photos, dict(masks=masks)       # the rgb-guidance (`ps`) config with `solver: ddim`: mask + robust


def run_case(sampling, model, name, batch_size):
    cfg, photos, kw = case(name)
    return sampling.restore_images(model, photos, cfg, device=DEV, batch_size=batch_size, **kw, **SUB)


def max_diff(a, b):
    """max |a - b| over the entries that are finite in either, inf where only one is finite (phi_metric: over its tensors)."""
    if isinstance(a, dict):
        return max(max_diff(a[k], b[k]) for k in a)
    a, b = torch.as_tensor(a, dtype=torch.float64), torch.as_tensor(b, dtype=torch.float64)
    fa, fb = torch.isfinite(a), torch.isfinite(b)
    if bool((fa != fb).any()):
        return math.inf
    return float((a - b)[fa].abs().max()) if bool(fa.any()) else 0.0


@pytest.mark.parametrize("name", ["a", "b", "c"])
def test_a_batch_of_two_gives_every_image_the_option_keys_of_its_own_run(pkg, monkeypatch, model48, name):
    """Three photos as batches [2, 1] and alone.  The key sets agree but for what a batch does differently today and is kept: an
    image without a range map gets the prior's keys beside one that has a map (case a, image 1: confidence 0, an undefined fit),
    and only a single image's result names the chain's `solver` / `steps` (case c)."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    two, one = run_case(sampling, model48, name, 2), run_case(sampling, model48, name, 1)
    assert sorted(two) == sorted(one) == [0, 1, 2]
    worst = {}
    for i in range(3):
        batched = i < 2
        assert set(one[i]) - set(two[i]) == ({"solver", "steps"} if name == "c" and batched else set()), i
        assert set(two[i]) - set(one[i]) == (DEPTH_KEYS - {"phi_metric"} if name == "a" and i == 1 else set()), i
        if name == "c" and not batched:
            assert two[i]["solver"] == one[i]["solver"] == "ddim" and two[i]["steps"] == one[i]["steps"] == 10
        for k in set(two[i]) & set(one[i]):
            a, b = two[i][k], one[i][k]
            if k in EXACT:
                assert a == b if isinstance(a, str) else torch.equal(a, b), (i, k)
            elif k in ABSOLUTE or k in RELATIVE or k in PRINTED:
                worst[k] = max(worst.get(k, 0.0), max_diff(a, b))
                if k in ABSOLUTE:
                    assert max_diff(a, b) <= ABSOLUTE[k], (i, k, max_diff(a, b))
                elif k in RELATIVE:
                    assert abs(a - b) <= RELATIVE[k] * abs(b), (i, k, a, b)
                else:
                    assert math.isfinite(max_diff(a, b)), (i, k)
    print(f"DRIVEROPTIONS case {name}: batch of 2 vs alone, max |difference|: " + ", ".join(f"{k} {worst[k]:.2e}" for k in sorted(worst)))
    if name == "a":
        r = two[1]          # batched beside image 0 without a map of its own: no prior for it
        assert float(r["depth_confidence"].max()) == 0.0 and math.isnan(r["depth_scale"]) and bool(torch.isnan(r["depth_metric"]).all())
        assert all(k in two[i] for i in (0, 2) for k in ("robust_weight", "robust_scale", "mask", *DEPTH_KEYS - {"phi_metric"}))
    if name == "b":
        assert all(k in two[i] for i in range(3) for k in ("gain_nodes", "gain_field", "flat_fielded", "mask", *DEPTH_KEYS))
    if name == "c":
        assert all(k in two[i] for i in range(3) for k in ("robust_weight", "robust_scale", "mask")) and "pred_xstart" not in two[0]
