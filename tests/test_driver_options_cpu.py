"""The driver's plumbing of the data-term options (validity mask, range-map depth prior, robust term, gain field; `kernel`, `solver` /
`steps`), the parts that need no GPU: a stub sampler and a stub conditioner that return per-image distinct, deterministic values, so
that what `restore_image` / `restore_images` make of a chain's end is compared image by image between a batch and single images; and
the one declaration of every option's keys (`condition_methods.py`) that `p_sample_loop` and `sampling` both read."""
import numpy as np
import pytest
import torch

from osmosis_diffusion_code_amd import sampling
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M

H, W, GRID = 8, 6, (3, 4)
OKW = dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8", phi_inf="0.14, 0.29, 0.49")
MASK_KEYS = {"mask"}
DEPTH_KEYS = {"depth_prior", "depth_confidence", "depth_scale", "depth_shift", "depth_loss_final", "depth_align", "depth_metric", "phi_metric"}
ROBUST_KEYS = {"robust_weight", "robust_scale"}
GAIN_KEYS = {"gain_nodes", "gain_field", "flat_fielded"}
CHAIN_KEYS = {"kernel", "solver", "steps"}
OPTION_KEYS = MASK_KEYS | DEPTH_KEYS | ROBUST_KEYS | GAIN_KEYS | CHAIN_KEYS | {"tiling"}


def rows(tag, ids, *shape, lo=0.0, hi=1.0):
    """[len(ids), *shape]: row k depends on (tag, ids[k]) alone -- image ids[k]'s value however the images are batched."""
    return torch.stack([lo + (hi - lo) * torch.rand(shape, generator=torch.Generator().manual_seed(7919 * tag + i)) for i in ids])


class StubSampler:
    """`p_sample_loop` returns image (image_idx + b)'s tensors in row b and tells the conditioner which images the chain had."""
    solver, num_timesteps = "ddim", 7

    def __init__(self, seen):
        self.seen = seen

    def p_sample_loop(self, **kw):
        self.seen.append(kw)
        ids = range(kw["image_idx"], kw["image_idx"] + kw["x_start"].shape[0])
        cond = kw["measurement_cond_fn"].__self__
        cond.ids = ids
        sample = rows(1, ids, 4, H, W, lo=-1.0)
        if kw["rgb_guidance"]:
            return sample
        variables = {"phi_a": rows(2, ids, 3, 1, 1, lo=0.5), "phi_b": rows(3, ids, 3, 1, 1, lo=0.5), "phi_inf": rows(4, ids, 3, 1, 1)}
        return sample, variables, rows(5, ids).numpy(), rows(6, ids, 4, H, W, lo=-1.0)


class StubCond:
    """The conditioner's value readers over the chain's images, per-image distinct rows."""
    _depth = {"align": "scale"}

    def __init__(self, operator):
        self.operator, self.ids = operator, None

    def conditioning(self, **kw):
        raise AssertionError("the stub sampler never calls the conditioner")

    def depth_prior_values(self):
        return {"loss": rows(10, self.ids), "scale": rows(11, self.ids, lo=0.5, hi=2.0), "shift": torch.zeros(len(self.ids))}

    def depth_prior_rows(self, B, Hh, Ww, device):
        assert (B, Hh, Ww) == (len(self.ids), H, W)
        return rows(12, self.ids, 1, H * W, lo=1.0, hi=9.0), (rows(13, self.ids, 1, H * W) > 0.3).to(torch.float32)

    def robust_values(self):
        return {"weight": rows(14, self.ids, 3, H * W), "scale": rows(15, self.ids, lo=0.01)}

    def gain_values(self):
        return {"nodes": rows(16, self.ids, *GRID, lo=0.5), "field": rows(17, self.ids, 1, H * W, lo=0.5)}


class StubBlindOperator:
    """What the driver reads of a `blind_blur` operator that is no grid operator: the photo is the measurement, one PSF per chain."""
    degradation, device = None, "cpu"

    def reset(self):
        pass

    def kernel2d(self):
        return np.arange(9, dtype=np.float64).reshape(3, 3) / 36.0


@pytest.fixture
def seen(monkeypatch):
    calls = []
    monkeypatch.setattr(sampling, "create_sampler", lambda **kw: StubSampler(calls))
    monkeypatch.setattr(sampling, "get_conditioning_method", lambda name, operator, noiser, **kw: StubCond(operator))
    real = sampling.get_operator
    monkeypatch.setattr(sampling, "get_operator", lambda name, **kw: StubBlindOperator() if name == "blind_blur" else real(name, **kw))
    return calls


def config(branch, **measurement):
    if branch == "osmosis":
        operator, method, rgb = dict(OKW, name="underwater_physical_revised"), "osmosis", False
    else:
        operator, method, rgb = {"name": "blind_blur", "simulate": False}, "ps", True
    return {"measurement": dict(operator=operator, noise={"name": "clean"}, **measurement),
            "conditioning": {"method": method, "params": {}}, "diffusion": {}, "sample_pattern": {"pattern": "original"}, "aux_loss": {},
            "unet_model": {"pretrain_model": "osmosis"}, "rgb_guidance": rgb, "manual_seed": 3}


def photos(n):
    return [rows(20, [i], 3, H, W, lo=-0.9, hi=0.9) for i in range(n)]


def same(a, b, what):
    assert type(a) is type(b), what
    if isinstance(a, dict):
        assert set(a) == set(b), what
        for k in a:
            same(a[k], b[k], f"{what}[{k}]")
    elif isinstance(a, torch.Tensor):
        assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), what
    elif isinstance(a, np.ndarray):
        assert np.array_equal(a, b), what
    else:
        assert a == b, what


# ------------------------------------------------------------------------------------------------------------ [2, 1] against [1, 1, 1]
@pytest.mark.parametrize("branch", ["osmosis", "ps"])
def test_batches_of_two_and_one_against_three_batches_of_one(seen, branch):
    """Three photos as batches [2, 1] and as [1, 1, 1]: image by image the same keys and `torch.equal` values -- but for the three
    places where a batch is not the single image, asserted as they are: an image without a mask in a batch WITH masks gets ones
    (alone: no `mask`), one without a range map in a batch WITH maps gets the prior's keys (alone: none), and only a single
    image's result names the chain's `solver` / `steps` (the per-image results of a batch do not)."""
    imgs = photos(3)
    masks = [rows(21, [0], 1, H, W), None, rows(21, [2], 3, H, W)]
    kw = dict(masks=masks, robust={"loss": "huber"}, device="cpu")
    expect = MASK_KEYS | ROBUST_KEYS | CHAIN_KEYS                     # (`kernel`: the ps branch's operator learns a PSF)
    if branch == "osmosis":
        kw.update(depths=[rows(22, [0], 1, H, W, lo=1.0, hi=5.0), None, rows(22, [2], 1, H, W, lo=1.0, hi=5.0)])
        expect = expect - {"kernel"} | DEPTH_KEYS | GAIN_KEYS
    cfg = config(branch, **({"gain": {"grid": list(GRID)}} if branch == "osmosis" else {}))     # the ps branch has no gain field
    two = sampling.restore_images(None, imgs, cfg, batch_size=2, **kw)
    assert [c["x_start"].shape[0] for c in seen] == [2, 1]
    one = sampling.restore_images(None, imgs, cfg, batch_size=1, **kw)
    assert [c["x_start"].shape[0] for c in seen[2:]] == [1, 1, 1]
    assert sorted(two) == sorted(one) == [0, 1, 2]
    # images 0 and 2 carry every option; image 2 is alone in both runs
    same(two[2], one[2], "image 2")
    assert set(one[0]) & OPTION_KEYS == expect and set(one[2]) & OPTION_KEYS == expect
    assert set(one[0]) - set(two[0]) == {"solver", "steps"} and set(two[0]) - set(one[0]) == set()
    for k in set(two[0]):
        same(two[0][k], one[0][k], f"image 0 [{k}]")
    assert one[0]["solver"] == "ddim" and one[0]["steps"] == 7 and torch.equal(one[0]["mask"], masks[0].expand(1, 3, H, W))
    # image 1 has neither a mask nor a range map
    alone_lacks = MASK_KEYS | (DEPTH_KEYS if branch == "osmosis" else set())
    assert set(two[1]) - set(one[1]) == alone_lacks and set(one[1]) - set(two[1]) == {"solver", "steps"}
    for k in set(two[1]) & set(one[1]):
        same(two[1][k], one[1][k], f"image 1 [{k}]")
    assert torch.equal(two[1]["mask"], torch.ones(1, 3, H, W))
    assert "measurement_mask" not in seen[3] and "depth_prior" not in seen[3]
    if branch == "osmosis":
        assert float(seen[0]["depth_prior"]["confidence"][1].abs().max()) == 0.0        # no prior for it: confidence 0
        assert two[1]["depth_scale"] == float(rows(11, [1], lo=0.5, hi=2.0)[0])      # its own row of the chain's values


# ------------------------------------------------------------------------------------------------------------ restore_image, B = 2
def test_restore_image_keeps_image_0_of_a_batch(seen):
    ref = torch.cat(photos(2), 0)
    mask = rows(21, [0, 1], 1, H, W)
    depth = rows(22, [0, 1], 1, H, W, lo=1.0, hi=5.0)
    res = sampling.restore_image(None, ref, config("osmosis"), device="cpu", mask=mask, depth=depth, robust={"loss": "tukey"},
                                 gain={"grid": GRID})[-1]
    for k in ("sample", "pred_xstart", "measurement", "mask"):
        assert res[k].shape[0] == 2, k
    assert torch.equal(res["mask"], mask.expand(2, 3, H, W)) and torch.equal(res["measurement"], ref)
    assert torch.equal(res["sample"], rows(1, [0, 1], 4, H, W, lo=-1.0)) and torch.equal(res["pred_xstart"], rows(6, [0, 1], 4, H, W, lo=-1.0))
    assert torch.equal(res["rgb"], res["pred_xstart"][0, 0:3]) and res["phi"]["phi_a"].shape[0] == 2
    assert torch.equal(res["robust_weight"], rows(14, [0], 3, H * W).view(3, H, W)) and res["robust_scale"] == float(rows(15, [0], lo=0.01)[0])
    assert torch.equal(res["gain_nodes"], rows(16, [0], *GRID, lo=0.5)[0]) and torch.equal(res["gain_field"], rows(17, [0], 1, H * W, lo=0.5).view(H, W))
    assert torch.equal(res["flat_fielded"], ((ref[0] + 1.0) / (2.0 * res["gain_field"])).clamp(0.0, 1.0))
    assert torch.equal(res["depth_prior"], rows(12, [0], 1, H * W, lo=1.0, hi=9.0).view(H, W)) and res["depth_align"] == "scale"
    assert res["depth_scale"] == float(rows(11, [0], lo=0.5, hi=2.0)[0]) and res["depth_loss_final"] == float(rows(10, [0])[0])
    assert res["solver"] == "ddim" and res["steps"] == 7 and set(res) & OPTION_KEYS == MASK_KEYS | DEPTH_KEYS | ROBUST_KEYS | GAIN_KEYS | {"solver", "steps"}


# ------------------------------------------------------------------------------------------------------------ nothing given
@pytest.mark.parametrize("branch", ["osmosis", "ps"])
def test_no_option_no_keyword_and_no_key(seen, monkeypatch, branch):
    monkeypatch.setattr(StubSampler, "solver", None)
    cfg = config(branch)
    if branch == "ps":
        cfg["measurement"]["operator"] = {"name": "noise"}          # (no PSF to report either)
    for res in (sampling.restore_image(None, photos(1)[0], cfg, device="cpu")[-1],
                *sampling.restore_images(None, photos(2), cfg, device="cpu", batch_size=2).values()):
        assert not set(res) & OPTION_KEYS
    for call in seen:
        assert not set(call) & {"measurement_mask", "depth_prior", "robust", "gain_field", "tiling"}


# ------------------------------------------------------------------------------------------------------------ one declaration
class _Reached(Exception):
    pass


class RecordingCond:
    """A conditioner whose setters record what reaches them and end the call there."""
    def __init__(self):
        self.got = None

    def conditioning(self, **kw):
        raise AssertionError

    def _set(self, **kw):
        self.got = kw
        raise _Reached

    set_robust = set_gain_field = set_depth_prior = _set


def real_sampler():
    return gd.get_sampler("ddpm")(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                  model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False,
                                  clip_denoised=False, rescale_timesteps=False)


def loop_kw(cond):
    return dict(model=None, x_start=torch.zeros(1, 4, H, W), measurement=torch.zeros(1, 3, H, W), measurement_cond_fn=cond.conditioning,
                record=False, save_root=None, pretrain_model="osmosis")


DECLARED = {"robust": ("ConditioningMethod", "ROBUST_CHAIN_KEYS"), "gain_field": ("PosteriorSamplingOsmosis", "GAIN_FIELD_CHAIN_KEYS"),
            "depth_prior": ("PosteriorSamplingOsmosis", "DEPTH_PRIOR_CHAIN_KEYS")}


def declared(option):
    cls, name = DECLARED[option]
    return getattr(getattr(CM, cls), name)


@pytest.mark.parametrize("option", sorted(DECLARED))
def test_p_sample_loop_accepts_exactly_the_declared_keys(option):
    keys = declared(option)
    always = {"z": torch.ones(1, 1, H, W)} if option == "depth_prior" else {}
    cond = RecordingCond()
    with pytest.raises(_Reached):
        real_sampler().p_sample_loop(**{option: dict({k: 1 for k in keys}, **always)}, **loop_kw(cond))
    assert set(cond.got) - {"batch", "device"} == set(keys)
    every = {k for other in DECLARED for k in declared(other)} | {"path", "bogus"}
    for k in sorted(every - set(keys)):
        cond = RecordingCond()
        with pytest.raises(ValueError, match=rf"^{option}: unknown keys \['{k}'\]$"):
            real_sampler().p_sample_loop(**{option: dict(always, **{k: 1})}, **loop_kw(cond))
        assert cond.got is None


def test_the_config_keys_are_the_declared_ones_with_a_path_for_the_arrays():
    P = CM.PosteriorSamplingOsmosis
    assert sampling.ROBUST_KEYS == CM.ConditioningMethod.ROBUST_CHAIN_KEYS == ("loss", "c", "scale", "sigma_min", "per_pixel")
    assert sampling.GAIN_KEYS == ("grid", "eta", "n_iter", "smooth", "g_min", "learn", "path")
    assert set(sampling.GAIN_KEYS) == set(P.GAIN_FIELD_CHAIN_KEYS) - {"init"} | {"path"}
    assert sampling.DEPTH_PRIOR_KEYS == ("weight", "align", "loss", "scale", "scale_min", "path")
    assert set(sampling.DEPTH_PRIOR_KEYS) == set(P.DEPTH_PRIOR_CHAIN_KEYS) - {"z", "confidence"} | {"path"}


def test_unknown_config_keys_raise_before_the_sampler_runs(seen):
    ref = photos(1)[0]
    for key, known in (("robust", "loss, c, scale, sigma_min, per_pixel"), ("gain", "grid, eta, n_iter, smooth, g_min, learn, path"),
                       ("depth", "weight, align, loss, scale, scale_min, path")):
        with pytest.raises(ValueError, match=rf"^measurement\.{key}: unknown key\(s\) \['bogus'\] \(known: {known}\)$"):
            sampling.restore_image(None, ref, config("osmosis", **{key: {"bogus": 1}}), device="cpu")
    for arg in ("robust", "gain"):          # the argument wins over the config key, and is named in the message
        with pytest.raises(ValueError, match=rf"^{arg}: unknown key\(s\) \['bogus'\]"):
            sampling.restore_image(None, ref, config("osmosis", **{arg: {"loss": "huber"} if arg == "robust" else {"grid": [3, 3]}}),
                                   device="cpu", **{arg: {"bogus": 1}})
        with pytest.raises(ValueError, match=rf"^{arg} must be a mapping of "):
            sampling.restore_image(None, ref, config("osmosis"), device="cpu", **{arg: [1]})
    assert seen == []


# ------------------------------------------------------------------------------------------------------------ a conflicting pair
def test_gain_field_with_robust_is_refused_by_p_sample_loop():
    op = M.get_operator("underwater_physical_revised", device="cpu", batch_size=1, **OKW)
    cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), loss_function="norm", loss_weight="depth",
                                      weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True, gradient_clip="False,0",
                                      n_iter=1, pattern="pcgs")
    with pytest.raises(NotImplementedError, match="^gain_field: the gain field together with the robust data term"):
        real_sampler().p_sample_loop(gain_field={"grid": (3, 3)}, robust={"loss": "huber"}, **loop_kw(cond))
    assert cond._gain is not None and cond._gain["state"] is not None          # the field was set and opened first: the order stands
