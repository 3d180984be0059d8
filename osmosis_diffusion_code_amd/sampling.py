"""Per-image driver contract of the reference's `osmosis_sampling.py` main loop (:117-345), as functions
(SURVEY.md section 8 rows a23 and N2): what the reference does around `p_sample_loop` for every image.

    restore_image(model, ref_img, cfg)      one image (or one independent batch) through the guided sampler
    postprocess(...)                        the outputs the reference saves / logs for that image
    restore_images(model, images, cfg, ...) a list of images, sharded images[rank::world] (section 8e)

`cfg` is the parsed YAML of the reference (`configs/osmosis_sample_config.yaml`): keys `measurement`
{operator, noise}, `conditioning` {method, params}, `diffusion`, `sample_pattern`, `aux_loss`, `unet_model`,
`manual_seed`, `degamma_input`, `rgb_guidance`.

    load_config(path)                       the YAML file -> that dictionary (osmosis_utils/utils.py:357-360,466-476)
    save_outputs(post, out_dir, name, ...)  the files the reference writes per image (osmosis_sampling.py:319-353)

Beyond the reference (which only ever writes 256 x 256 results):

    reconstruct_full_resolution(post, original, geometry, operator_cfg, ...)
                                            the physical model inverted on the ORIGINAL pixel grid from phi and the upsampled depth
    restore_image(..., tiling=) / config key `tiling: {tile, stride, window}`
                                            a photo larger than the network's grid sampled as overlapping tiles of the network's size
    tile_grid(Hc, Wc, tile, stride, window) the tiles of a canvas: origins, the separable window and the blend normalisation
"""
import os
from types import SimpleNamespace

import numpy as np
import torch

from .guided_diffusion.condition_methods import ConditioningMethod, PosteriorSamplingOsmosis, get_conditioning_method
from .guided_diffusion.gaussian_diffusion import create_sampler, parse_tiling, tile_grid  # noqa: F401  (tile_grid: public helper)
from .guided_diffusion.measurements import GRID_OPERATORS, PSFFieldOperator, get_noise, get_operator
from .osmosis_utils import utils as utilso
from .sharding import shard_indices


def global_iterations(sample_pattern):
    """osmosis_sampling.py:182-188."""
    if sample_pattern["pattern"] == "original":
        return 1
    if sample_pattern["pattern"] == "pcgs":
        return sample_pattern["global_N"]
    raise ValueError(f"Unrecognized sample pattern: {sample_pattern['pattern']}")


def degamma(y):
    """osmosis_sampling.py:173-175 (haze configs): [-1,1] image -> linear light, back to [-1,1]."""
    return 2 * torch.pow(0.5 * (y + 1), 2.2) - 1


def postprocess(out_xstart, variable_dict, ref_img, operator_cfg, loss=None, observed=None):
    """Outputs of one restored image (osmosis_sampling.py:199-300), all CPU tensors.

    out_xstart [B,4,H,W] (the final pred_xstart -- the reference saves THAT, not the final x_t), ref_img
    [B,3,H,W] in [-1,1]; like the reference only image 0 of the batch is post-processed.
    observed (a chain whose physical operator carries a `degradation` A; ref_img is then the photo on A's grid [B,3,h,w]):
    2 A forward_predicted - 1 of image 0, [3,h,w], computed by the caller with the chain's operator.  The result carries it as
    `observed`, `norm_loss_final` is taken against it, and `rgb_recon` (the closed form from the photo) is present only when the
    photo has the image's size."""
    out_xstart = out_xstart.detach().cpu()
    ref = ref_img.detach().cpu()
    ref_img_01 = 0.5 * (ref[0] + 1)
    sample_rgb = out_xstart[0, 0:-1, :, :]
    depth = out_xstart[0, -1, :, :].unsqueeze(0)
    rgb01 = 0.5 * (sample_rgb + 1)
    out = {
        "rgb": sample_rgb,
        "rgb_01": rgb01,
        "rgb_01_clip": torch.clamp(rgb01, min=0, max=1),
        "depth": depth,
        "depth_mm": utilso.min_max_norm_range(depth[0].unsqueeze(0)),
        "depth_pmm": utilso.min_max_norm_range_percentile(depth, vmin=0, vmax=1, percent_low=0.03,
                                                          percent_high=0.99, is_uint8=False),
    }
    depth_calc = utilso.convert_depth(depth.repeat(3, 1, 1), depth_type=operator_cfg["depth_type"],
                                      value=operator_cfg["value"])
    name = operator_cfg["name"]
    ones = torch.ones_like(sample_rgb)
    phi_inf = variable_dict["phi_inf"].cpu().squeeze(0) * ones
    if "underwater_physical_revised" in name:
        phi_a = variable_dict["phi_a"].cpu().squeeze(0) * ones
        phi_b = variable_dict["phi_b"].cpu().squeeze(0) * ones
    elif "haze" in name or "underwater_physical" in name:
        phi_a = phi_b = variable_dict["phi_ab"].cpu().squeeze(0) * ones
    else:
        raise NotImplementedError("Operator can be for 'underwater' or 'haze' ")
    backscatter = phi_inf * (1 - torch.exp(-phi_b * depth_calc))
    attenuation = torch.exp(-phi_a * depth_calc)
    forward_pred = rgb01 * attenuation + backscatter
    degraded = 2 * forward_pred - 1
    out.update(
        depth_calc=depth_calc, backscatter=backscatter, attenuation=attenuation,
        forward_predicted=forward_pred, degraded=degraded,
        phi={k: v.detach().cpu() for k, v in variable_dict.items()},
        loss=None if loss is None else np.asarray(loss),
    )
    if observed is None:
        out["norm_loss_final"] = float(np.round(torch.linalg.norm(degraded - ref).numpy(), decimals=3))
    else:
        observed = observed.detach().cpu()
        if tuple(observed.shape) != tuple(ref.shape[1:]):
            raise ValueError(f"observed must be {tuple(ref.shape[1:])} (the photo's grid), got {tuple(observed.shape)}")
        out["observed"] = observed
        out["norm_loss_final"] = float(np.round(torch.linalg.norm(observed - ref[0]).numpy(), decimals=3))
    if tuple(ref.shape[-2:]) == tuple(sample_rgb.shape[-2:]):
        out["rgb_recon"] = torch.exp(phi_a * depth_calc) * (ref_img_01 - backscatter)   # "clean" image from phi and the input
    return out


def observed_image(operator, out_xstart):
    """`postprocess`'s `observed` for a physical operator with a degradation: 2 A I - 1 of every image of the batch at the chain's
    final phi (per image), [B,3,h,w], computed on the operator's device (the degradation's own kernel); `postprocess` takes row 0,
    `postprocess_each` row b."""
    with torch.no_grad():
        return 2 * operator.observe(out_xstart.detach().to(operator.device, torch.float32).contiguous()) - 1


def _refuse_unknown_keys(where, given, known, also=()):
    """`where`: unknown key(s) ... (known: ...) for a mapping with keys outside `known` (+ `also`, accepted but not advertised)."""
    unknown = set(given) - set(known) - set(also)
    if unknown:
        raise ValueError(f"{where}: unknown key(s) {sorted(unknown)} (known: {', '.join(known)})")


def _option_mapping(argument, name, config_value, config_key, known, also=()):
    """An option given as an argument (a dict, which wins) or under a config key: (a copy of the chosen mapping, or None when
    neither is given; how to name it in a message).  Anything but a mapping raises, and so do unknown keys."""
    chosen, where = (argument, name) if argument is not None else (config_value, config_key)
    if not chosen:
        return None, where
    if not isinstance(chosen, dict):
        raise ValueError(f"{where} must be a mapping of {', '.join(known)}")
    _refuse_unknown_keys(where, chosen, known, also)
    return dict(chosen), where


# The keys a config can carry for each option: what the option's setter takes from a chain (declared beside it in
# condition_methods.py), with a `path` to a .npy in the place of the arrays.
DEPTH_PRIOR_KEYS = tuple(k for k in PosteriorSamplingOsmosis.DEPTH_PRIOR_CHAIN_KEYS if k not in ("z", "confidence")) + ("path",)
ROBUST_KEYS = ConditioningMethod.ROBUST_CHAIN_KEYS
GAIN_KEYS = tuple(k for k in PosteriorSamplingOsmosis.GAIN_FIELD_CHAIN_KEYS if k != "init") + ("path",)


def depth_prior_config(depth_cfg):
    """The optional config key `measurement.depth: {weight, align, loss, scale, scale_min, path}` as keyword arguments of
    `set_depth_prior` (only the keys given) and the `path` of a `.npy` range map at the photo's resolution (or None).  Unknown keys
    raise."""
    if not depth_cfg:
        return {}, None
    _refuse_unknown_keys("measurement.depth", depth_cfg, DEPTH_PRIOR_KEYS)
    params = {k: depth_cfg[k] for k in ("align", "loss") if k in depth_cfg}
    params.update({k: float(depth_cfg[k]) for k in ("weight", "scale", "scale_min") if k in depth_cfg})
    return params, depth_cfg.get("path")


def robust_config(robust_cfg=None, robust=None):
    """The `robust=` dict of a chain (`p_sample_loop(robust=)`, `ConditioningMethod.set_robust`) from the optional config key
    `measurement.robust: {loss, c, scale, sigma_min, per_pixel}` or the argument `robust` (a dict, which wins over the config), or
    None when neither is given.  Unknown keys raise."""
    return _option_mapping(robust, "robust", robust_cfg, "measurement.robust", ROBUST_KEYS)[0]


def gain_nodes_from_flat_field(flat, grid):
    """The [gh,gw] nodes whose bilinear field (include/osmosis_gain.h: nodes on the image corners) is closest in least squares to a
    full-resolution flat field [H,W] > 0, on the host in float64; scaled to max = 1."""
    from .ops import gain_tables_host
    flat = np.asarray(flat, dtype=np.float64)
    if flat.ndim != 2 or not np.isfinite(flat).all() or not (flat > 0).all():
        raise ValueError(f"measurement.gain: a flat field must be a finite [H,W] array > 0, got shape {flat.shape}")
    gh, gw = grid
    H, W = flat.shape
    iy0, fy, ix0, fx = gain_tables_host(H, W, gh, gw)

    def hat(i0, f, g):
        Hm = np.zeros((i0.shape[0], g))
        Hm[np.arange(i0.shape[0]), i0] += 1.0 - f.astype(np.float64)
        Hm[np.arange(i0.shape[0]), i0 + 1] += f.astype(np.float64)
        return Hm
    Hy, Hx = hat(iy0, fy, gh), hat(ix0, fx, gw)
    nodes = np.linalg.pinv(Hy) @ flat @ np.linalg.pinv(Hx).T         # argmin ||Hy n Hx^T - flat||_F (both have full column rank)
    if not (nodes > 0).all():
        raise ValueError("measurement.gain: the flat field's least-squares nodes are not all > 0")
    return nodes / nodes.max()


def gain_config(gain_cfg=None, gain=None, grid_hw=None):
    """The `gain_field=` dict of a chain (`p_sample_loop(gain_field=)`, `PosteriorSamplingOsmosis.set_gain_field`) from the optional
    config key `measurement.gain: {grid, eta, n_iter, smooth, g_min, learn, path}` or the argument `gain` (a dict, which wins over
    the config; it may carry `init` nodes instead of `path`), or None when neither is given.  `path`: a .npy of nodes [gh,gw] or of a
    full-resolution flat field [H,W] on the network's grid `grid_hw`, reduced to nodes by least squares.  Unknown keys raise."""
    out, where = _option_mapping(gain, "gain", gain_cfg, "measurement.gain", GAIN_KEYS, also=("init",))
    if out is None:
        return None
    out["grid"] = tuple(int(v) for v in out.get("grid", (5, 5)))
    path = out.pop("path", None)
    if path is not None:
        if out.get("init") is not None:
            raise ValueError(f"{where}: give `path` or `init`, not both")
        arr = np.load(path)
        if arr.ndim == 2 and tuple(arr.shape) == out["grid"]:
            out["init"] = np.asarray(arr, dtype=np.float64)
        elif arr.ndim == 2 and (grid_hw is None or tuple(arr.shape) == tuple(grid_hw)):
            out["init"] = gain_nodes_from_flat_field(arr, out["grid"])
        else:
            raise ValueError(f"{where}: {path} holds {arr.shape}: neither nodes {out['grid']} nor a flat field on the grid {grid_hw}")
    return out


def attach_gain(post, nodes, field, y):
    """The gain field's keys of one image's result: `gain_nodes` [gh,gw], `gain_field` [H,W] (both of the chain's last guided
    sub-step) and `flat_fielded` = clip((y + 1) / (2 G), 0, 1) [3,H,W], the photo with the field divided out."""
    G = field.detach().cpu().to(torch.float32).view(y.shape[-2], y.shape[-1])
    post.update(gain_nodes=nodes.detach().cpu().to(torch.float32), gain_field=G,
                flat_fielded=((y.detach().cpu().to(torch.float32) + 1.0) / (2.0 * G)).clamp(0.0, 1.0))
    return post


def attach_robust(post, weight, scale):
    """The robust term's keys of one image's result: `robust_weight` (omega [3,h,w] of the chain's last guided sub-step, on the
    measurement's grid) and `robust_scale` (its sigma)."""
    post.update(robust_weight=weight.detach().cpu().to(torch.float32), robust_scale=float(scale))
    return post


def depth_prior_inputs(grid, depth_cfg=None, depth=None, depth_confidence=None, geometry=None):
    """The `depth_prior=` dict of a chain whose images live on `grid` = (H, W), or None when no range map is given.  depth /
    depth_confidence: [B,1,H,W], [1,1,H,W] or [B,H,W] on the network's grid (`data.transform_range` takes one from the photo's
    resolution there); without `depth`, the `.npy` of `measurement.depth.path` at the photo's resolution goes through
    `transform_range` with `geometry` (the photo's `data.Geometry`, as `fit_transform` returned it).  Without a geometry the
    photo's transform is NOT known here and is assumed to be the default one for the grid: the [size, size] center crop of
    `default_transform` for a square grid, `fit_transform`'s grid with its default multiple otherwise; a photo that was prepared
    differently needs `geometry` or a ready-made `depth`.  `path` is ONE file: with B > 1 its map serves every image of the batch
    (one scene), per-image maps go through `depth=` / `restore_images(depths=)`."""
    params, path = depth_prior_config(depth_cfg)
    if depth is None and path is None:
        if depth_confidence is not None:
            raise ValueError("depth_confidence comes with a range map (`depth=` or measurement.depth.path)")
        return None
    H, W = int(grid[0]), int(grid[1])
    if depth is None:
        from .osmosis_utils import data as datao
        if geometry is not None:
            depth, conf = datao.transform_range(np.load(path), geometry=geometry)
        else:
            depth, conf = datao.transform_range(np.load(path), size=min(H, W), crop="center" if H == W else "fit")
        if depth_confidence is None:
            depth_confidence = conf
        else:
            depth_confidence = torch.as_tensor(depth_confidence).to(torch.float32) * conf
    depth = torch.as_tensor(depth)
    if tuple(depth.shape[-2:]) != (H, W):
        raise ValueError(f"the range map {tuple(depth.shape)} does not match the image grid {(H, W)} (the prior lives on the image's "
                         "grid, also with a degradation)")
    return dict(params, z=depth, confidence=depth_confidence)


def attach_depth_prior(post, z, m, scale, shift, loss, align):
    """The range prior's keys of one image's result (`post` from `postprocess`): `depth_prior` (z [H,W]), `depth_confidence` [H,W],
    `depth_scale` / `depth_shift` (the fit d ~ a z + c at the chain's end), `depth_loss_final`, `depth_metric` [H,W] =
    (depth_calc - c) / a -- the depth in the range map's unit, NaN where a is undefined (a guard skipped the image) -- and, when
    align is 'scale' or 'none' (c = 0, so exp(-phi d) = exp(-(phi a) z)), `phi_metric`: phi_a a and phi_b a (phi_ab a) per unit of
    range, phi_inf unchanged."""
    a, c = float(scale), float(shift)
    H, W = post["depth_calc"].shape[-2:]
    post.update(depth_prior=z.detach().cpu().reshape(H, W).to(torch.float32), depth_confidence=m.detach().cpu().reshape(H, W).to(torch.float32),
                depth_scale=a, depth_shift=c, depth_loss_final=float(loss), depth_align=align)
    dc = post["depth_calc"][0].to(torch.float64)
    post["depth_metric"] = ((dc - c) / a).to(torch.float32) if (np.isfinite(a) and np.isfinite(c) and a != 0.0) \
        else torch.full((H, W), float("nan"))
    if align in ("scale", "none") and np.isfinite(a):
        post["phi_metric"] = {k: (v.clone() if k == "phi_inf" else v * a) for k, v in post["phi"].items()}
    return post


def load_config(path):
    """The reference's `arguments_from_file` (osmosis_utils/utils.py:466-476 -> load_yaml :357-360): the YAML file as a plain
    dictionary (the reference copies the same keys onto an argparse.Namespace; `restore_image(s)` reads them by key).
    yaml.FullLoader like the reference, so `1e-5` stays the STRING the operators parse themselves and `32, 16, 8` a string."""
    import yaml
    with open(path) as f:
        cfg = yaml.load(f, Loader=yaml.FullLoader)
    if not isinstance(cfg, dict):
        raise ValueError(f"{path}: expected a mapping at the top level of the configuration file")
    return cfg


def _to_pil_u8(t):
    """torchvision.transforms.functional.to_pil_image on a float tensor [C,H,W] (0.14.1, functional.py:257-340 as the
    reference uses it at osmosis_sampling.py:321-337): `pic.mul(255).byte()` -- TRUNCATION, not rounding -- then HWC;
    one channel -> mode 'L', three -> 'RGB'."""
    if t.dim() == 2:
        t = t.unsqueeze(0)
    if t.dim() != 3 or t.shape[0] not in (1, 3):
        raise ValueError(f"pic should be 2/3 dimensional with 1 or 3 channels. Got {tuple(t.shape)}")
    if t.is_floating_point():
        t = t.mul(255).byte()
    arr = t.permute(1, 2, 0).contiguous().numpy()
    return arr[:, :, 0] if arr.shape[2] == 1 else arr


def make_grid(tensors, nrow=8, padding=2, pad_value=0.0):
    """torchvision.utils.make_grid (0.14.1) for a list of equally sized [C,H,W] tensors, normalize=False: the list is stacked
    (dtype promotion as torch.stack does it: the viridis depth is float64), single-channel images are repeated to three, tile k
    sits at row k // xmaps, column k % xmaps of a (pad_value)-filled canvas with `padding` pixels before every tile and after
    the last one."""
    dt = tensors[0].dtype
    for t in tensors[1:]:
        dt = torch.promote_types(dt, t.dtype)
    x = torch.stack([t.to(dt) for t in tensors], 0)
    if x.shape[1] == 1:
        x = x.repeat(1, 3, 1, 1)
    if x.shape[0] == 1:              # make_grid returns the single image itself (no border)
        return x[0]
    n = x.shape[0]
    xmaps = min(nrow, n)
    ymaps = (n + xmaps - 1) // xmaps
    h, w = x.shape[2] + padding, x.shape[3] + padding
    grid = x.new_full((x.shape[1], h * ymaps + padding, w * xmaps + padding), pad_value)
    for k in range(n):
        r, c = divmod(k, xmaps)
        grid[:, r * h + padding: r * h + padding + x.shape[2], c * w + padding: c * w + padding + x.shape[3]] = x[k]
    return grid


def _replicate_to(img, hw):
    """[C,h,w] -> [C,H,W] by pixel replication (nearest neighbour): a measurement of a downsampling operator beside its sample in
    a grid; an image already of that size is returned as it is."""
    if tuple(img.shape[-2:]) == tuple(hw):
        return img
    ri = (torch.arange(hw[0]) * img.shape[-2]) // hw[0]
    ci = (torch.arange(hw[1]) * img.shape[-1]) // hw[1]
    return img[:, ri][:, :, ci]


def output_images(post, ref_img, gt_rgb_01=None, gt_depth_01=None):
    """The uint8 arrays of the five images the reference writes for one restored image (osmosis_sampling.py:319-353):
    `input` = the reference image in [0,1], `rgb` = the clipped restoration, `depth_color` = viridis of the percentile-normalised
    depth, `depth_raw` = the min-max-normalised depth (one channel), `grid` = make_grid([input, rgb, depth_color] (+ [zeros,
    gt rgb, gt depth colour] when a ground truth exists: :341-344), nrow=3, pad_value=1.) through the reference's
    clip_image(scale=False, move=False, is_uint8=True) (clamp, truncate).
    A result without depth entries (`rgb_guidance_result` of a 3-channel sample): `input`, `rgb` and the grid of those two tiles
    (+ the ground-truth rgb)."""
    ref01 = 0.5 * (ref_img.detach().cpu()[0] + 1)
    if "depth_pmm" not in post:
        tiles = [_replicate_to(ref01, post["rgb_01_clip"].shape[-2:]), post["rgb_01_clip"]] + ([] if gt_rgb_01 is None else [gt_rgb_01])
        grid = make_grid(tiles, nrow=3, pad_value=1.0)
        grid = (grid * 255).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
        return {"input": _to_pil_u8(ref01), "rgb": _to_pil_u8(post["rgb_01_clip"]), "grid": grid}
    col = depth_color(post)
    tiles = [_replicate_to(ref01, post["rgb_01_clip"].shape[-2:]), post["rgb_01_clip"], col]
    if gt_rgb_01 is not None:
        tiles += [torch.zeros_like(post["rgb_01"]), gt_rgb_01, utilso.depth_tensor_to_color_image(gt_depth_01)]
    grid = make_grid(tiles, nrow=3, pad_value=1.0)
    grid = (grid * 255).clamp(0, 255).to(torch.uint8).permute(1, 2, 0).contiguous().numpy()
    return {"input": _to_pil_u8(ref01), "rgb": _to_pil_u8(post["rgb_01_clip"]), "depth_color": _to_pil_u8(col),
            "depth_raw": _to_pil_u8(post["depth_mm"]), "grid": grid}


def save_outputs(post, ref_img, out_dir, name, global_ii=0, save_singles=True, save_grids=True, gt_rgb_01=None,
                 gt_depth_01=None, rgb_guidance=None, full_res=None):
    # (a result that carries `mask` -- a chain guided through a validity mask -- also gets single_images/mask/<name>_mask.png)
    """Writes what the reference writes for one image (osmosis_sampling.py:84-104 directory layout, :319-353 files):
    `<out_dir>/single_images/{input,rgb,depth_color,depth_raw}/<name>.png` and `<out_dir>/grid_results/<name>_g<ii>_grid.png`.
    Returns {kind: path}.  (`<name>_process.png` is written by the sampler itself when `record` is on.)
    A result of the rgb-guidance branch (`restore_image` with `rgb_guidance: True`: the dict carries `sample`, no phi; override
    with `rgb_guidance=`) is written as the reference's second branch writes it (:382-401): the same four single images -- the
    min-max depth as a three-channel PNG, it is `depth.repeat(3, 1, 1)` there -- and the grid as `<name>.png`.
    `full_res` (a result of `reconstruct_full_resolution`) adds `<out_dir>/full_resolution/<name>_recon_full.png` and
    `<name>_depth_full.png` (viridis of the percentile-normalised full-resolution depth); without it nothing else is written."""
    if rgb_guidance is None:
        rgb_guidance = "sample" in post and "phi" not in post
    from PIL import Image
    imgs = output_images(post, ref_img, gt_rgb_01, gt_depth_01)
    paths = {}
    if save_singles:
        for kind in (k for k in ("input", "rgb", "depth_color", "depth_raw") if k in imgs):
            d = os.path.join(out_dir, "single_images", kind)
            os.makedirs(d, exist_ok=True)
            paths[kind] = os.path.join(d, f"{name}.png")
            Image.fromarray(imgs[kind], mode="L" if imgs[kind].ndim == 2 else "RGB").save(paths[kind])
    if save_singles and post.get("mask") is not None:       # only when the chain used a validity mask
        d = os.path.join(out_dir, "single_images", "mask")
        os.makedirs(d, exist_ok=True)
        paths["mask"] = os.path.join(d, f"{name}_mask.png")
        Image.fromarray(_to_pil_u8(post["mask"][0].clamp(0, 1)), mode="RGB").save(paths["mask"])
    if save_singles and post.get("robust_weight") is not None:      # only a chain with the robust data term
        d = os.path.join(out_dir, "single_images", "robust")
        os.makedirs(d, exist_ok=True)
        paths["robust"] = os.path.join(d, f"{name}_robust.png")
        lo = post["robust_weight"].to(torch.float32).amin(dim=0).clamp(0.0, 1.0)        # the per-pixel minimum of omega over the channels
        Image.fromarray((lo * 255.0 + 0.5).to(torch.uint8).numpy(), mode="L").save(paths["robust"])
    if save_singles and post.get("gain_field") is not None:         # only a chain with a gain field
        d = os.path.join(out_dir, "single_images", "gain")
        os.makedirs(d, exist_ok=True)
        paths["gain"] = os.path.join(d, f"{name}_gain.png")
        Image.fromarray((post["gain_field"].to(torch.float32).clamp(0.0, 1.0) * 255.0 + 0.5).to(torch.uint8).numpy(), mode="L").save(paths["gain"])
    if save_singles and post.get("depth_metric") is not None:       # only a chain with a range-map prior
        d = os.path.join(out_dir, "single_images", "depth_metric")
        os.makedirs(d, exist_ok=True)
        metric_u8, prior_u8 = depth_metric_images_u8(post)
        paths["depth_metric"] = os.path.join(d, f"{name}_depth_metric.png")
        paths["depth_prior"] = os.path.join(d, f"{name}_depth_prior.png")
        Image.fromarray(metric_u8, mode="RGB").save(paths["depth_metric"])
        Image.fromarray(prior_u8, mode="RGB").save(paths["depth_prior"])
    if save_singles and post.get("kernel") is not None:     # a `blind_blur` chain: the learnt PSF ([3,k,k] per channel: one RGB picture); `field_blur`: the mosaic of the node kernels
        d = os.path.join(out_dir, "single_images", "kernel")
        os.makedirs(d, exist_ok=True)
        paths["kernel"] = os.path.join(d, f"{name}_kernel.png")
        u8 = kernel_image_u8(post["kernel"])
        Image.fromarray(u8, mode="L" if u8.ndim == 2 else "RGB").save(paths["kernel"])
    if save_grids:
        d = os.path.join(out_dir, "grid_results")
        os.makedirs(d, exist_ok=True)
        paths["grid"] = os.path.join(d, f"{name}.png" if rgb_guidance else f"{name}_g{global_ii}_grid.png")
        Image.fromarray(imgs["grid"], mode="RGB").save(paths["grid"])
    if full_res is not None:
        d = os.path.join(out_dir, "full_resolution")
        os.makedirs(d, exist_ok=True)
        paths["recon_full"] = os.path.join(d, f"{name}_recon_full.png")
        Image.fromarray(full_res["rgb_recon_full_u8"].numpy(), mode="RGB").save(paths["recon_full"])
        paths["depth_full"] = os.path.join(d, f"{name}_depth_full.png")
        Image.fromarray(full_depth_color_u8(full_res), mode="RGB").save(paths["depth_full"])
    return paths


def depth_metric_images_u8(post):
    """(`depth_metric`, `depth_prior`) of a result as viridis uint8 [H,W,3] images under ONE normalisation: the range of the valid
    range-map pixels and the finite metric depths together, so equal colours are equal ranges; pixels without a value are black."""
    metric, z, m = post["depth_metric"].to(torch.float64), post["depth_prior"].to(torch.float64), post["depth_confidence"]
    have_m, have_z = torch.isfinite(metric), m > 0
    vals = torch.cat([metric[have_m], z[have_z]])
    lo, hi = (float(vals.min()), float(vals.max())) if vals.numel() else (0.0, 1.0)
    span = hi - lo if hi > lo else 1.0
    out = []
    for plane, have in ((metric, have_m), (z, have_z)):
        norm = torch.where(have, ((plane - lo) / span).clamp(0, 1), torch.zeros_like(plane))
        col = utilso.depth_tensor_to_color_image(norm) * have.to(torch.float64)
        out.append(_to_pil_u8(col.to(torch.float32)))
    return out[0], out[1]


def kernel_image_u8(kernel, side=128):
    """uint8 [k z, k z] picture of a PSF [k, k]: the kernel over its maximum (negative values clamped to 0), every tap replicated to a
    z x z block of pixels, z = max(1, side // k) -- no interpolation, a tap stays a square.  A per-channel PSF [3, k, k]: one RGB
    picture uint8 [k z, k z, 3], every plane over the COMMON maximum.  A field [gh, gw, kh, kw]: the gh x gw mosaic of the node
    kernels (node (jy, jx) in block row jy, block column jx) over their common maximum, uint8 [gh kh z, gw kw z]."""
    k = torch.as_tensor(kernel, dtype=torch.float32).clamp(min=0)
    if k.dim() == 4:        # a field of PSFs [gh,gw,kh,kw] (`field_blur`): the gh x gw mosaic of the node kernels, one common maximum
        gh, gw, kh, kw = k.shape
        k = k.permute(0, 2, 1, 3).reshape(gh * kh, gw * kw)
    top = float(k.max())
    k = k / top if top > 0 else k
    z = max(1, int(side) // int(max(k.shape[-2:])))
    u8 = (k * 255.0 + 0.5).clamp(0, 255).to(torch.uint8)
    u8 = u8.repeat_interleave(z, dim=-2).repeat_interleave(z, dim=-1)
    return (u8.permute(1, 2, 0) if u8.dim() == 3 else u8).contiguous().numpy()


def full_depth_color_u8(full_res):
    """uint8 [Hc,Wc,3] viridis of the percentile-normalised full-resolution depth (the helpers and percentiles of `depth_color`)."""
    d = full_res["depth_full"].unsqueeze(0)
    if d.numel() <= 1 << 24:
        pmm = utilso.min_max_norm_range_percentile(d, vmin=0, vmax=1, percent_low=0.03, percent_high=0.99, is_uint8=False)
    else:       # torch.quantile stops at 2^24 elements (a 16.7-megapixel photo): the same quantiles from exact order statistics
        flat = d.reshape(-1)

        def quantile(q):
            pos = q * (flat.numel() - 1)
            k = int(pos)
            lo = flat.kthvalue(k + 1)[0]
            return lo + (flat.kthvalue(min(k + 2, flat.numel()))[0] - lo) * (pos - k)
        pmm = utilso.min_max_norm_range(torch.clamp(d, quantile(0.03), quantile(0.99)), vmin=0, vmax=1)
    return _to_pil_u8(utilso.depth_tensor_to_color_image(pmm))


UPSAMPLE_MODES = {"bilinear": 0, "joint_bilateral": 1}


def reconstruct_full_resolution(post, original, geometry, operator_cfg, upsample="bilinear", device=None, radius=2,
                                sigma_s=1.0, sigma_r=0.1):
    """`rgb_recon` at the photo's own resolution: exp(phi_a D) (I - phi_inf (1 - exp(-phi_b D))) with I = the ORIGINAL image and
    D = convert_depth of the network's depth map upsampled to the original pixel grid (one HIP kernel, osm_recon_fullres).

    post: a result dict of `postprocess` / `restore_image` (its `pred_xstart`, `phi` and `measurement` are read, image 0);
    original: the `to_tensor` photo [3,H0,W0] in [0,1], used as the 256-class path uses `ref_img` (no degamma);
    geometry: `data.transform_geometry(H0, W0, ...)` of the transform that produced the sampler's input;
    upsample: "bilinear", or "joint_bilateral" (joint bilateral upsampling guided by the photo; `radius`, `sigma_s` in network
    pixels, `sigma_r` in [0,1] intensity -- parameters, not tuned values).
    Returns CPU tensors: rgb_recon_full [3,Hc,Wc] (unclipped), rgb_recon_full_u8 [Hc,Wc,3], depth_full [Hc,Wc] (raw network depth)
    and `rect` = (y0, x0, Hc, Wc), the covered rectangle of the photo.  At identity geometry rgb_recon_full is `rgb_recon`."""
    from . import ops
    if upsample not in UPSAMPLE_MODES:
        raise ValueError(f"upsample must be one of {sorted(UPSAMPLE_MODES)}, got {upsample!r}")
    x0 = post["pred_xstart"]
    device = device if device is not None else (x0.device if x0.is_cuda else "cuda")
    h, w = x0.shape[-2:]
    if (h, w) != (geometry.h, geometry.w):
        raise ValueError(f"the result is {h} x {w} but the geometry describes a {geometry.h} x {geometry.w} network grid")
    if original.dim() != 3 or tuple(original.shape) != (3, geometry.H0, geometry.W0):
        raise ValueError(f"original must be [3,{geometry.H0},{geometry.W0}], got {tuple(original.shape)}")
    name = operator_cfg["name"]
    phi = post["phi"]
    if "underwater_physical_revised" in name:
        pa, pb = phi["phi_a"], phi["phi_b"]
    elif "haze" in name or "underwater_physical" in name:
        pa = pb = phi["phi_ab"]
    else:
        raise NotImplementedError("Operator can be for 'underwater' or 'haze' ")

    def vec3(p):        # image 0 of [B,3,1,1] / [B,1,1,1] -> fp32 [3] on the device
        return p.detach().to(device=device, dtype=torch.float32)[0].reshape(-1).expand(3).contiguous()
    code, dval = utilso.depth_code_and_values(operator_cfg["depth_type"], operator_cfg["value"])
    y0, xl, Hc, Wc = geometry.y0, geometry.x0, geometry.Hc, geometry.Wc
    image = original[:, y0:y0 + Hc, xl:xl + Wc].to(device=device, dtype=torch.float32).contiguous()
    depth = x0[0, -1].detach().to(device=device, dtype=torch.float32).contiguous()
    guide = (0.5 * (post["measurement"][0].detach().to(device=device, dtype=torch.float32) + 1)).contiguous()
    rgb = torch.empty((3, Hc, Wc), device=device, dtype=torch.float32)
    u8 = torch.empty((Hc, Wc, 3), device=device, dtype=torch.uint8)
    full = torch.empty((Hc, Wc), device=device, dtype=torch.float32)
    ops.recon_fullres(depth, guide, image, vec3(pa), vec3(pb), vec3(phi["phi_inf"]), code, dval, geometry.rect_map(), rgb, u8, full,
                      UPSAMPLE_MODES[upsample], radius, sigma_s, sigma_r)
    return {"rgb_recon_full": rgb.cpu(), "rgb_recon_full_u8": u8.cpu(), "depth_full": full.cpu(), "rect": (y0, xl, Hc, Wc),
            "upsample": upsample}


def depth_color(post):
    """viridis rendering of the percentile-normalised depth (what the reference writes to depth_pmm_color)."""
    return utilso.depth_tensor_to_color_image(post["depth_pmm"])


def rgb_guidance_result(sample, measurement):
    """What the reference driver derives from the sample of an rgb-guidance / non-osmosis chain (osmosis_sampling.py:366-380; image 0
    of `sample`): RGB and depth split, the clipped [0, 1] RGB, the min-max and the percentile-normalised three-channel depth.  No phi,
    no recomposition.  CPU tensors.  A 3-channel sample (the RGB model family) has no depth plane: its three planes are `rgb`, and
    the result has no depth entries."""
    if sample.shape[1] == 3:
        return {"sample": sample, "rgb": sample[0], "rgb_01_clip": torch.clamp(0.5 * (sample[0] + 1), 0, 1), "measurement": measurement}
    depth3 = sample[0, -1].repeat(3, 1, 1)
    return {"sample": sample, "rgb": sample[0, 0:-1], "rgb_01_clip": torch.clamp(0.5 * (sample[0, 0:-1] + 1), 0, 1),
            "depth_mm": utilso.min_max_norm_range(depth3, vmin=0, vmax=1, is_uint8=False),
            "depth_pmm": utilso.min_max_norm_range_percentile(depth3, percent_low=0.05, percent_high=0.99),
            "measurement": measurement}


def measurement_grid(operator_cfg, hw):
    """(h, w) of the measurement `restore_image` derives from an image of size hw: the operator's `out_shape` for a blur /
    super-resolution operator that simulates its measurement, hw itself otherwise (every other operator; `simulate: False`,
    where the image handed in IS the measurement)."""
    from .guided_diffusion import measurements
    cls = measurements.__OPERATOR__.get(operator_cfg.get("name"))
    if operator_cfg.get("degradation") is not None:
        # a physical operator with a degradation: the image handed in IS the measurement, so is its grid (the chain's image lives on
        # the network's grid, `model_grid`, whose `out_shape` this must be); the name is checked against the registry, nothing is built
        deg = operator_cfg["degradation"]
        if isinstance(deg, dict):
            dcls = measurements.__OPERATOR__.get(deg.get("name"))
            if dcls is None:
                raise NameError(f"degradation: name {deg.get('name')!r} is not defined")
            if not issubclass(dcls, GRID_OPERATORS):
                raise ValueError(f"degradation: {deg.get('name')!r} is not a linear operator with a grid of its own")
        return tuple(hw)
    if cls is None or not issubclass(cls, GRID_OPERATORS) or not operator_cfg.get("simulate", True):
        return tuple(hw)
    kw = {k: v for k, v in operator_cfg.items() if k != "name"}
    if "batch_size" not in kw:          # per-image PSFs: the batch is as large as the list says (the grid does not depend on it)
        if isinstance(kw.get("seed"), (list, tuple)):
            kw["batch_size"] = len(kw["seed"])
        elif kw.get("per_image") and isinstance(kw.get("kernel"), (list, tuple, np.ndarray, torch.Tensor)):
            kw["batch_size"] = len(kw["kernel"])
    return tuple(cls(device="cpu", **kw).out_shape(int(hw[0]), int(hw[1])))


def model_grid(model, ref_img):
    """(H, W) of the image a chain produces when `ref_img` is not on the image's grid (a measurement handed in as it is): the
    network's `image_size`."""
    n = getattr(model, "image_size", None)
    if n is None:
        raise ValueError("simulate: False needs a network that states its image_size")
    return (int(n), int(n)) if np.isscalar(n) else (int(n[0]), int(n[1]))


def measurement_mask(ref_img, mask_cfg=None, mask=None):
    """The validity mask of a chain, [B,3,H,W] fp32 on ref_img's device, or None when neither source is given.
    mask_cfg: the optional config key `measurement.mask`; `{auto_exposure: {low, high, soft, per_pixel}}` builds the mask from
    the exposure of the photo as loaded (ref_img in [-1, 1], before the noiser and `degamma_input`) with osm_exposure_mask:
    0 where a channel's value leaves (low, high), a ramp of width `soft` inside; `per_pixel: true` drops the whole pixel when
    any channel is clipped.  mask: an explicit one ([B,3,H,W], [B,1,H,W], [1,3,H,W] or [1,1,H,W] in [0, 1]); both: their product."""
    from .guided_diffusion.condition_methods import validate_measurement_mask
    out = None
    if mask is not None:
        m = validate_measurement_mask(mask, ref_img.shape[0])
        if tuple(m.shape[2:]) != tuple(ref_img.shape[2:]):
            raise ValueError(f"mask {tuple(m.shape)} does not match the image grid {tuple(ref_img.shape[2:])}")
        out = m.to(ref_img.device).expand(ref_img.shape[0], 3, *ref_img.shape[2:]).contiguous()
    if mask_cfg:
        _refuse_unknown_keys("measurement.mask", mask_cfg, ("auto_exposure",))
        ae = mask_cfg.get("auto_exposure")
        if ae:
            from . import ops
            y = ref_img.detach().to(torch.float32).contiguous()
            auto = torch.empty_like(y)
            ops.exposure_mask(y, auto, y.shape[0], y.shape[2] * y.shape[3], float(ae.get("low", 0.0)), float(ae.get("high", 1.0)),
                              float(ae.get("soft", 0.0)), bool(ae.get("per_pixel", False)))
            out = auto if out is None else out * auto
    return out


def restore_image(model, ref_img, cfg, device=None, image_idx=0, x_scale=1.0, same_seed_per_image=False, mask=None, tiling=None,
                  depth=None, depth_confidence=None, depth_geometry=None, robust=None, gain=None, **loop_kwargs):
    """One image through the reference's per-image sequence: fresh operator / noiser / conditioning method /
    sampler (:142-155), y = noiser(ref) (+ degamma), manual_seed + x_T ~ N(0, I) per global iteration
    (:191-196), guided p_sample_loop, post-processing.  Returns a list with one dict per global iteration.

    `ref_img` may carry B > 1 images: one batch of independent chains.  With `same_seed_per_image` every image of
    the batch starts from the SAME x_T and receives the SAME per-step noise -- exactly what B separate calls (each
    re-seeded with `manual_seed`, as the reference driver does per image) would draw -- so an image's result does not
    depend on how images are grouped into batches or spread over ranks.  Like the reference, only image 0 of a batch is
    post-processed (`_image_result(whole=True)`): `sample`, `pred_xstart`, `measurement` and `mask` are over the whole batch, every
    other key is image 0's.  `restore_images` builds every image's result from the same chain (`_run_chains`).

    `mask` (and / or the optional config key `measurement.mask`, see `measurement_mask`): a per-pixel validity mask of the
    measurement on the network grid (`data.transform_mask` takes one from the photo's resolution there).  The chain is guided
    through it (`p_sample_loop(measurement_mask=)`) and every result carries it as `mask` [B,3,H,W]; without either, nothing
    is passed and the results have no such key.

    `diffusion: {solver, solver_eta, timestep_spacing}` (optional config keys; `create_sampler`): a few-step solver ('ddim' |
    'dpmpp_2m') as the step rule and 'quad' / 'logsnr' index selection for `timestep_respacing: "<count>"`.  Every result then
    carries `solver` and `steps` (the indices the chain has); without a solver there are no such keys.

    `tiling` (or the optional top-level config key `tiling`; the argument wins): `{tile, stride, window}` (`parse_tiling`; unknown
    keys raise) for ONE image larger than the network's grid, e.g. the 512-class grid of `data.fit_transform(size=512)`: the
    network sees overlapping tiles of side `tile`, everything else acts on the whole image (`p_sample_loop(tiling=)`).  Every
    result then carries `tiling` = {tile, stride, window, origins int32 [n,2]}; without it nothing is passed and there is no such key.

    `depth` / `depth_confidence` (and / or the optional config key `measurement.depth: {weight, align, loss, scale, scale_min, path}`,
    see `depth_prior_inputs`): a range map on the network's grid, [B,1,H,W], [1,1,H,W] or [B,H,W] (`data.transform_range` takes one
    from the photo's resolution there), handed to the data term as a prior on the depth plane (`p_sample_loop(depth_prior=)`,
    include/osmosis_depthprior.h).  Every result then carries `depth_prior`, `depth_confidence`, `depth_scale`, `depth_shift`,
    `depth_loss_final`, `depth_metric` and, for align 'scale' / 'none', `phi_metric` (`attach_depth_prior`) -- each image's own,
    also when the batch is walked in chunks; a chain without a guided sub-step leaves the fit undefined (NaN).  Without a range
    map nothing is passed and there are no such keys.  `depth_geometry`: the photo's `data.Geometry` for the map of
    `measurement.depth.path` (`depth_prior_inputs` says what is assumed without it).

    `robust` (or the optional config key `measurement.robust: {loss, c, scale, sigma_min, per_pixel}`; the argument wins; unknown
    keys raise): the robust data term (`p_sample_loop(robust=)`, include/osmosis_robust.h).  Every result then carries
    `robust_weight` (omega [3,h,w] of the last guided sub-step) and `robust_scale` (its sigma) -- each image's own, also when the
    batch is walked in chunks; `save_outputs` writes the per-pixel minimum of omega over the channels as `<name>_robust.png`.
    Without it nothing is passed and there are no such keys.

    `gain` (or the optional config key `measurement.gain: {grid, eta, n_iter, smooth, g_min, learn, path}`; the argument wins;
    unknown keys raise): a learnt vignetting gain field in the Osmosis data term (`p_sample_loop(gain_field=)`,
    include/osmosis_gain.h); `path`: a .npy of nodes or of a full-resolution flat field (least squares to nodes, `gain_config`),
    with `learn: False` a measured flat field that stays fixed.  The field starts afresh at every global iteration.  Every result
    then carries `gain_field` [H,W], `gain_nodes` [gh,gw] and `flat_fielded` = clip((y + 1) / (2 G), 0, 1) -- each image's own,
    also in chunked batches; `save_outputs` writes `<name>_gain.png`.  Without it nothing is passed and there are no such keys.

    Operator `field_blur` (a field of PSFs on a node grid, spatially varying blur): simulated as `psf_blur` is (y = noiser(A ref);
    `simulate: False` as there), the field shared by every image of a batch; every result carries `kernel` fp32 [gh,gw,kh,kw] (the
    node kernels) and `save_outputs` writes `<name>_kernel.png`, their gh x gw mosaic over the common maximum.

    Operator `blind_blur` (the PSF is learnt during the chain): `operator.reset()` before every global iteration, every result
    carries `kernel` fp32 [k,k] (the estimate at the end of its chain; [3,k,k] with `per_channel`; `save_outputs` writes it as
    `<name>_kernel.png`, a per-channel one as one RGB picture), and `simulate: True` needs `simulate_with: {name: <a grid operator>,
    ...}` -- the blur that makes y = noiser(A* ref); it must keep the image's size.  Without `per_image` ONE PSF serves the whole
    batch (photos through one optical system); with `per_image: True` every image of the batch learns -- and its result carries --
    its own.

    Operator `blind_field_blur` (the FIELD is learnt during the chain): as `blind_blur` -- `operator.reset()` before every global
    iteration, `simulate: True` needs `simulate_with` (typically `field_blur`) -- with `field_blur`'s results: `kernel` fp32
    [gh,gw,k,k], the node kernels at the end of the chain, and their mosaic as `<name>_kernel.png`.  One field serves the whole
    batch; not tiled."""
    return [_image_result(run, 0, whole=True)
            for run in _run_chains(model, ref_img, cfg, device=device, image_idx=image_idx, x_scale=x_scale,
                                   same_seed_per_image=same_seed_per_image, mask=mask, tiling=tiling, depth=depth,
                                   depth_confidence=depth_confidence, depth_geometry=depth_geometry, robust=robust, gain=gain,
                                   **loop_kwargs)]


def _run_chains(model, ref_img, cfg, device=None, image_idx=0, x_scale=1.0, same_seed_per_image=False, mask=None, tiling=None,
                depth=None, depth_confidence=None, depth_geometry=None, robust=None, gain=None, **loop_kwargs):
    """`restore_image`'s arguments through set-up and `p_sample_loop`: one record per global iteration of what the chain left for the
    WHOLE batch, on the host -- what `_image_result` builds any image's result dict from.  Fields (None where the chain has no such
    thing): `sample`; on the Osmosis branch `variables`, `loss`, `pred_xstart`, `observed` [B,3,h,w] (`observed_image`, a
    degradation), `depth` {z, m [B,1,HW], scale, shift, loss [B], align}, `gain` {nodes, field} and `tiling`; `mask` [B,3,h,w];
    `robust` {weight [B,3,h,w], scale [B]}; `kernel` [nb,nc,k,k] (`operator.kernels()`); `solver` / `steps`; `measurement` (y_n);
    `ref_img` and `operator_cfg` for `postprocess`."""
    tiling = tiling if tiling is not None else cfg.get("tiling")
    tiling_info = None
    if tiling is not None:
        th, tw, sy, sx, window = parse_tiling(tiling)
        tiling_info = {"tile": (th, tw), "stride": (sy, sx), "window": window,
                       "origins": tile_grid(ref_img.shape[-2], ref_img.shape[-1], (th, tw), (sy, sx), window)[0]}
        loop_kwargs = dict(loop_kwargs, tiling={"tile": (th, tw), "stride": (sy, sx), "window": window})
    device = device if device is not None else ref_img.device
    measure, cond_cfg = cfg["measurement"], cfg["conditioning"]
    op_cfg = dict(measure["operator"])
    op_cfg["batch_size"] = ref_img.shape[0]
    operator = get_operator(device=device, **op_cfg)
    degraded = getattr(operator, "degradation", None) is not None       # `measurement.operator.degradation: {name: ..., ...}`
    if degraded and tiling is not None:
        raise NotImplementedError("tiling: a degradation inside the physical operator is not tiled")
    noiser = get_noise(**measure["noise"])
    cond = get_conditioning_method(cond_cfg["method"], operator, noiser, **cond_cfg["params"],
                                   **cfg["sample_pattern"], **cfg["aux_loss"])
    sampler = create_sampler(**cfg["diffusion"])
    ref_img = ref_img.to(device)
    pretrain = cfg["unet_model"]["pretrain_model"]
    shape = list(ref_img.shape)
    y_clean = ref_img
    is_blind = op_cfg.get("name") in ("blind_blur", "blind_field_blur")
    blind_name = op_cfg.get("name")
    if blind_name == "blind_field_blur" and tiling is not None:
        raise NotImplementedError("blind_field_blur: tiling is not supported (the learnt field spans one frame; the 'ps' branch is not tiled)")
    is_field = isinstance(operator, PSFFieldOperator)       # a field of PSFs: every result carries the node kernels
    if isinstance(operator, GRID_OPERATORS):
        # a blur / super-resolution operator: the measurement is simulated from the clean image, y = noiser(A ref), as the DPS driver
        # does; `measurement.operator.simulate: False` takes ref_img as the measurement itself, on the operator's own grid
        if op_cfg.get("simulate", True) and is_blind:
            # the PSF is what the chain looks for, so the operator cannot simulate its own measurement: another grid operator stands
            # for the unknown optics, y = noiser(A* ref)
            sim_cfg = op_cfg.get("simulate_with")
            if not isinstance(sim_cfg, dict) or sim_cfg.get("name") is None:
                raise ValueError(f"{blind_name}: " "`simulate: True` needs `simulate_with: {name: <a grid operator>, ...}` (the blur that produces "
                                 "the measurement); `simulate: False` takes the photo as it is")
            sim_cfg = dict(sim_cfg)
            sim_cfg["batch_size"] = ref_img.shape[0]
            truth = get_operator(device=device, **sim_cfg)
            if not isinstance(truth, GRID_OPERATORS):
                raise ValueError(f"{blind_name}: simulate_with {sim_cfg['name']!r} is not a linear operator with a grid of its own")
            if tuple(truth.out_shape(*ref_img.shape[-2:])) != tuple(ref_img.shape[-2:]):
                raise ValueError(f"{blind_name}: simulate_with {sim_cfg['name']!r} changes the image's size {tuple(ref_img.shape[-2:])} -> "
                                 f"{tuple(truth.out_shape(*ref_img.shape[-2:]))}; a PSF keeps it")
            y_clean = truth.forward(ref_img[:, 0:3].to(torch.float32).contiguous())
        elif op_cfg.get("simulate", True):
            y_clean = operator.forward(ref_img[:, 0:3].to(torch.float32).contiguous())
        else:
            grid = model_grid(model, ref_img)
            if tuple(ref_img.shape[-2:]) != tuple(operator.out_shape(*grid)):
                raise ValueError(f"simulate: False takes the measurement itself: expected {tuple(operator.out_shape(*grid))} (the "
                                 f"operator's grid for a {grid[0]} x {grid[1]} image), got {tuple(ref_img.shape[-2:])}")
            shape[2:] = grid
        y_n = noiser(y_clean)
    else:
        if degraded:
            # the photo IS the measurement (it is never simulated here): it lives on the degradation's grid for the network's image
            grid = model_grid(model, ref_img)
            if tuple(ref_img.shape[-2:]) != tuple(operator.out_shape(*grid)):
                raise ValueError(f"degradation: the photo is the measurement itself: expected {tuple(operator.out_shape(*grid))} (the "
                                 f"degradation's grid for a {grid[0]} x {grid[1]} image), got {tuple(ref_img.shape[-2:])}")
            shape[2:] = grid
        y_n = noiser(ref_img)
    if cfg.get("degamma_input", False):
        y_n = degamma(y_n)
    m_dev = measurement_mask(y_clean, measure.get("mask"), mask)
    if m_dev is not None:
        loop_kwargs = dict(loop_kwargs, measurement_mask=m_dev)
    shape[1] = 4 if pretrain == "osmosis" else shape[1]
    prior = depth_prior_inputs(shape[2:], measure.get("depth"), depth, depth_confidence, depth_geometry)
    if prior is not None:
        loop_kwargs = dict(loop_kwargs, depth_prior=prior)
    robust = robust_config(measure.get("robust"), robust)
    if robust is not None:
        loop_kwargs = dict(loop_kwargs, robust=robust)
    gain = gain_config(measure.get("gain"), gain, shape[2:])
    if gain is not None:
        loop_kwargs = dict(loop_kwargs, gain_field=gain)
    for global_ii in range(global_iterations(cfg["sample_pattern"])):
        torch.manual_seed(cfg.get("manual_seed", 0))
        if is_blind:
            operator.reset()        # every global iteration learns the PSF from its initial weights
        if same_seed_per_image and shape[0] > 1:
            x_start = torch.randn([1] + shape[1:], device=device).repeat(shape[0], 1, 1, 1)
            loop_kwargs = dict(loop_kwargs, shared_noise=True)
        else:
            x_start = torch.randn(shape, device=device)
        if x_scale != 1.0:          # sub-chains started at a low timestep (tools/full_chain.py --last)
            x_start = x_start * x_scale
        rgb_guidance = cfg.get("rgb_guidance", False)
        ret = sampler.p_sample_loop(
            model=model, x_start=x_start, measurement=y_n, measurement_cond_fn=cond.conditioning,
            record=cfg.get("record_process", False) and loop_kwargs.get("save_grids_path") is not None, save_root=None,
            pretrain_model=pretrain, image_idx=image_idx, record_every=cfg.get("record_every", 150),
            rgb_guidance=rgb_guidance, sample_pattern=cfg["sample_pattern"], global_iteration=global_ii, **loop_kwargs)
        solver = getattr(sampler, "solver", None)
        run = SimpleNamespace(
            ref_img=ref_img, operator_cfg=measure["operator"], measurement=y_n.detach().cpu(), variables=None, loss=None,
            pred_xstart=None, observed=None, depth=None, gain=None, tiling=None, robust=None,
            mask=None if m_dev is None else m_dev.detach().cpu(),
            kernel=_operator_kernels(operator) if is_blind or is_field else None,      # [nb,nc,k,k]; a field: [gh,gw,kh,kw]
            kernel_field=is_field,
            solver=solver, steps=None if solver is None else sampler.num_timesteps)
        vals = None if robust is None else cond.robust_values()     # (None: no guided sub-step on a loop that never opened the state)
        if vals is not None:
            run.robust = dict(weight=vals["weight"].detach().cpu().view(y_n.shape[0], 3, *y_n.shape[2:]), scale=vals["scale"].detach().cpu())
        if rgb_guidance or pretrain != "osmosis":
            # the rgb-guidance / non-osmosis chain returns the sample only (gaussian_diffusion.py:340); the
            # reference driver splits it into RGB and depth (osmosis_sampling.py:366-380): no phi, no recomposition
            run.sample = ret.detach().cpu()
            yield run
            continue
        sample, variables, loss, run.pred_xstart = ret
        run.sample, run.variables = sample.detach().cpu(), {k: v.detach().cpu() for k, v in variables.items()}
        run.loss, run.tiling = None if loss is None else np.asarray(loss), tiling_info
        if degraded:
            run.observed = observed_image(operator, run.pred_xstart).cpu()
        if prior is not None:       # every image's fit and loss from the chain's last guided sub-step (NaN: there was none)
            zr, mr = (t.detach().cpu() for t in cond.depth_prior_rows(shape[0], shape[2], shape[3], device))
            run.depth = dict({k: v.detach().cpu() for k, v in cond.depth_prior_values().items()}, z=zr, m=mr, align=cond._depth["align"])
        if gain is not None:
            run.gain = {k: v.detach().cpu() for k, v in cond.gain_values().items()}
        yield run


def _operator_kernels(operator):
    """fp32 [nb,nc,k,k]: every PSF of a `blind_blur` operator at the end of its chain (`kernels()`; an operator that only knows
    `kernel2d()` has the one)."""
    ks = operator.kernels() if hasattr(operator, "kernels") else np.asarray(operator.kernel2d())[None, None]
    return torch.from_numpy(np.ascontiguousarray(ks)).to(torch.float32)


def _image_result(run, b, whole=False):
    """Image b's result dict from a chain's record (`_run_chains`): the one place where the end of a chain becomes a result.
    whole (`restore_image`'s contract, b = 0): post-processing sees the batch as the reference's driver does and keeps image 0's
    outputs, `sample` / `pred_xstart` / `measurement` / `mask` stay over the whole batch, and the result names the chain's `solver` /
    `steps`.  Otherwise (`restore_images` with a batch) all of them are image b's rows [1,...], and there is no `solver` / `steps`."""
    rows = slice(None) if whole else slice(b, b + 1)
    if run.variables is None:
        post = rgb_guidance_result(run.sample[rows], run.measurement[rows])
    else:
        post = postprocess(run.pred_xstart[rows], {k: v[rows] for k, v in run.variables.items()}, run.ref_img[rows], run.operator_cfg,
                           run.loss if whole or run.loss is None else run.loss[rows], observed=None if run.observed is None else run.observed[b])
        post.update(sample=run.sample[rows], pred_xstart=run.pred_xstart[rows], measurement=run.measurement[rows])
        if run.depth is not None:
            d = run.depth
            attach_depth_prior(post, d["z"][b], d["m"][b], d["scale"][b], d["shift"][b], d["loss"][b], d["align"])
        if run.gain is not None:
            attach_gain(post, run.gain["nodes"][b], run.gain["field"][b], run.measurement[b])
        if run.tiling is not None:
            post["tiling"] = run.tiling
    if run.mask is not None:
        post["mask"] = run.mask[rows]
    if run.robust is not None:
        attach_robust(post, run.robust["weight"][b], run.robust["scale"][b])
    if run.kernel is not None and getattr(run, "kernel_field", False):     # `field_blur`: the whole field [gh,gw,kh,kw], shared by the batch
        post["kernel"] = run.kernel
    elif run.kernel is not None:        # image b's own PSF ([nb,nc,k,k]: one row for the batch, or one per image): [k,k], or [3,k,k] per channel
        kb = run.kernel[b if run.kernel.shape[0] > 1 else 0]
        post["kernel"] = kb[0] if kb.shape[0] == 1 else kb
    if whole and run.solver is not None:
        post.update(solver=run.solver, steps=run.steps)
    return post


def _rows_of_batch(items, idxs, blank, channels, what):
    """The walk `batch_depth` and `batch_mask` share: the [1,C,H,W] entries of a list aligned with the images as the float32 rows of the
    batch `idxs`, `blank(i)` for an image without one; None when the list is, or none of the batch's images has one."""
    if items is None or all(items[i] is None for i in idxs):
        return None
    rows = []
    for i in idxs:
        t = blank(i) if items[i] is None else torch.as_tensor(items[i]).to(torch.float32)
        if t.dim() != 4 or t.shape[0] != 1 or t.shape[1] not in channels:
            raise ValueError(f"{what}[{i}] must be {' or '.join(f'[1,{c},H,W]' for c in channels)}, got {tuple(t.shape)}")
        rows.append(t)
    return rows


def _cat_rows(rows):
    return torch.cat([r.to(rows[0].device) for r in rows], 0)


def batch_depth(depths, depth_confidences, idxs):
    """(depth, confidence) rows [n,1,H,W] of one batch from `depths` / `depth_confidences` as `restore_image`'s keyword arguments, or
    {} when none of its images has a map; an image without one gets z = 0 (no valid range: confidence 0)."""
    zs = _rows_of_batch(depths, idxs, lambda i: torch.zeros(1, 1, *next(d for d in (depths[j] for j in idxs) if d is not None).shape[-2:]),
                     (1,), "depths")
    if zs is None:
        return {}
    ms = []
    for i, z in zip(idxs, zs):
        c = None if depth_confidences is None else depth_confidences[i]
        ms.append((torch.isfinite(z) & (z > 0)).to(torch.float32) if c is None else torch.as_tensor(c).to(torch.float32).reshape(z.shape))
    return dict(depth=_cat_rows(zs), depth_confidence=_cat_rows(ms))


def batch_mask(masks, images, cfg, idxs):
    """`masks` (a list aligned with `images`: [1,1,H,W] / [1,3,H,W] each, or None for an image without one) of one batch [n,3,h,w], or
    None when none of its images has one; an image without one gets ones on the measurement's grid (the mask lives there)."""
    rows = _rows_of_batch(masks, idxs, lambda i: torch.ones(1, 3, *measurement_grid(cfg["measurement"]["operator"], images[i].shape[-2:])), (1, 3), "masks")
    return None if rows is None else _cat_rows([m.expand(1, 3, *m.shape[2:]) for m in rows])


def postprocess_each(out_xstart, variable_dict, ref_img, operator_cfg, loss=None, observed=None):
    """`postprocess` for every image of a batch (the reference only ever has one).  observed: [B,3,h,w] (`observed_image`) for a
    chain whose physical operator carries a degradation -- required then, as the photo lives on the degradation's grid."""
    if operator_cfg.get("degradation") is not None and observed is None:
        raise ValueError("postprocess_each: a physical operator with a degradation needs `observed` [B,3,h,w] (observed_image)")
    if observed is not None and observed.shape[0] != out_xstart.shape[0]:
        raise ValueError(f"observed must have one row per image: {tuple(observed.shape)} for {out_xstart.shape[0]} images")
    outs = []
    for b in range(out_xstart.shape[0]):
        vd = {k: v[b:b + 1] for k, v in variable_dict.items()}
        outs.append(postprocess(out_xstart[b:b + 1], vd, ref_img[b:b + 1], operator_cfg,
                                None if loss is None else np.asarray(loss)[b:b + 1],
                                observed=None if observed is None else observed[b]))
    return outs


def batch_operator_config(cfg, idxs, n_images):
    """`cfg` for the batch of images `idxs` out of `n_images`: what the operator config gives PER IMAGE of the whole list -- a list
    under `seed` (`motion_blur`, also inside `simulate_with`) or a `psf_blur` `kernel` with `per_image` (also inside `simulate_with`)
    -- is sliced to the batch's entries, as masks and depths are, on a COPY of the config; `cfg` itself when there is nothing to
    slice.  ValueError when such a list does not have one entry per image."""
    op = cfg.get("measurement", {}).get("operator")
    if not isinstance(op, dict):
        return cfg

    def sliced(c, where):
        out = None
        if isinstance(c.get("seed"), (list, tuple)):
            if len(c["seed"]) != n_images:
                raise ValueError(f"{where}seed: a list has one entry per image: {len(c['seed'])} seeds for {n_images} images")
            out = dict(c, seed=[c["seed"][i] for i in idxs])
        if c.get("per_image") and c.get("name") == "psf_blur" and c.get("kernel") is not None:
            k = c["kernel"]
            if isinstance(k, (str, bytes)) or hasattr(k, "__fspath__"):
                k = np.load(k, allow_pickle=False)
            k = k.detach().cpu().numpy() if isinstance(k, torch.Tensor) else np.asarray(k, dtype=np.float64)
            if k.ndim < 3 or k.shape[0] != n_images:
                raise ValueError(f"{where}kernel: per_image takes one kernel per image: shape {k.shape} for {n_images} images")
            out = dict(out if out is not None else c, kernel=k[list(idxs)])
        return out

    new_op = sliced(op, "measurement.operator.")
    sim = op.get("simulate_with")
    new_sim = sliced(sim, "measurement.operator.simulate_with.") if isinstance(sim, dict) else None
    if new_op is None and new_sim is None:
        return cfg
    new_op = dict(new_op if new_op is not None else op)
    if new_sim is not None:
        new_op["simulate_with"] = new_sim
    return dict(cfg, measurement=dict(cfg["measurement"], operator=new_op))


def restore_images(model, images, cfg, rank=0, world=1, device=None, gt_rgb=None, batch_size=1, originals=None,
                   geometries=None, full_res_upsample="bilinear", masks=None, tiling=None, shared_water=False, depths=None,
                   depth_confidences=None, robust=None, gain=None, **loop_kwargs):
    """images[rank::world] (no collective on the path).  Returns {image index: result dict of the
    last global iteration}; when `gt_rgb` (list of [3,H,W] in [0,1]) is given each result carries `psnr`.

    `batch_size` > 1 carries that many of this rank's images per pass (BASELINE config 4: 8 images per GPU): they
    are independent chains with per-image phi, per-image reductions and -- like the reference's per-image
    `manual_seed` -- the same x_T / noise stream each, so image i's result is the one a batch-1 run gives.

    `originals` (list of `to_tensor` photos [3,H0,W0]) with `geometries` (their `data.Geometry`) attaches
    `reconstruct_full_resolution(..., upsample=full_res_upsample)` to every result that carries phi, under `full_res`.

    `tiling` goes to `restore_image` as it is (one canvas per call: `batch_size` stays 1 with it).

    `shared_water=True`: the photos were taken in ONE water body (a burst, a clip, a survey transect), so every batch this call
    forms (`batch_size` images of this rank) is one water group -- `phi_groups="all"` on a copy of the operator config of that
    batch: one phi estimated from all its images (`_PhysicalOperator(phi_groups=)`; `measurement.operator.phi_reduce` chooses
    "mean" or "sum").  A batch of one stays ungrouped.  Every result carries `water_group`, the image indices that shared its phi;
    everything downstream reads the per-image phi rows as before.  Not with `tiling`, nor with a `ps` / rgb-guidance config (no
    phi there).

    `depths` / `depth_confidences` (lists aligned with `images`: a range map [1,1,H,W] on the network's grid each, or None for an
    image without one): rows per image, chunked with the images (`restore_image(depth=, depth_confidence=)`); in a batch, an image
    without a map gets confidence 0 everywhere -- no prior for it.  The fit stays per image, also with `shared_water`.

    `robust` / `gain` are `restore_image`'s (they win over `measurement.robust` / `measurement.gain`); every result carries its own
    `robust_weight` / `robust_scale` and `gain_field` / `gain_nodes` / `flat_fielded`, also in chunked batches.

    Per-image point-spread functions: a LIST under `seed` (`motion_blur`, also inside `blind_blur`'s `simulate_with`) or a `psf_blur`
    `kernel` with `per_image: True` has one entry per image of `images`; every batch gets its slice on a copy of the config
    (`batch_operator_config`), as `masks` / `depths` are sliced.  With `blind_blur: {per_image: True}` every image of a batch learns
    its own PSF and its result carries it as `kernel`.

    Every batch is one chain (`_run_chains`, which takes `restore_image`'s other keyword arguments as they are), and every image's
    result is built from what it left (`_image_result`): a batch of one gives `restore_image`'s result, a larger one every image's
    own rows [1,...] of `sample` / `pred_xstart` / `measurement` / `mask` and of every option's values -- without the chain's
    `solver` / `steps`, which only a single image's result names."""
    if robust is not None:
        loop_kwargs = dict(loop_kwargs, robust=robust)
    if gain is not None:
        loop_kwargs = dict(loop_kwargs, gain=gain)
    if shared_water:
        if tiling is not None or cfg.get("tiling") is not None:
            raise NotImplementedError("shared_water: tiling is one canvas per call, water parameters are not shared across canvases")
        if cfg.get("rgb_guidance", False) or cfg.get("conditioning", {}).get("method") == "ps":
            raise ValueError("shared_water: the rgb-guidance ('ps') chain has no water parameters to share")
    if tiling is not None:
        loop_kwargs = dict(loop_kwargs, tiling=tiling)
    if (originals is None) != (geometries is None):
        raise ValueError("originals and geometries go together")
    if originals is not None and cfg.get("measurement", {}).get("operator", {}).get("degradation") is not None:
        raise NotImplementedError("full-resolution reconstruction with a degradation inside the physical operator is not implemented")
    if masks is not None and len(masks) != len(images):
        raise ValueError(f"masks must align with images: {len(masks)} masks for {len(images)} images")

    for what, lst in (("depths", depths), ("depth_confidences", depth_confidences)):
        if lst is not None and len(lst) != len(images):
            raise ValueError(f"{what} must align with images: {len(lst)} for {len(images)} images")
    if depth_confidences is not None and depths is None:
        raise ValueError("depth_confidences come with depths")

    out = {}
    mine = shard_indices(len(images), rank, world)
    for k in range(0, len(mine), max(1, batch_size)):
        idxs = mine[k:k + max(1, batch_size)]
        bcfg = batch_operator_config(cfg, idxs, len(images))     # per-image seeds / kernels: this batch's slice, on a copy
        if shared_water and len(idxs) > 1:      # this batch is one water group (a copy: the caller's config stays as it is)
            bcfg = dict(bcfg, measurement=dict(bcfg["measurement"], operator=dict(bcfg["measurement"]["operator"], phi_groups="all")))
        *_, run = _run_chains(model, torch.cat([images[i] for i in idxs], 0), bcfg, device=device, image_idx=idxs[0],
                              same_seed_per_image=len(idxs) > 1, mask=batch_mask(masks, images, bcfg, idxs),
                              **batch_depth(depths, depth_confidences, idxs), **loop_kwargs)
        # one image: `restore_image`'s result; a batch: every image's own rows (`blind_blur`: ONE PSF for the batch, or with
        # `per_image` every image's own)
        res = [_image_result(run, b, whole=len(idxs) == 1) for b in range(len(idxs))]
        for i, r in zip(idxs, res):
            if shared_water:
                r["water_group"] = list(idxs)
            if gt_rgb is not None:
                r["psnr"] = float(utilso.psnr(r["rgb_01_clip"], gt_rgb[i]))
            if originals is not None and "phi" in r:
                r["full_res"] = reconstruct_full_resolution(r, originals[i], geometries[i], cfg["measurement"]["operator"],
                                                            upsample=full_res_upsample, device=device)
            out[i] = r
    return out
