#!/usr/bin/env python3
"""Wall time per step of a full-size rgb-guidance chain (DDPM.p_sample + `ps`, clip_denoised, gaussian noiser with sigma 0: the
shipped configs/rgb_guidance_sample_config.yaml) on the 3 -> 6 network (pretrain_model "imagenet": the torso of the bench network
with a 3-channel stem and a 6-channel head), fused and -- with --generic -- on `_generic_loop` (OSM_FUSED_RGB=0: autograd over the
HIP UNet operator); --net rgbd times the same chain on the 4 -> 8 bench network for a same-box comparison (its fused loop only).
Bench architecture (552.8 M parameters, seeded weights), 256 x 256, B = 1.  Prints one JSON line.

    python tools/rgb_chain_time.py [--net rgb|rgbd] [--window 200] [--warmup 8] [--generic] [--mean-only]

The chain is respaced to `--window` steps and timed whole (`_generic_loop` has no index range), after a `--warmup`-step chain that
builds the engine, records its plans and captures the graphs.  Seeded synthetic weights do not denoise: compare loops and networks
on the same setting only (`finite` in the output line).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (configuration constants of the benchmark)
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--net", choices=("rgb", "rgbd"), default="rgb")
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--generic", action="store_true", help="OSM_FUSED_RGB=0: time `_generic_loop` (3-channel network only)")
    ap.add_argument("--mean-only", action="store_true", help="rgb_guidance=False: the mean-only branch (3-channel network only)")
    a = ap.parse_args()
    rgb = a.net == "rgb"
    assert rgb or not (a.generic or a.mean_only), "--generic / --mean-only go with --net rgb"
    if a.generic:
        os.environ["OSM_FUSED_RGB"] = "0"
    dev = torch.device("cuda", 0)
    pretrain = "imagenet" if rgb else "osmosis"
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**dict(bench.UNET_KW, pretrain_model=pretrain))
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    C = model.in_channels
    assert (C, model.out_channels) == ((3, 6) if rgb else (4, 8))
    x_T, y = bench.synthetic_inputs(0, 1, 256)
    x_T, y = x_T[:, :C].contiguous().to(dev), y.to(dev)
    op = M.get_operator("rgb_guidance", device=dev, batch_size=1)
    cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0), scale="3" if rgb else "3,3,3,0.1")

    def chain(steps):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, clip_denoised=True, timestep_respacing=str(steps)))
        fused = sampler._fast_path_ok(model, cond.conditioning, pretrain, not a.mean_only, bench.PATTERN, tuple(x_T.shape)) is not None
        assert fused != a.generic, "the chain did not take the requested loop"
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                    save_root=None, pretrain_model=pretrain, rgb_guidance=not a.mean_only,
                                    sample_pattern=bench.PATTERN)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, img

    chain(a.warmup)
    dt, img = chain(a.window)
    print(json.dumps({"net": f"{C} -> {model.out_channels}", "loop": "generic" if a.generic else "fused",
                      "branch": "mean-only" if a.mean_only else "rgb-guidance", "steps": a.window, "seconds": round(dt, 3),
                      "ms_per_step": round(1e3 * dt / a.window, 3), "conv_mode": model.conv_mode,
                      "finite": bool(torch.isfinite(img).all())}))


if __name__ == "__main__":
    main()
