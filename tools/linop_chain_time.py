#!/usr/bin/env python3
"""Wall time per step of full-size rgb-guidance chains (DDPM.p_sample + `ps`, clip_denoised, gaussian noiser with sigma 0) through
the blur and super-resolution measurement operators, on the 3 -> 6 network (the bench architecture, 552.8 M parameters, seeded
weights), 256 x 256, B = 1.  ONE process times, in this order, after a warm-up chain each:

    fused gaussian_blur (61, 3.0)      fused super_resolution x 4 (bicubic)      fused identity `ps`      gaussian_blur on `_generic_loop`

The expectation: the fused operator chains land within a few launches' cost of the identity chain (two osm_linop_apply launches
per step more) and clearly under `_generic_loop` (OSM_FUSED_RGB=0: autograd over the HIP UNet operator and osmosis::linop_apply).
Prints one JSON line.

    python tools/linop_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3]

Seeded synthetic weights do not denoise: compare the chains of one run only (`finite` in the output line).
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

CHAINS = (("blur_fused", "gaussian_blur", dict(kernel_size=61, intensity=3.0), True),
          ("sr4_fused", "super_resolution", dict(scale_factor=4), True),
          ("identity_fused", "rgb_guidance", {}, True),
          ("blur_generic", "gaussian_blur", dict(kernel_size=61, intensity=3.0), False))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--conv-mode", default="f16x3")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**dict(bench.UNET_KW, pretrain_model="imagenet"))
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (3, 6)
    x_T, ref = bench.synthetic_inputs(0, 1, 256)
    x_T, ref = x_T[:, :3].contiguous().to(dev), ref.to(dev)

    def chain(cond, y, steps, fused):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, clip_denoised=True, timestep_respacing=str(steps)))
        took = sampler._fast_path_ok(model, cond.conditioning, "imagenet", True, bench.PATTERN, tuple(x_T.shape)) is not None
        assert took == fused, "the chain did not take the requested loop"
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=bench.PATTERN)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, img

    out = {"net": "3 -> 6", "steps": a.window, "conv_mode": model.conv_mode, "ms_per_step": {}, "finite": True}
    for name, opname, okw, fused in CHAINS:
        os.environ["OSM_FUSED_RGB"] = "1" if fused else "0"
        op = M.get_operator(opname, device=dev, batch_size=1, **okw)
        cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0), scale="3")
        y = op.forward(ref).detach() if isinstance(op, M.SeparableOperator) else ref          # the measurement, simulated
        chain(cond, y, a.warmup, fused)
        dt, img = chain(cond, y, a.window, fused)
        out["ms_per_step"][name] = round(1e3 * dt / a.window, 3)
        out["finite"] = out["finite"] and bool(torch.isfinite(img).all())
    os.environ.pop("OSM_FUSED_RGB", None)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
