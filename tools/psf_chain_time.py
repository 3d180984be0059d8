#!/usr/bin/env python3
"""Wall time per step of full-size rgb-guidance chains (DDPM.p_sample + `ps`, clip_denoised, gaussian noiser with sigma 0) through
the motion-blur measurement operator, on the 3 -> 6 network (the bench architecture, 552.8 M parameters, seeded weights),
256 x 256, B = 1.  ONE process times, in this order, after a warm-up chain each:

    fused motion_blur (61, 0.5, seed 0)      fused identity `ps`      motion_blur on `_generic_loop`

The expectation: the fused operator chain lands within two launches' cost of the identity chain (two osm_psf_apply launches per
step more) and under `_generic_loop` (OSM_FUSED_RGB=0: autograd over the HIP UNet operator and osmosis::psf_apply).

It then times osm_psf_apply alone, forward and adjoint, at 3 x 256^2 for the default trajectory and for a dense 61 x 61 PSF: device
events around `--reps` back-to-back launches after a warm-up (`psf_us`).  `--kernels-only` runs just those launches, for a kernel
trace taken in a run of its own:

    python tools/psf_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3] [--reps 50]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/psf_chain_time.py --kernels-only

Prints one JSON line.  Seeded synthetic weights do not denoise: compare the chains of one run only (`finite` in the output line).
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (configuration constants of the benchmark)
from osmosis_diffusion_code_amd import ops  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402

MOTION = dict(kernel_size=61, intensity=0.5, seed=0)
CHAINS = (("motion_fused", "motion_blur", MOTION, True),
          ("identity_fused", "rgb_guidance", {}, True),
          ("motion_generic", "motion_blur", MOTION, False))


def kernel_times(dev, reps):
    """{name: microseconds per launch} of osm_psf_apply at B = 1, 3 planes of 256 x 256 read from / written to [1,4,HW]."""
    H = W = 256
    dense = np.random.default_rng(0).standard_normal((61, 61))
    psfs = (("motion61", M.get_operator("motion_blur", device=dev, **MOTION)),
            ("dense61", M.get_operator("psf_blur", device=dev, kernel=dense)))
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 4, H, W, generator=g).to(dev)
    r = torch.randn(1, 3, H, W, generator=g).to(dev)
    Ax, gx = torch.empty(1, 3, H, W, device=dev), torch.empty(1, 4, H, W, device=dev)
    out = {}
    for name, op in psfs:
        taps, (Ry, Rx) = op.taps(dev), op.radius()
        out[name + ".taps"] = int(taps[2].numel())
        for tag, launch in (("fwd", lambda: ops.psf_apply(x, Ax, *taps, Ry, Rx, 1, 3, 4 * H * W, 3 * H * W, H, W)),
                            ("adj", lambda: ops.psf_apply(r, gx, *taps, Ry, Rx, 1, 3, 3 * H * W, 4 * H * W, H, W, adjoint=True, zero_planes=1))):
            for _ in range(3):
                launch()
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(reps):
                launch()
            e1.record()
            torch.cuda.synchronize()
            out[f"{name}.{tag}"] = round(1e3 * e0.elapsed_time(e1) / reps, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed osm_psf_apply window")
    ap.add_argument("--kernels-only", action="store_true", help="only the osm_psf_apply launches (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.kernels_only:
        print(json.dumps({"psf_us": kernel_times(dev, a.reps)}))
        return
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
        y = op.forward(ref).detach() if isinstance(op, M.GRID_OPERATORS) else ref           # the measurement, simulated
        chain(cond, y, a.warmup, fused)
        dt, img = chain(cond, y, a.window, fused)
        out["ms_per_step"][name] = round(1e3 * dt / a.window, 3)
        out["finite"] = out["finite"] and bool(torch.isfinite(img).all())
    os.environ.pop("OSM_FUSED_RGB", None)
    out["psf_us"] = kernel_times(dev, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
