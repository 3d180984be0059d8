#!/usr/bin/env python3
"""Wall time per step of full-size Osmosis chains (the headline configuration: `osmosis` conditioning with
underwater_physical_revised, n_iter = 20, the 4 -> 8 network of bench.py with seeded weights, 256 x 256, B = 1) with a linear
operator between the image-formation model and the photo (`measurement.operator.degradation`).  ONE process times these chains,
alternated `--rounds` times after one warm-up chain each, in bench.py's window (every step inside the phi-update regime: started at
t = 0.3 T from 0.5 x_T, 20 phi iterations per step, so the plain chain is bench.py's workload and the values stay finite):

    plain (no degradation)     gaussian_blur (61, 3.0)     motion_blur (default)     super_resolution x 4 bicubic (y 64 x 64)

The composed phi loop is six launches per inner iteration (forward, A, resid, A^T, reduce_lin, finalize_lin) against the plain
loop's two; the plain chain of the same run is the yardstick.  Timing is device-synchronised wall time around p_sample_loop.
Prints one JSON line.

    python tools/physlin_chain_time.py [--window 200] [--warmup 8] [--rounds 2] [--conv-mode f16x3]
    python tools/physlin_chain_time.py --kernels-only      # a few guided steps of each composed chain, for a kernel trace

Seeded synthetic weights do not denoise: compare the chains of one run only (`finite` in the output line, per chain).
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
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402

CHAINS = (("plain", None),
          ("gaussian_blur_61", dict(name="gaussian_blur", kernel_size=61, intensity=3.0)),
          ("motion_blur_61", dict(name="motion_blur")),
          ("sr4_bicubic", dict(name="super_resolution", scale_factor=4, method="bicubic")))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed steps per chain")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps per chain that build the plans")
    ap.add_argument("--rounds", type=int, default=2, help="timed chains per variant, the variants alternated")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--kernels-only", action="store_true", help="only a --warmup-long chain of each composed variant (for a kernel trace)")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**bench.UNET_KW)
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (4, 8)
    x_T, ref = bench.synthetic_inputs(0, 1, 256)
    x_T, ref = x_T.to(dev), ref.to(dev)

    T = 1000
    first = int(0.3 * T) - 1                                      # bench.py's window: the phi-update regime, started at t = 0.3 T
    x_s = 0.5 * x_T                                               # from a bounded x_t, so that seeded weights keep the values finite

    def chain(deg, y, steps):
        """`steps` guided steps as windows (first .. 0) restarted from the same bounded x_t, as bench.py's run(): (seconds, finite)."""
        op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, degradation=deg, **bench.OPERATOR)
        cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
        sampler = gd.create_sampler(**bench.DIFFUSION)
        assert sampler.num_timesteps == T
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, bench.PATTERN, tuple(x_T.shape)) is cond
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        left, finite = steps, True
        while left > 0:
            n = min(left, first + 1)
            out = sampler.p_sample_loop(model=model, x_start=x_s, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                        save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=bench.PATTERN,
                                        index_range=(first, first - n + 1), reference_rng_order=False)
            left -= n
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        finite = bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all()) and bool(np.isfinite(np.asarray(out[2])).all())
        return dt, finite

    ys = {}
    for name, deg in CHAINS:                                      # the measurement of each variant, simulated once from the same photo
        ys[name] = ref if deg is None else M.build_degradation(deg, dev).forward(ref).detach()
    out = {"net": "4 -> 8", "steps": a.window, "rounds": a.rounds, "conv_mode": model.conv_mode, "window": f"idx {first} down, x_t = 0.5 x_T",
           "ms_per_step": {}, "finite": {name: True for name, _ in CHAINS}}
    if a.kernels_only:
        for name, deg in CHAINS[1:]:
            chain(deg, ys[name], a.warmup)
        print(json.dumps({"kernels_only": True, "steps": a.warmup}))
        return
    for name, deg in CHAINS:
        chain(deg, ys[name], a.warmup)
    times = {name: [] for name, _ in CHAINS}
    for _ in range(a.rounds):
        for name, deg in CHAINS:
            dt, finite = chain(deg, ys[name], a.window)
            times[name].append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = out["finite"][name] and finite
    out["ms_per_step"] = times
    print(json.dumps(out))


if __name__ == "__main__":
    main()
