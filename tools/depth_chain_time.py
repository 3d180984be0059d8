#!/usr/bin/env python3
"""What a range-map depth prior in the data term costs a full-size Osmosis chain: wall time per step of the headline configuration
(`osmosis` conditioning with underwater_physical_revised, n_iter = 20, the 4 -> 8 network of bench.py with seeded weights,
256 x 256, B = 1, the conv arithmetic of --conv-mode) on the fused loop, with and without a dense prior.  ONE process times the two
chains, alternated `--rounds` times after one warm-up chain each, in bench.py's window (every step inside the phi-update regime:
started at t = 0.3 T from 0.5 x_T, 20 phi iterations per step, the chain shape of tools/burst_chain_time.py):

    no_prior         no range map (the launch sequence of the chain as it always was)
    dense_prior      a range map with every pixel valid, align = affine, loss = norm: three more launches per guided sub-step
                     (osm_depth_loss_grad, after the 42 of the phi loop)

and the three launches alone by device events over `--launches` back-to-back calls at 256 x 256 (osm_depth_reduce, osm_depth_fit,
osm_depth_grad, and the one C call that enqueues all three).  The prior's kernels read at most three planes of the image (0.8 MB):
they are expected at the launch floor, three launches of about 10 us under 0.5 % of an 18.4 ms step.  Timing of the chains is
device-synchronised wall time around p_sample_loop.  Prints one JSON line.

    python tools/depth_chain_time.py [--window 200] [--warmup 8] [--rounds 2] [--launches 50] [--conv-mode f16x3]

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
from osmosis_diffusion_code_amd import ops  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402

CHAINS = ("no_prior", "dense_prior")


def launch_times(dev, n):
    """us per launch of the prior's kernels at 256 x 256, B = 1: device events around n back-to-back calls, after one untimed call."""
    H = W = 256
    g = torch.Generator().manual_seed(3)
    x0 = (0.6 * torch.randn(1, 4, H, W, generator=g)).clamp(-1, 1).to(dev)
    z = (torch.rand(1, 1, H * W, generator=g) * 4 + 0.5).to(dev)
    m = torch.ones(1, 1, H * W, device=dev)
    gbuf = torch.zeros(1, 4, H, W, device=dev)
    desc = ops.depth_desc("affine", "norm", 1.0, 1.0, 1e-3, 1, (1.4, 1.4, 1.0), 1, H * W)
    part = torch.empty(ops.depth_nblk(H * W) * 8, device=dev, dtype=torch.float64)
    fit, loss = torch.zeros(1, 4, device=dev, dtype=torch.float64), torch.zeros(1, device=dev)
    calls = {"osm_depth_reduce": lambda: ops.depth_reduce(desc, x0, z, m, part), "osm_depth_fit": lambda: ops.depth_fit(desc, part, fit, loss),
             "osm_depth_grad": lambda: ops.depth_grad(desc, x0, z, m, fit, gbuf),
             "osm_depth_loss_grad": lambda: ops.depth_loss_grad(desc, x0, z, m, part, fit, loss, gbuf)}
    out = {}
    for name, fn in calls.items():
        fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out[name] = round(1e3 * e0.elapsed_time(e1) / n, 2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed steps per chain")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps per chain that build the plans")
    ap.add_argument("--rounds", type=int, default=2, help="timed chains per variant, the variants alternated")
    ap.add_argument("--launches", type=int, default=50, help="back-to-back launches per kernel timing")
    ap.add_argument("--conv-mode", default="f16x3")
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
    yy, xx = torch.meshgrid(torch.linspace(0, 1, 256), torch.linspace(0, 1, 256), indexing="ij")
    z = (1.0 + 3.0 * yy + 0.5 * xx)[None, None]                   # a dense range map: every pixel valid

    def chain(name, steps):
        """`steps` guided steps as windows (first .. 0) restarted from the same bounded x_t, as bench.py's run(): (seconds, finite)."""
        op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, **bench.OPERATOR)
        cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
        sampler = gd.create_sampler(**bench.DIFFUSION)
        assert sampler.num_timesteps == T
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, bench.PATTERN, tuple(x_T.shape)) is cond
        kw = {} if name == "no_prior" else {"depth_prior": dict(z=z, weight=1.0, align="affine", loss="norm")}
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        left = steps
        while left > 0:
            n = min(left, first + 1)
            out = sampler.p_sample_loop(model=model, x_start=x_s, measurement=ref, measurement_cond_fn=cond.conditioning, record=False,
                                        save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=bench.PATTERN,
                                        index_range=(first, first - n + 1), reference_rng_order=False, **kw)
            left -= n
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        finite = bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all()) and bool(np.isfinite(np.asarray(out[2])).all())
        vals = cond.depth_prior_values()
        if name == "dense_prior":
            finite = finite and vals is not None and all(bool(torch.isfinite(v).all()) for v in vals.values())
        else:
            finite = finite and vals is None
        return dt, finite
    out = {"net": "4 -> 8", "batch": 1, "steps": a.window, "rounds": a.rounds, "conv_mode": model.conv_mode,
           "window": f"idx {first} down, x_t = 0.5 x_T", "ms_per_step": {}, "finite": {name: True for name in CHAINS}}
    for name in CHAINS:
        chain(name, a.warmup)
    times = {name: [] for name in CHAINS}
    for _ in range(a.rounds):
        for name in CHAINS:
            dt, finite = chain(name, a.window)
            times[name].append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = out["finite"][name] and finite
    out["ms_per_step"] = times
    out["prior_vs_none_percent"] = round(100.0 * (min(times["dense_prior"]) / min(times["no_prior"]) - 1.0), 2)
    out["us_per_launch_256x256"] = launch_times(dev, a.launches)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
