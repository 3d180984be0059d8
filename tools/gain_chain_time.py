#!/usr/bin/env python3
"""What a learnt vignetting gain field costs a full-size Osmosis chain: wall time per step of the headline configuration (`osmosis`
conditioning with underwater_physical_revised, n_iter = 20, the 4 -> 8 network of bench.py with seeded weights, 256 x 256, B = 1, the
conv arithmetic of --conv-mode) on the fused loop.  ONE process times two chains, alternated `--rounds` times after one warm-up
chain each, in bench.py's window (every step inside the phi-update regime: started at t = 0.3 T from 0.5 x_T, 20 phi iterations per
step, the chain shape of tools/depth_chain_time.py):

    no_gain          the chain as it always was (the unmasked route)
    gain_5x5         `gain_field=dict(grid=(5, 5))`: osm_phys_forward + the three launches of osm_gain_prepare per guided sub-step,
                     then the masked route on (y', M G)

and the three kernels alone by device events over `--launches` back-to-back calls at 256 x 256 (osm_gain_rows, osm_gain_step,
osm_gain_expand, and the one C call that enqueues all three).

Expectation, stated before anything was measured (no bar is fixed): one osm_phys_forward (about 5 us in the committed trace) plus
three launch-floor launches (about 10 us each), the masked route in the unmasked one's place (measured free) -- under 0.3 % of the
18.4 ms step.  Timing of the chains is device-synchronised wall time around p_sample_loop.  Prints one JSON line.

    python tools/gain_chain_time.py [--window 200] [--warmup 8] [--rounds 2] [--launches 50] [--conv-mode f16x3]

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

CHAINS = ("no_gain", "gain_5x5")
EXPECTATION = ("one osm_phys_forward (~5 us) plus three launch-floor launches (~10 us each), the masked route in the unmasked one's "
               "place (measured free): under 0.3 % of the 18.4 ms step")


def launch_times(dev, n):
    """us per launch of the term's kernels at 256 x 256, B = 1, 5 x 5 nodes: device events around n back-to-back calls, after one
    untimed call."""
    H = W = 256
    g = torch.Generator().manual_seed(3)
    F = torch.rand(1, 4, H * W, generator=g).to(dev)
    y = (2 * torch.rand(1, 3, H * W, generator=g) - 1).to(dev)
    M0 = torch.ones(1, 3, H * W, device=dev)
    nodes = torch.ones(1, 5, 5, device=dev)
    ye, me = (torch.empty(1, 3, H * W, device=dev) for _ in range(2))
    field = torch.empty(1, 1, H * W, device=dev)
    desc = ops.gain_desc((5, 5), 0.01, 1, 0.0, 0.05, True, 0, 4, 1, H, W)
    tabs = ops.gain_tables(H, W, 5, 5, dev)
    t, s, cs = ops.gain_workspace(desc, dev)
    calls = {"osm_gain_rows": lambda: ops.gain_rows(desc, tabs, nodes, F, y, M0, t, s),
             "osm_gain_step": lambda: ops.gain_step(desc, tabs, t, s, nodes, cs),
             "osm_gain_expand": lambda: ops.gain_expand(desc, tabs, nodes, y, M0, ye, me, field),
             "osm_gain_prepare": lambda: ops.gain_prepare(desc, tabs, F, y, M0, nodes, t, s, cs, ye, me, field)}
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

    def chain(name, steps):
        """`steps` guided steps as windows (first .. 0) restarted from the same bounded x_t, as bench.py's run(): (seconds, finite)."""
        op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, **bench.OPERATOR)
        cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
        sampler = gd.create_sampler(**bench.DIFFUSION)
        assert sampler.num_timesteps == T
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, bench.PATTERN, tuple(x_T.shape)) is cond
        kw = {}
        if name == "gain_5x5":
            kw["gain_field"] = dict(grid=(5, 5))
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
        vals = cond.gain_values()
        if name == "gain_5x5":
            finite = finite and vals is not None and bool(torch.isfinite(vals["nodes"]).all()) and bool(torch.isfinite(vals["field"]).all())
        else:
            finite = finite and vals is None
        return dt, finite, None if vals is None else (float(vals["nodes"].min()), float(vals["nodes"].max()))
    out = {"net": "4 -> 8", "batch": 1, "steps": a.window, "rounds": a.rounds, "conv_mode": model.conv_mode,
           "window": f"idx {first} down, x_t = 0.5 x_T", "expectation": EXPECTATION, "ms_per_step": {},
           "finite": {name: True for name in CHAINS}}
    for name in CHAINS:
        chain(name, a.warmup)
    times = {name: [] for name in CHAINS}
    for _ in range(a.rounds):
        for name in CHAINS:
            dt, finite, vals = chain(name, a.window)
            times[name].append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = out["finite"][name] and finite
            if vals is not None:
                out["min_and_max_node_at_the_end"] = [round(v, 5) for v in vals]
    out["ms_per_step"] = times
    out["gain_vs_none_percent"] = round(100.0 * (min(times["gain_5x5"]) / min(times["no_gain"]) - 1.0), 2)
    out["us_per_launch_256x256"] = launch_times(dev, a.launches)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
