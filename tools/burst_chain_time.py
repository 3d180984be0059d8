#!/usr/bin/env python3
"""Wall time per step of full-size Osmosis chains on a burst of B = 4 photos (the headline configuration: `osmosis` conditioning
with underwater_physical_revised, n_iter = 20, the 4 -> 8 network of bench.py with seeded weights, 256 x 256) with and without
shared water parameters (`measurement.operator.phi_groups`).  ONE process times these chains, alternated `--rounds` times after one
warm-up chain each, in bench.py's window (every step inside the phi-update regime: started at t = 0.3 T from 0.5 x_T, 20 phi
iterations per step, the chain shape of tools/physlin_chain_time.py):

    per_image        every image its own phi (the code path and launch sequence of an ungrouped batch)
    one_group        phi_groups = "all": one phi for the four images, one engine pass
    one_group_2+2    the same group with the batch forced to walk as chunks of [2, 2]: every chunk's forward, one data term over the
                     batch, every chunk's forward AGAIN before its backward -- the re-forward cost
    per_image_2+2    the ungrouped batch walked as [2, 2] (no re-forward): what one_group_2+2 is compared with

The grouped phi loop has the launches of the per-image one (the grouped finalize in the place of the plain one), so one_group is
expected within the box-to-box spread of per_image.  Timing is device-synchronised wall time around p_sample_loop.  Prints one
JSON line.

    python tools/burst_chain_time.py [--batch 4] [--window 200] [--warmup 8] [--rounds 2] [--conv-mode f16x3]

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

# (name, phi_groups, forced chunk walk as fractions of the batch or None)
CHAINS = (("per_image", None, None), ("one_group", "all", None), ("one_group_2+2", "all", 2), ("per_image_2+2", None, 2))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--window", type=int, default=200, help="timed steps per chain")
    ap.add_argument("--warmup", type=int, default=8, help="untimed steps per chain that build the plans")
    ap.add_argument("--rounds", type=int, default=2, help="timed chains per variant, the variants alternated")
    ap.add_argument("--conv-mode", default="f16x3")
    a = ap.parse_args()
    B = a.batch
    assert B >= 2 and B % 2 == 0, "--batch must be even (the forced walk is two equal chunks)"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**bench.UNET_KW)
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (4, 8)
    x_T, ref = bench.synthetic_inputs(0, B, 256)
    x_T, ref = x_T.to(dev), ref.to(dev)

    T = 1000
    first = int(0.3 * T) - 1                                      # bench.py's window: the phi-update regime, started at t = 0.3 T
    x_s = 0.5 * x_T                                               # from a bounded x_t, so that seeded weights keep the values finite
    plain_chunks = gd.GaussianDiffusion.__dict__["chunk_sizes"]       # (the staticmethod object, to put back as it was)

    def chain(groups, halves, steps):
        """`steps` guided steps as windows (first .. 0) restarted from the same bounded x_t, as bench.py's run(): (seconds, finite)."""
        kw = {} if groups is None else {"phi_groups": groups}
        op = M.get_operator("underwater_physical_revised", device=dev, batch_size=B, **bench.OPERATOR, **kw)
        cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
        sampler = gd.create_sampler(**bench.DIFFUSION)
        assert sampler.num_timesteps == T
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, bench.PATTERN, tuple(x_T.shape)) is cond
        gd.GaussianDiffusion.chunk_sizes = plain_chunks if halves is None else staticmethod(lambda n, cap: [n // halves] * halves)
        try:
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            left = steps
            while left > 0:
                n = min(left, first + 1)
                out = sampler.p_sample_loop(model=model, x_start=x_s, measurement=ref, measurement_cond_fn=cond.conditioning, record=False,
                                            save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=bench.PATTERN,
                                            index_range=(first, first - n + 1), reference_rng_order=False)
                left -= n
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
        finally:
            gd.GaussianDiffusion.chunk_sizes = plain_chunks
        finite = bool(torch.isfinite(out[0]).all()) and bool(torch.isfinite(out[3]).all()) and bool(np.isfinite(np.asarray(out[2])).all())
        if groups is not None:                                    # one water body: every row carries the same phi
            finite = finite and all(bool((v == v[0:1]).all()) for v in out[1].values())
        return dt, finite

    out = {"net": "4 -> 8", "batch": B, "steps": a.window, "rounds": a.rounds, "conv_mode": model.conv_mode,
           "window": f"idx {first} down, x_t = 0.5 x_T", "one_pass_chunks": gd.GaussianDiffusion.chunk_sizes(B, model.images_in_flight(B, 256, 256)),
           "ms_per_step": {}, "finite": {name: True for name, _, _ in CHAINS}}
    for name, groups, halves in CHAINS:
        chain(groups, halves, a.warmup)
    times = {name: [] for name, _, _ in CHAINS}
    for _ in range(a.rounds):
        for name, groups, halves in CHAINS:
            dt, finite = chain(groups, halves, a.window)
            times[name].append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = out["finite"][name] and finite
    out["ms_per_step"] = times
    print(json.dumps(out))


if __name__ == "__main__":
    main()
