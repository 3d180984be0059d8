#!/usr/bin/env python3
"""What a per-pixel validity mask in the data term costs a full-size Osmosis chain: wall time per step of the headline
configuration (the 4 -> 8 bench network, 552.8 M parameters, seeded weights, 256 x 256, B = 1, `underwater_physical_revised`,
n_iter = 20, the conv arithmetic of --conv-mode) on the fused loop, three chains in ONE run on one box:

    unmasked          no mask (osm_phys_optimize)
    ones              a mask of ones (osm_phys_optimize_m: the masked kernels, the unmasked values)
    half              a random mask with about half of its pixels at zero

    python tools/mask_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3] [--repeats 1] [--unmasked-only]

Each chain is respaced to `--window` steps and timed whole, after a `--warmup`-step chain per variant that builds the engine,
records its plans and captures the graphs; `--repeats` > 1 reports the fastest.  `--unmasked-only` times the first chain alone
(a tree without the feature: the same-box comparison against the parent commit).  Prints one JSON line.  Seeded synthetic
weights do not denoise: timing is value independent (`finite` in the output line).
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
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--repeats", type=int, default=1)
    ap.add_argument("--unmasked-only", action="store_true")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**bench.UNET_KW)
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    x_T, y = bench.synthetic_inputs(0, 1, 256)
    x_T, y = x_T.to(dev), y.to(dev)
    g = torch.Generator().manual_seed(7)
    masks = {"unmasked": None}
    if not a.unmasked_only:
        masks["ones"] = torch.ones(1, 3, 256, 256)
        masks["half"] = torch.rand(1, 3, 256, 256, generator=g) * (torch.rand(1, 1, 256, 256, generator=g) > 0.5).float()

    def chain(steps, mask):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, timestep_respacing=str(steps)))
        op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, **bench.OPERATOR)
        cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, bench.PATTERN, tuple(x_T.shape)) is cond
        kw = {} if mask is None else {"measurement_mask": mask}
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                    save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=bench.PATTERN,
                                    noise_seed=1, **kw)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out[0]

    res = {}
    for name, mask in masks.items():
        chain(a.warmup, mask)
        dt, img = min((chain(a.window, mask) for _ in range(max(1, a.repeats))), key=lambda r: r[0])
        res[name] = {"seconds": round(dt, 3), "ms_per_step": round(1e3 * dt / a.window, 3), "finite": bool(torch.isfinite(img).all())}
    base = res["unmasked"]["ms_per_step"]
    for name in res:
        if name != "unmasked":
            res[name]["vs_unmasked_percent"] = round(100.0 * (res[name]["ms_per_step"] / base - 1.0), 2)
    print(json.dumps({"net": "4 -> 8", "loop": "fused", "steps": a.window, "conv_mode": model.conv_mode, "chains": res}))


if __name__ == "__main__":
    main()
