#!/usr/bin/env python
"""Timing of tiled sampling (README "State", DESIGN section 4 rows `tile_gather_kernel` / `tile_blend_kernel`).

    python tools/tiled_chain_time.py                 everything below, one JSON line at the end
    python tools/tiled_chain_time.py --no-profile    the step times only

Full-size network (the 4 -> 8 bench network, seeded weights, `--conv-mode` f16x3), `underwater_physical_revised`, n_iter = 20:
1. ms per guided step of ONE 512 x 768 canvas as 3 x 5 = 15 tiles of 256 x 256 at stride 128 (hann window), next to the measured
   B = 1 256 x 256 step of the same process (`--steps` timed steps after a warm-up chain that builds engines, plans and graphs;
   the setup of a loop cancels in the difference of two chain lengths).
2. The share of the four tile passes per step (osm_tile_gather x 2, osm_tile_blend x 2) in the kernel time of a tiled chain:
   ONE child run of this script (`--child`) under `timeout ... rocprofv3 --kernel-trace --stats -d DIR -- python ...`, summed
   over the dispatches between the first and the last tile kernel.
Expectation before any hardware run: the four passes move under 100 MB per step (15 tiles x (4 + 8 + 8 + 4) channels x 256 x 256
x 4 B = 94 MB on the tile side) against 15 network passes -- well under 1 % of the step.  (README "State" records the measured run.)
"""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CANVAS, TILE, STRIDE, WINDOW = (512, 768), 256, 128, "hann"


def setup(conv_mode):
    import torch

    import bench
    from osmosis_diffusion_code_amd.guided_diffusion import unet
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**bench.UNET_KW)
    bench.seeded_weights(model)
    model = model.to("cuda:0").eval()
    model.conv_mode = conv_mode
    return torch, bench, model


def chain_seconds(torch, bench, model, hw, tiling, n):
    """wall time of the last n indices of the benchmark's chain on an hw image (tiling None: the untiled fused loop)"""
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    dev = "cuda:0"
    g = torch.Generator().manual_seed(1)
    x = (0.1 * torch.randn(1, 4, *hw, generator=g)).to(dev)
    y = (torch.rand(1, 3, *hw, generator=g) * 1.6 - 0.8).to(dev)
    sampler = gd.create_sampler(**bench.DIFFUSION)
    op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, **bench.OPERATOR)
    cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **bench.PATTERN, aux_loss=bench.AUX)
    kw = {} if tiling is None else {"tiling": tiling}
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=bench.PATTERN,
                                noise_seed=1, index_range=(n - 1, 0), **kw)
    torch.cuda.synchronize()
    return time.perf_counter() - t0, bool(torch.isfinite(out[0]).all())


def step_times(conv_mode, steps, warmup):
    torch, bench, model = setup(conv_mode)
    tiling = dict(tile=TILE, stride=STRIDE, window=WINDOW)
    out = {}
    for name, hw, t in (("untiled_256x256", (256, 256), None), (f"tiled_{CANVAS[0]}x{CANVAS[1]}", CANVAS, tiling)):
        chain_seconds(torch, bench, model, hw, t, warmup)
        t_short, _ = chain_seconds(torch, bench, model, hw, t, warmup)
        t_long, finite = chain_seconds(torch, bench, model, hw, t, warmup + steps)
        out[name] = {"ms_per_step": round((t_long - t_short) / steps * 1e3, 3), "finite": finite}
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    n = gd.tile_grid(*CANVAS, TILE, STRIDE, WINDOW)[0].shape[0]
    out["tiles"] = n
    out["chunks"] = gd.GaussianDiffusion.chunk_sizes(n, model.images_in_flight(n, TILE, TILE))
    out["tiled_over_tiles_x_untiled"] = round(out[f"tiled_{CANVAS[0]}x{CANVAS[1]}"]["ms_per_step"] /
                                              (n * out["untiled_256x256"]["ms_per_step"]), 3)
    return out


def child(conv_mode, steps, warmup):
    """what the profiler watches: one tiled chain of warmup + steps indices"""
    torch, bench, model = setup(conv_mode)
    chain_seconds(torch, bench, model, CANVAS, dict(tile=TILE, stride=STRIDE, window=WINDOW), warmup + steps)


def kernel_trace(conv_mode, steps, warmup, limit):
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not on PATH"}
    d = tempfile.mkdtemp(prefix="osm_tiled_")
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child", "--conv-mode", conv_mode, "--steps", str(steps), "--warmup", str(warmup)]
    try:
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if rc.returncode != 0:
            return {"error": f"profiled child exited with {rc.returncode}: {rc.stderr[-300:]}"}
        rows = []
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                rows.append((float(r["Start_Timestamp"]), float(r["End_Timestamp"]), r["Kernel_Name"]))
        tile = [r for r in rows if "tile_gather_kernel" in r[2] or "tile_blend_kernel" in r[2]]
        if not tile:
            return {"error": "no kernel-trace rows for tile_gather_kernel / tile_blend_kernel"}
        lo, hi = min(r[0] for r in tile), max(r[1] for r in tile)
        inside = [r for r in rows if r[0] >= lo and r[1] <= hi]
        t_tile, t_all = sum(r[1] - r[0] for r in tile), sum(r[1] - r[0] for r in inside)
        per = {}
        for name in ("tile_gather_kernel", "tile_blend_kernel"):
            v = [r[1] - r[0] for r in tile if name in r[2]]
            per[name] = {"dispatches": len(v), "avg_us": round(sum(v) / len(v) / 1e3, 2)}
        return {"tile_kernels_ms": round(t_tile / 1e6, 3), "all_kernels_ms": round(t_all / 1e6, 3),
                "share_percent": round(100.0 * t_tile / t_all, 3), "indices": warmup + steps, **per}
    finally:
        shutil.rmtree(d, ignore_errors=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-steps", type=int, default=5)
    ap.add_argument("--profile-timeout", type=int, default=300)
    a = ap.parse_args()
    if a.child:
        return child(a.conv_mode, a.steps, a.warmup)
    res = {"canvas": f"{CANVAS[0]}x{CANVAS[1]}", "tile": TILE, "stride": STRIDE, "window": WINDOW, "conv_mode": a.conv_mode,
           "steps": a.steps, "step_ms": step_times(a.conv_mode, a.steps, a.warmup)}
    if not a.no_profile:
        res["kernel_trace"] = kernel_trace(a.conv_mode, a.profile_steps, a.warmup, a.profile_timeout)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
