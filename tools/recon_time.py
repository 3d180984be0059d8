#!/usr/bin/env python
"""Timing of the full-resolution path (DESIGN section 4 row `recon_kernel`, README "State").

    python tools/recon_time.py                 everything below, one JSON line at the end
    python tools/recon_time.py --no-step       the operator only

1. `osm_recon_fullres` on a 6000 x 4000 planar image (network grid 256 x 384), bilinear and joint bilateral (R = 2), all three
   outputs: ONE child run of this script (`--child`) under `timeout ... rocprofv3 --kernel-trace --stats -d DIR -- python ...`;
   the kernel's average End - Start per mode from the kernel trace, next to its floor = bytes moved / the float4-copy rate
   (12 B read + 12 B written per pixel, + 3 B for the 8-bit image + 4 B for the depth map; 4.8 TB/s).
2. The same formula (bilinear) in torch on the host with 16 threads.
3. One guided step of the full-size network at 256 x 352 against 256 x 256, from this process (HIP events around the fused
   loop's steps, the mean of the timed steps after a warm-up).
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H0, W0, NH, NW = 4000, 6000, 256, 384
COPY_RATE = 4.8e12
BYTES_PER_PIXEL = 12 + 12 + 3 + 4
REPS = 10


def inputs(device):
    import torch
    g = torch.Generator().manual_seed(0)
    depth = (torch.rand(NH, NW, generator=g) * 1.8 - 0.9).to(device)
    guide = torch.rand(3, NH, NW, generator=g).to(device)
    image = torch.rand(3, H0, W0, generator=g).to(device)
    phi = [torch.tensor(v).to(device) for v in ([1.1, 0.95, 0.95], [0.95, 0.8, 0.8], [0.14, 0.29, 0.49])]
    ay, ax = NH / H0, NW / W0
    return depth, guide, image, phi, (ay, 0.5 * ay - 0.5, ax, 0.5 * ax - 0.5)


def child():
    """what the profiler watches: REPS launches per mode after one warm-up each"""
    import torch
    from osmosis_diffusion_code_amd import ops
    depth, guide, image, phi, amap = inputs("cuda:0")
    rgb = torch.empty(3, H0, W0, device="cuda:0")
    u8 = torch.empty(H0, W0, 3, device="cuda:0", dtype=torch.uint8)
    full = torch.empty(H0, W0, device="cuda:0")
    for mode in (0, 1):
        for _ in range(REPS + 1):
            ops.recon_fullres(depth, guide, image, *phi, 1, [1.4, 1.4, 1.0], amap, rgb, u8, full, mode, 2, 1.0, 0.1)
    torch.cuda.synchronize()


def kernel_trace(limit):
    if shutil.which("rocprofv3") is None:
        return {"error": "rocprofv3 not on PATH"}
    d = tempfile.mkdtemp(prefix="osm_recon_")
    cmd = ["timeout", "-k", "10", str(limit), "rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "--",
           sys.executable, os.path.abspath(__file__), "--child"]
    try:
        rc = subprocess.run(cmd, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)
        if rc.returncode != 0:
            return {"error": f"profiled child exited with {rc.returncode}: {rc.stderr[-300:]}"}
        durs = {0: [], 1: []}
        for f in glob.glob(d + "/**/*kernel_trace.csv", recursive=True):
            for r in csv.DictReader(open(f)):
                for mode in (0, 1):
                    if f"recon_kernel<{mode}>" in r["Kernel_Name"]:
                        durs[mode].append(float(r["End_Timestamp"]) - float(r["Start_Timestamp"]))
        out = {}
        for mode, name in ((0, "bilinear"), (1, "joint_bilateral")):
            v = sorted(durs[mode])[:-1] if len(durs[mode]) > 1 else durs[mode]      # drop the slowest (the warm-up launch)
            if not v:
                return {"error": f"no kernel-trace rows for recon_kernel<{mode}>"}
            out[name] = {"avg_us": round(sum(v) / len(v) / 1e3, 1), "min_us": round(v[0] / 1e3, 1), "dispatches": len(v)}
        return out
    finally:
        shutil.rmtree(d, ignore_errors=True)


def host_formula():
    """bilinear upsampling + the closed form in torch on the host, 16 threads: best of 3"""
    import torch
    import torch.nn.functional as F
    torch.set_num_threads(16)
    depth, guide, image, phi, amap = inputs("cpu")
    pa, pb, pinf = (p.view(3, 1, 1) for p in phi)
    best = None
    for _ in range(3):
        t0 = time.perf_counter()
        d = F.interpolate(depth[None, None], size=(H0, W0), mode="bilinear", align_corners=False)[0]
        D = (d + 1.4) * 1.4
        rgb = torch.exp(pa * D) * (image - pinf * (1 - torch.exp(-pb * D)))
        u8 = (rgb.clamp(0, 1) * 255).to(torch.uint8).permute(1, 2, 0).contiguous()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    del u8
    return {"ms": round(best * 1e3, 1), "threads": 16}


def step_times(steps, warmup):
    """ms per guided step of the full-size network, B = 1, at 256 x 256 and 256 x 352, in this process"""
    import contextlib
    import io

    import torch

    import baseline_configs as BC
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    from osmosis_diffusion_code_amd.guided_diffusion import unet
    dev = "cuda:0"
    cfg = BC.SAMPLE
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**BC.UNET)
    model.reset_parameters(1234)
    model = model.to(dev).eval()
    out = {}
    for H, W in ((256, 256), (256, 352)):
        g = torch.Generator().manual_seed(1)
        x = (0.1 * torch.randn(1, 4, H, W, generator=g)).to(dev)
        y = (torch.rand(1, 3, H, W, generator=g) * 1.6 - 0.8).to(dev)
        opc = dict(cfg["measurement"]["operator"])
        name = opc.pop("name")

        def run(n):
            op = M.get_operator(name, device=dev, batch_size=1, **opc)
            cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **cfg["conditioning"]["params"],
                                              **cfg["sample_pattern"], **cfg["aux_loss"])
            sampler = gd.create_sampler(**cfg["diffusion"])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            sampler.p_sample_loop(model=model, x_start=x, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                  save_root=None, pretrain_model="osmosis", rgb_guidance=False,
                                  sample_pattern=cfg["sample_pattern"], index_range=(n - 1, 0))
            torch.cuda.synchronize()
            return time.perf_counter() - t0
        run(warmup)                              # builds the engine and its graphs for this shape
        t_short, t_long = run(warmup), run(warmup + steps)
        out[f"{H}x{W}"] = round((t_long - t_short) / steps * 1e3, 3)      # the setup of a loop cancels
    out["ratio"] = round(out["256x352"] / out["256x256"], 3)
    out["pixel_ratio"] = 1.375
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", action="store_true")
    ap.add_argument("--no-step", action="store_true")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--profile-timeout", type=int, default=240)
    a = ap.parse_args()
    if a.child:
        return child()
    px = H0 * W0
    res = {"image": f"{W0}x{H0}", "network_grid": f"{NH}x{NW}", "floor_us": round(px * BYTES_PER_PIXEL / COPY_RATE * 1e6, 1),
           "bytes_per_pixel": BYTES_PER_PIXEL, "kernel_trace": kernel_trace(a.profile_timeout), "host_torch": host_formula()}
    if not a.no_step:
        res["guided_step_ms"] = step_times(a.steps, a.warmup)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
