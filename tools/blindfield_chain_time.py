#!/usr/bin/env python3
"""What LEARNING a field of point-spread functions costs (include/osmosis_blindfield.h), in ONE process, device-synchronised.

Kernel level (`launch_us`, microseconds per launch; device events around `--reps` back-to-back launches after a warm-up), B = 1,
3 planes of 256 x 256, a dense k = 31 support (961 taps) under 5 x 5 nodes:
    field_tap_grad     osm_field_tap_grad, one launch
    single_tap_grad    ONE osm_psf_tap_grad over the same image and tap list
    composed           the baseline a user could build from the single-PSF kernel: 25 torch products hat_n r plus 25 osm_psf_tap_grad
                       launches
    field_tap_step     osm_field_tap_step (the kernel and the copy of the workspace over w)
alternated in this order, `field_tap_grad` timed again at the end.

Chain level (`ms_per_step`): full-size `ps` chains (DDPM.p_sample, clip_denoised, gaussian noiser with sigma 0) on the 3 -> 6 network
(the bench architecture, seeded weights), 256 x 256, B = 1, f16x3: `blind_field_blur` (k = 31, 5 x 5, n_iter 1) next to `field_blur`
with a dense radial_defocus field of the same size, alternated `--rounds` times after a warm-up chain each, `--window` timed steps.

    python tools/blindfield_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3] [--reps 50] [--rounds 2] [--kernels-only]

Prints one JSON line.  Seeded synthetic weights do not denoise and their chains can go non-finite: `finite` says
whether the image did.  Compare the numbers of one run only.
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
from osmosis_diffusion_code_amd import ops  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402

K = 31
GRID = [5, 5]


def _timed(launch, reps):
    for _ in range(3):
        launch()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        launch()
    e1.record()
    torch.cuda.synchronize()
    return round(1e3 * e0.elapsed_time(e1) / reps, 2)


def launch_times(dev, reps):
    H = W = 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, H, W, generator=g).to(dev)
    r = torch.randn(1, 3, H, W, generator=g).to(dev)
    op = M.get_operator("blind_field_blur", device=dev, kernel_size=K, grid=GRID)
    dy, dx, w = op.taps(dev)
    gh, gw = op.grid
    T = int(dy.numel())
    tabs = op.field_tables(H, W, dev)
    Ry, Rx = op.radius()
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, 3, dev)
    part = torch.empty(NP * T, device=dev)
    plain = torch.empty(ops.tap_grad_nparts(3, H, W) * T, device=dev)
    iy0, fy, ix0, fx = tabs
    j = torch.arange(gh, device=dev)[:, None]
    hy = torch.where(iy0[None] == j, 1.0 - fy[None], torch.where(iy0[None] == j - 1, fy[None], torch.zeros((), device=dev)))
    j = torch.arange(gw, device=dev)[:, None]
    hx = torch.where(ix0[None] == j, 1.0 - fx[None], torch.where(ix0[None] == j - 1, fx[None], torch.zeros((), device=dev)))
    hat = (hy[:, None, :, None] * hx[None, :, None, :]).contiguous()                      # [gh,gw,H,W]
    loss = torch.ones(1, device=dev)
    w_new = torch.empty_like(w)

    def field():
        ops.field_tap_grad(x, r, dy, dx, tabs, lay, NP, gh, gw, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, part)

    def single():
        ops.psf_tap_grad(x, r, dy, dx, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, plain)

    def composed():
        for a in range(gh):
            for b in range(gw):
                ops.psf_tap_grad(x, (hat[a, b] * r).contiguous(), dy, dx, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, plain)

    def step():
        ops.field_tap_step(w, w_new, part, loss, lay, NP, 1, 3 * H * W, 0.1, 0.0, 1e-4)
    out = {"taps": T, "partials_per_image": NP, "tiles_x_planes": ops.tap_grad_nparts(3, H, W)}
    out["field_tap_grad"] = _timed(field, reps)
    out["single_tap_grad"] = _timed(single, reps)
    out["composed"] = _timed(composed, max(1, reps // 5))
    out["field_tap_step"] = _timed(step, reps)
    out["field_tap_grad_again"] = _timed(field, reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed kernel window")
    ap.add_argument("--rounds", type=int, default=2, help="how often the chains alternate")
    ap.add_argument("--kernels-only", action="store_true", help="only the kernel-level launches")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.kernels_only:
        print(json.dumps({"launch_us": launch_times(dev, a.reps)}))
        return
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**dict(bench.UNET_KW, pretrain_model="imagenet"))
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (3, 6)
    x_T, ref = bench.synthetic_inputs(0, 1, 256)
    x_T, ref = x_T[:, :3].contiguous().to(dev), ref.to(dev)
    fixed = M.get_operator("field_blur", device=dev, model="radial_defocus", kernel_size=K, grid=GRID)
    blind = M.get_operator("blind_field_blur", device=dev, kernel_size=K, grid=GRID)
    y = fixed.forward(ref).detach()
    conds = {name: CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0), scale="3")
             for name, op in (("field_blur", fixed), ("blind_field_blur", blind))}

    def chain(c, steps):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, clip_denoised=True, timestep_respacing=str(steps)))
        assert sampler._fast_path_ok(model, c.conditioning, "imagenet", True, bench.PATTERN, tuple(x_T.shape)) is c
        if hasattr(c.operator, "reset"):
            c.operator.reset()
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=c.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=bench.PATTERN)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, img

    out = {"net": "3 -> 6", "steps": a.window, "conv_mode": model.conv_mode, "batch": 1, "kernel_size": K, "grid": GRID,
           "ms_per_step": {}, "finite": {}}
    for c in conds.values():
        chain(c, a.warmup)
    for _ in range(a.rounds):
        for name, c in conds.items():
            dt, img = chain(c, a.window)
            out["ms_per_step"].setdefault(name, []).append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = bool(torch.isfinite(img).all())
    out["launch_us"] = launch_times(dev, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
