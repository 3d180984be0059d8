#!/usr/bin/env python3
"""What a FIELD of point-spread functions costs (include/osmosis_psffield.h), in ONE process, device-synchronised.

Kernel level (`apply_us`, microseconds per launch; device events around `--reps` back-to-back launches after a warm-up), B = 1,
3 planes of 256 x 256, forward and adjoint, for a 5 x 5 `roll_shake` field (k = 31, 6 degrees: sparse streaks) and a dense 5 x 5
`radial_defocus` field (k = 31):
    field          osm_psf_field_apply, one launch
    single         osm_psf_apply with the centre node's weights over the same tap list
    composed       the baseline a user could build from the single-PSF kernel: 25 osm_psf_apply launches plus the torch combine
                   (forward: the hat-weighted sum of the 25 outputs; adjoint: 25 hat products, 25 launches, the running sum)
alternated in this order, `field` timed again at the end.

Chain level (`ms_per_step`): full-size `ps` chains (DDPM.p_sample, clip_denoised, gaussian noiser with sigma 0) on the 3 -> 6 network
(the bench architecture, seeded weights), 256 x 256, B = 1, f16x3: `field_blur` (roll_shake, k = 31, 5 x 5) next to `psf_blur` with
the field's corner node, alternated `--rounds` times after a warm-up chain each, `--window` timed steps.

    python tools/psffield_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3] [--reps 50] [--rounds 2] [--kernels-only]

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
FIELDS = {"roll_shake": dict(model="roll_shake", kernel_size=K, angle_deg=6.0, grid=[5, 5], image_size=[256, 256]),
          "radial_defocus": dict(model="radial_defocus", kernel_size=K, grid=[5, 5])}


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


def apply_times(dev, reps):
    H = W = 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, H, W, generator=g).to(dev)
    o = torch.empty(1, 3, H, W, device=dev)
    out = {}
    for tag, kw in FIELDS.items():
        op = M.get_operator("field_blur", device=dev, **kw)
        dy, dx, w = op.taps(dev)
        gh, gw = op.grid
        tabs = op.field_tables(H, W, dev)
        Ry, Rx = op.radius()
        iy0, fy, ix0, fx = tabs
        j = torch.arange(gh, device=dev)[:, None]
        hy = torch.where(iy0[None] == j, 1.0 - fy[None], torch.where(iy0[None] == j - 1, fy[None], torch.zeros((), device=dev)))
        j = torch.arange(gw, device=dev)[:, None]
        hx = torch.where(ix0[None] == j, 1.0 - fx[None], torch.where(ix0[None] == j - 1, fx[None], torch.zeros((), device=dev)))
        hat = (hy[:, None, :, None] * hx[None, :, None, :]).contiguous()                      # [gh,gw,H,W]
        wn = [[w[a, b].contiguous() for b in range(gw)] for a in range(gh)]
        parts = torch.empty(gh, gw, 1, 3, H, W, device=dev)
        out[f"{tag}.taps"] = int(dy.numel())
        for adj in (False, True):
            def field():
                ops.psf_field_apply(x, o, dy, dx, w, tabs, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj)

            def single():
                ops.psf_apply(x, o, dy, dx, wn[gh // 2][gw // 2], Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj)

            def composed():
                if not adj:
                    for a in range(gh):
                        for b in range(gw):
                            ops.psf_apply(x, parts[a, b], dy, dx, wn[a][b], Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W)
                    return (hat[:, :, None, None] * parts).sum(dim=(0, 1))
                u = (hat[:, :, None, None] * x).contiguous()
                for a in range(gh):
                    for b in range(gw):
                        ops.psf_apply(u[a, b], parts[a, b], dy, dx, wn[a][b], Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=True)
                return parts.sum(dim=(0, 1))
            name = f"{tag}.{'adj' if adj else 'fwd'}"
            out[name + ".field"] = _timed(field, reps)
            out[name + ".single"] = _timed(single, reps)
            out[name + ".composed"] = _timed(composed, max(1, reps // 5))
            out[name + ".field_again"] = _timed(field, reps)
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
        print(json.dumps({"apply_us": apply_times(dev, a.reps)}))
        return
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**dict(bench.UNET_KW, pretrain_model="imagenet"))
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (3, 6)
    x_T, ref = bench.synthetic_inputs(0, 1, 256)
    x_T, ref = x_T[:, :3].contiguous().to(dev), ref.to(dev)
    field = M.get_operator("field_blur", device=dev, **FIELDS["roll_shake"])
    single = M.get_operator("psf_blur", device=dev, kernel=field.kernels()[0, 0])
    y = field.forward(ref).detach()
    conds = {name: CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0), scale="3")
             for name, op in (("field_blur", field), ("psf_blur", single))}

    def chain(c, steps):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, clip_denoised=True, timestep_respacing=str(steps)))
        assert sampler._fast_path_ok(model, c.conditioning, "imagenet", True, bench.PATTERN, tuple(x_T.shape)) is c
        torch.manual_seed(0)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        img = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=c.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=bench.PATTERN)
        torch.cuda.synchronize()
        return time.perf_counter() - t0, img

    out = {"net": "3 -> 6", "steps": a.window, "conv_mode": model.conv_mode, "batch": 1, "kernel_size": K, "grid": list(field.grid),
           "ms_per_step": {}, "finite": {}}
    for c in conds.values():
        chain(c, a.warmup)
    for _ in range(a.rounds):
        for name, c in conds.items():
            dt, img = chain(c, a.window)
            out["ms_per_step"].setdefault(name, []).append(round(1e3 * dt / a.window, 3))
            out["finite"][name] = bool(torch.isfinite(img).all())
    out["apply_us"] = apply_times(dev, a.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
