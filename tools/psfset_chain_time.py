#!/usr/bin/env python3
"""Wall time per step of full-size blind-deblurring chains (DDPM.p_sample + `ps`, clip_denoised, gaussian noiser with sigma 0,
`blind_blur` k = 31, n_iter = 1) with ONE learnt PSF for the batch against one PER IMAGE (include/osmosis_psfset.h), on the 3 -> 6
network (the bench architecture, seeded weights), 256 x 256, f16x3.  ONE process; after a warm-up chain each, the chains of a
group alternate `--rounds` times:

    (a) B = 4 shared        (b) B = 4 per_image                        ... again      -- equal launch counts; nb step workgroups for one
    (c) B = 1                                                                          -- (b) per image should lie below it
    (d) B = 4 per_image walked [2, 2]        B = 4 shared walked [2, 2]  ... again     -- the shared walk re-runs every chunk's forward

Every image of a batch is measured through its own shake, y_b = motion_blur(k, 0.5, seed b)(ref_b).

It then times osm_psf_apply_s against osm_psf_apply alone at 3 x 256^2 (forward and adjoint) for the default 61 x 61 trajectory's
taps and a dense 31 x 31 list: device events around `--reps` back-to-back launches after a warm-up (`apply_us`).  With
`--parent-lib PATH` (a libosmosis_hip.so built from the parent commit) the parent's osm_psf_apply is timed in the same call, through
ctypes, on the same buffers.

    python tools/psfset_chain_time.py [--window 200] [--warmup 8] [--conv-mode f16x3] [--reps 50] [--rounds 2] [--parent-lib PATH]

Prints one JSON line.  Seeded synthetic weights do not denoise and their chains can go non-finite: `finite` says
whether the image did; every kernel estimate must stay finite, non-negative and of sum 1 either way (`kernel_ok`).  Compare the
chains of one run only.
"""
import argparse
import contextlib
import ctypes
import io
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench  # noqa: E402  (configuration constants of the benchmark)
from osmosis_diffusion_code_amd import _lib, ops  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M  # noqa: E402
from osmosis_diffusion_code_amd.guided_diffusion import unet  # noqa: E402

K = 31


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


def apply_times(dev, reps, parent_lib=None):
    """{name: microseconds per launch}: osm_psf_apply, osm_psf_apply_s with one set (strides 0, 0) and with one set per plane, and the
    parent library's osm_psf_apply, B = 1, 3 planes of 256 x 256, alternated in this order per tap list and direction."""
    H = W = 256
    g = torch.Generator().manual_seed(0)
    x = torch.randn(1, 3, H, W, generator=g).to(dev)
    o = torch.empty(1, 3, H, W, device=dev)
    parent = None
    if parent_lib:
        parent = ctypes.CDLL(parent_lib).osm_psf_apply
        parent.argtypes, parent.restype = _lib.SIGS["osm_psf_apply"], ctypes.c_int
    lists = {"motion61": M.get_operator("motion_blur", device=dev), "dense31": M.get_operator("blind_blur", device=dev, kernel_size=31)}
    out = {}
    for tag, op in lists.items():
        dy, dx, w = op.taps(dev)
        Ry, Rx = op.radius()
        w1, w3 = w.reshape(1, 1, -1).contiguous(), w.reshape(1, 1, -1).repeat(1, 3, 1).contiguous()
        for adj in (False, True):
            name = f"{tag}.{'adj' if adj else 'fwd'}"
            out[name + ".apply"] = _timed(lambda: ops.psf_apply(x, o, dy, dx, w, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj), reps)
            out[name + ".apply_s"] = _timed(lambda: ops.psf_apply_s(x, o, dy, dx, w1, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj), reps)
            out[name + ".apply_s_per_plane"] = _timed(lambda: ops.psf_apply_s(x, o, dy, dx, w3, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj),
                                                      reps)
            if parent is not None:
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                args = (x.data_ptr(), o.data_ptr(), dy.data_ptr(), dx.data_ptr(), w.data_ptr(), int(w.numel()), Ry, Rx, 1, 3, 3 * H * W, 3 * H * W,
                        H, W, int(adj), 0, stream)
                assert parent(*args) == 0
                out[name + ".parent_apply"] = _timed(lambda: parent(*args), reps)
            out[name + ".apply_again"] = _timed(lambda: ops.psf_apply(x, o, dy, dx, w, Ry, Rx, 1, 3, 3 * H * W, 3 * H * W, H, W, adjoint=adj), reps)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window", type=int, default=200, help="timed chain length (respaced steps)")
    ap.add_argument("--warmup", type=int, default=8, help="length of the untimed chain that builds plans and graphs")
    ap.add_argument("--conv-mode", default="f16x3")
    ap.add_argument("--reps", type=int, default=50, help="launches per timed kernel window")
    ap.add_argument("--rounds", type=int, default=2, help="how often the chains of a group alternate")
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--parent-lib", default=None, help="a libosmosis_hip.so of the parent commit, for osm_psf_apply in the same call")
    ap.add_argument("--kernels-only", action="store_true", help="only the osm_psf_apply / osm_psf_apply_s launches")
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    if a.kernels_only:
        print(json.dumps({"apply_us": apply_times(dev, a.reps, a.parent_lib)}))
        return
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**dict(bench.UNET_KW, pretrain_model="imagenet"))
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    model.conv_mode = a.conv_mode
    assert (model.in_channels, model.out_channels) == (3, 6)
    B = a.batch
    x_T, ref = bench.synthetic_inputs(0, B, 256)
    x_T, ref = x_T[:, :3].contiguous().to(dev), ref.to(dev)
    y = M.get_operator("motion_blur", device=dev, batch_size=B, kernel_size=K, intensity=0.5, seed=list(range(B))).forward(ref).detach()

    def cond(n, per_image):
        op = M.get_operator("blind_blur", device=dev, batch_size=n, kernel_size=K, n_iter=1, per_image=per_image)
        return CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0), scale="3")

    def chain(c, n, steps, chunks=None):
        sampler = gd.create_sampler(**dict(bench.DIFFUSION, clip_denoised=True, timestep_respacing=str(steps)))
        assert sampler._fast_path_ok(model, c.conditioning, "imagenet", True, bench.PATTERN, (n,) + tuple(x_T.shape[1:])) is c
        saved = gd.GaussianDiffusion.__dict__["chunk_sizes"]          # (the staticmethod object itself)
        if chunks is not None:
            gd.GaussianDiffusion.chunk_sizes = staticmethod(lambda Bc, cap: list(chunks))
        try:
            torch.manual_seed(0)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            img = sampler.p_sample_loop(model=model, x_start=x_T[:n], measurement=y[:n], measurement_cond_fn=c.conditioning, record=False,
                                        save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=bench.PATTERN)
            torch.cuda.synchronize()
            return time.perf_counter() - t0, img
        finally:
            gd.GaussianDiffusion.chunk_sizes = saved

    half = [B // 2, B - B // 2]
    groups = [{"a.shared": (cond(B, False), B, None), "b.per_image": (cond(B, True), B, None)},
              {"c.single": (cond(1, False), 1, None)},
              {"d.per_image.chunked": (cond(B, True), B, half), "d.shared.chunked": (cond(B, False), B, half)}]
    out = {"net": "3 -> 6", "steps": a.window, "conv_mode": model.conv_mode, "batch": B, "kernel_size": K, "ms_per_step": {}, "finite": {},
           "kernel_ok": {}}
    for group in groups:
        for name, (c, n, chunks) in group.items():
            chain(c, n, a.warmup, chunks)
        for _ in range(a.rounds):
            for name, (c, n, chunks) in group.items():
                c.operator.reset()
                dt, img = chain(c, n, a.window, chunks)
                out["ms_per_step"].setdefault(name, []).append(round(1e3 * dt / a.window, 3))
                out["finite"][name] = bool(torch.isfinite(img).all())
                est = c.operator.kernels()
                out["kernel_ok"][name] = bool(np.isfinite(est).all() and (est >= 0).all() and np.abs(est.sum(axis=(2, 3)) - 1.0).max() < 1e-5)
    out["apply_us"] = apply_times(dev, a.reps, a.parent_lib)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
