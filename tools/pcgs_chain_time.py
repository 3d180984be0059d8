#!/usr/bin/env python3
"""Wall time of a full-size guided Osmosis chain with the PCGS inner alternation (local_M = 3 in [s_end, s_start] = [0.2, 0.6]:
each index there runs its step three times at the same t), on the fused loop or, with --generic, on `_generic_loop`
(OSM_FUSED_PCGS=0: autograd over the HIP UNet operator).  Bench network (552.8 M parameters, seeded weights), 256 x 256, B = 1,
revised underwater operator, n_iter = 20.  Prints one JSON line: sub-steps, seconds, ms per sub-step, finiteness.

    python tools/pcgs_chain_time.py [--steps 1000] [--local-M 3] [--generic] [--last N]

Seeded synthetic weights do not denoise: a chain's prediction leaves the operator's range and the outputs may go non-finite (SURVEY
F10; `finite` in the output line), which a power-limited kernel runs faster -- compare loops and local_M on the same setting only.
--last N times the fused loop over the last N indices from x_T scaled by 0.1 (as tools/full_chain.py --last does); with --local-M 1
it gives the per-step cost of the same window (`_generic_loop` has no index range).
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
    ap.add_argument("--steps", type=int, default=1000, help="respaced chain length")
    ap.add_argument("--local-M", type=int, default=3)
    ap.add_argument("--generic", action="store_true", help="OSM_FUSED_PCGS=0: time `_generic_loop`")
    ap.add_argument("--last", type=int, default=0, help="fused loop only: the last N indices from a bounded state")
    a = ap.parse_args()
    assert not (a.generic and a.last), "--last needs the fused loop"
    if a.generic:
        os.environ["OSM_FUSED_PCGS"] = "0"
    dev = torch.device("cuda", 0)
    with contextlib.redirect_stdout(io.StringIO()):
        model = unet.create_model(**bench.UNET_KW)
    bench.seeded_weights(model)
    model = model.to(dev).eval()
    pattern = dict(bench.PATTERN, local_M=a.local_M, s_start=0.6, s_end=0.2)
    sampler = gd.create_sampler(**dict(bench.DIFFUSION, timestep_respacing=str(a.steps)))
    T = sampler.num_timesteps
    first = a.last - 1 if a.last else T - 1
    n_sub = sum(alt for _, _, alt in gd.pcgs_schedule(pattern, T)[T - 1 - first:])
    op = M.get_operator("underwater_physical_revised", device=dev, batch_size=1, **bench.OPERATOR)
    cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **bench.COND, **pattern, aux_loss=bench.AUX)
    fused = sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, pattern, (1, 4, 256, 256)) is not None
    assert fused != a.generic, "the chain did not take the requested loop"
    x_T, y = bench.synthetic_inputs(0, 1, 256)
    x_T, y = x_T.to(dev), y.to(dev)
    kw = dict(index_range=(first, 0)) if a.last else {}
    if a.last:
        x_T = 0.1 * x_T
    torch.manual_seed(0)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    img, _variables, loss, x0 = sampler.p_sample_loop(model=model, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning,
                                                      record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False,
                                                      sample_pattern=pattern, **kw)
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"loop": "fused" if fused else "generic", "steps": T, "indices": first + 1, "local_M": a.local_M,
                      "sub_steps": n_sub, "seconds": round(dt, 2), "ms_per_sub_step": round(1e3 * dt / n_sub, 2),
                      "finite": bool(torch.isfinite(img).all() and torch.isfinite(x0).all()),
                      "final_loss": [float(v) for v in torch.as_tensor(loss).detach().cpu().reshape(-1)]}))


if __name__ == "__main__":
    main()
