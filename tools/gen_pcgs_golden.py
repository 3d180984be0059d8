"""CPU generator of tests/golden/loop_pcgs.npz: the PCGS inner alternation (`local_M > 1`) through the REAL reference.

Inside the [s_end, s_start] window the reference repeats each index's step `alternate_len` times at the same t
(guided_diffusion/gaussian_diffusion.py:225-309; osmosis_utils/utils.py:595-630 set_alternate_length); each repeat is a full step
(network, posterior, conditioning with its own n_iter phi steps, q_sample / step noise).  The chains run the tiny seeded UNet at 16 x 16
with 10 respaced steps (use_timesteps = range(0, 100, 10)); every torch.randn_like draw and every conditioning call is logged.
Recorded:
  osm.<op>.<win>.*   the guided Osmosis loop (<op> = revised: underwater_physical_revised, haze: haze_physical), local_M = 3,
                     update window [0, 0.7], sub-step window <win> = w62: [0.2, 0.6] (3 sub-steps at indices 6..2, 20 calls) or
                     w50: [0, 0.5] (indices 5..0, index 0 without noise, 22 calls; revised only): per call loss and phi, x0 and grad
                     on every second row and column (`x0_s2`, `grad_s2`: the fixture stays small); the step noise (`noise`, one per
                     call); final img, x0 and phi; drift_1e-6 (how far the reference's own final image moves when x_T is perturbed by
                     1e-6 N(0,1)); x_in (every call's input, for a teacher-forced comparison) when that drift exceeds 1e-3
  ps.<name>.*        the rgb-guidance chains (DDPM.p_sample / DDIM.p_sample + `ps`), local_M = 2 in [0, 0.5] (16 calls, index 0
                     alternates): per call loss; p_sample's draws (`draws_x`, one per call); final img; drift_1e-6 (x_in as above)
  sched.*            the reference's (guidance flag, is_freeze_phi, set_alternate_length) for idx = T-1 .. 0 over a grid of
                     patterns (`sched.pat`: update_start, update_end, s_start, s_end, local_M, start_guidance, stop_guidance,
                     original) and T in {10, 1000} (`sched.T<T>`, [pattern, T-1-idx, 3] int8).  The guidance flag is what the
                     reference's loop does (is the conditioner called at that index), observed on a stub network; `sched.calls.T<T>`
                     counts the conditioning calls per index.  `sched.bad`: patterns set_alternate_length asserts on.

Reuses oracle/tools/gen_golden.py (the reference import set-up, tiny_model, OPERATORS, PATTERN).  Run: python tools/gen_pcgs_golden.py [OUT]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))

import gen_golden as G  # noqa: E402  (puts the reference and its stubs on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from osmosis_utils import utils as R_utils  # noqa: E402  (the reference's osmosis_utils/utils.py)

OUT = os.path.join(REPO, "tests", "golden", "loop_pcgs.npz")
npy = G.npy
HW = 16
WINDOWS = {"w62": (0.6, 0.2), "w50": (0.5, 0.0)}
OSM_CHAINS = [("revised", "underwater_physical_revised", "w62"), ("revised", "underwater_physical_revised", "w50"),
              ("haze", "haze_physical", "w62")]


def pattern(win, local_M):
    s_start, s_end = WINDOWS[win]
    return dict(G.PATTERN, local_M=local_M, s_start=s_start, s_end=s_end)


def _sampler(name):
    return G.R_gd.get_sampler(name)(use_timesteps=range(0, 100, 10), betas=G.R_gd.get_named_beta_schedule("linear", 1000),
                                    model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False,
                                    clip_denoised=False, rescale_timesteps=False)


class _DrawLog:
    """Logs every torch.randn_like draw while active (seeded with torch.manual_seed(0) on entry)."""

    def __enter__(self):
        self.draws, self.orig = [], torch.randn_like

        def logged(t, **kw):
            r = self.orig(t, **kw)
            self.draws.append(r.clone())
            return r
        torch.manual_seed(0)
        torch.randn_like = logged
        return self

    def __exit__(self, *exc):
        torch.randn_like = self.orig
        return False


def osmosis_chain(m, opname, win, perturb=0.0):
    spec = G.OPERATORS[opname]
    pat = pattern(win, 3)
    operator = G.get_operator(device=torch.device("cpu"), batch_size=1, **spec["operator"])
    cond = G.get_conditioning_method("osmosis", operator, G.get_noise(name="clean"), **spec["cond"], **pat, **spec["aux"])
    sampler = _sampler("ddpm")
    x_T = 0.5 * torch.randn(1, 4, HW, HW, generator=torch.Generator().manual_seed(0))
    if perturb:
        x_T = x_T + perturb * torch.randn(1, 4, HW, HW, generator=torch.Generator().manual_seed(77))
    y = torch.rand(1, 3, HW, HW, generator=torch.Generator().manual_seed(7)) * 1.6 - 0.8
    trace, orig_cond = [], cond.conditioning

    def traced(**kw):
        rec = {"x_in": kw["x_prev"].detach().clone(), "x0": kw["x_0_hat"].detach().clone()}
        ret = orig_cond(**kw)
        rec["loss"] = np.array(ret[1], dtype=np.float32)
        rec["phi"] = {k: v.detach().clone() for k, v in ret[2].items()}
        rec["grad"] = ret[3].clone()
        trace.append(rec)
        return ret

    with _DrawLog() as log:
        img, variables, loss, x0 = sampler.p_sample_loop(
            model=m, x_start=x_T.clone().requires_grad_(), measurement=y, measurement_cond_fn=traced, record=False,
            save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat)
    # per call: q_sample's draw (3 channels, unused), then the step noise (4 channels)
    assert [d.shape[1] for d in log.draws] == [3, 4] * len(trace), [d.shape[1] for d in log.draws]
    return dict(x_T=x_T, y=y, img=img, x0=x0, variables=variables, trace=trace, noise=[d for d in log.draws if d.shape[1] == 4])


def ps_chain(m, name, perturb=0.0):
    pat = pattern("w50", 2)
    operator = G.get_operator(name="rgb_guidance", device=torch.device("cpu"), batch_size=1)
    cond = G.get_conditioning_method("ps", operator, G.get_noise(name="gaussian", sigma=0.05), scale="0.6,0.5,0.4,0.0")
    sampler = _sampler(name)
    x_T = 0.5 * torch.randn(1, 4, HW, HW, generator=torch.Generator().manual_seed(2))
    if perturb:
        x_T = x_T + perturb * torch.randn(1, 4, HW, HW, generator=torch.Generator().manual_seed(77))
    y = torch.rand(1, 3, HW, HW, generator=torch.Generator().manual_seed(9)) * 1.6 - 0.8
    losses, x_ins, orig_cond = [], [], cond.conditioning

    def traced(**kw):
        x_ins.append(kw["x_prev"].detach().clone())
        ret = orig_cond(**kw)
        losses.append(float(ret[1].detach()))
        return ret

    with _DrawLog() as log:
        img = sampler.p_sample_loop(model=m, x_start=x_T.clone().requires_grad_(), measurement=y, measurement_cond_fn=traced,
                                    record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=True, sample_pattern=pat)
    # per call: p_sample's draw (4 channels), then q_sample's (3 channels)
    assert [d.shape[1] for d in log.draws] == [4, 3] * len(losses), [d.shape[1] for d in log.draws]
    return dict(x_T=x_T, y=y, img=img, losses=losses, x_in=x_ins, draws_x=[d for d in log.draws if d.shape[1] == 4])


def gen_chains(m, out):
    for tag_op, opname, win in OSM_CHAINS:
        r = osmosis_chain(m, opname, win)
        tag = f"osm.{tag_op}.{win}"
        out[f"{tag}.x_T"], out[f"{tag}.y"] = npy(r["x_T"]), npy(r["y"])
        drift = float((osmosis_chain(m, opname, win, perturb=1e-6)["img"] - r["img"]).abs().max())
        out[f"{tag}.drift_1e-6"] = np.array(drift)
        if drift > 1e-3:
            out[f"{tag}.x_in"] = np.stack([npy(t["x_in"]) for t in r["trace"]])
        for key in ("x0", "grad"):
            out[f"{tag}.{key}_s2"] = np.stack([npy(t[key][..., ::2, ::2]) for t in r["trace"]])
        out[f"{tag}.loss"] = np.stack([t["loss"] for t in r["trace"]])
        for k in r["trace"][0]["phi"]:
            out[f"{tag}.phi.{k}"] = np.stack([npy(t["phi"][k]) for t in r["trace"]])
        out[f"{tag}.noise"] = np.stack([npy(d) for d in r["noise"]])
        out[f"{tag}.final_img"], out[f"{tag}.final_x0"] = npy(r["img"]), npy(r["x0"])
        for k, v in r["variables"].items():
            out[f"{tag}.final.{k}"] = npy(v)
        print(tag, "calls", len(r["trace"]), "final loss", float(out[f"{tag}.loss"][-1].reshape(-1)[0]),
              "drift", float(out[f"{tag}.drift_1e-6"]))
    for name in ("ddpm", "ddim"):
        r = ps_chain(m, name)
        tag = f"ps.{name}"
        out[f"{tag}.x_T"], out[f"{tag}.y"] = npy(r["x_T"]), npy(r["y"])
        drift = float((ps_chain(m, name, perturb=1e-6)["img"] - r["img"]).abs().max())
        out[f"{tag}.drift_1e-6"] = np.array(drift)
        if drift > 1e-3:
            out[f"{tag}.x_in"] = np.stack([npy(x) for x in r["x_in"]])
        out[f"{tag}.loss"] = np.array(r["losses"], dtype=np.float32)
        out[f"{tag}.draws_x"] = np.stack([npy(d) for d in r["draws_x"]])
        out[f"{tag}.final_img"] = npy(r["img"])
        print(tag, "calls", len(r["losses"]), "final loss", r["losses"][-1], "drift", float(out[f"{tag}.drift_1e-6"]))


# ------------------------------------------------------------------------------------------------------------ the schedule
# (update_start, update_end, s_start, s_end, local_M, start_guidance, stop_guidance, original)
GRID = [(0.7, 0.0, 1.0, 0.0, 1, 1.0, 0.0, 0), (0.7, 0.0, 0.6, 0.2, 3, 1.0, 0.0, 0), (0.7, 0.0, 0.5, 0.0, 3, 1.0, 0.0, 0),
        (1.0, 0.0, 1.0, 0.0, 2, 1.0, 0.0, 0), (0.7, 0.1, 0.65, 0.15, 4, 1.0, 0.3, 0), (0.9, 0.2, 0.55, 0.25, 2, 1.0, 0.5, 0),
        (0.7, 0.0, 0.6, 0.2, 1, 1.0, 0.0, 0), (0.8, 0.05, 0.8, 0.05, 5, 1.0, 0.0, 0), (0.7, 0.0, 0.6, 0.2, 3, 1.0, 0.0, 1),
        (0.35, 0.0, 0.3, 0.1, 2, 1.0, 0.0, 0), (0.7, 0.0, 0.6, 0.2, 3, 1.0, 0.9, 0)]
# patterns set_alternate_length asserts on: update_start <= update_end, s_start <= s_end, and with local_M > 1 an s window that leaves
# the update window (local_M = 1 with such a window is accepted)
BAD = [(0.5, 0.5, 0.6, 0.2, 3, 1.0, 0.0, 0), (0.3, 0.5, 0.6, 0.2, 1, 1.0, 0.0, 0), (0.7, 0.0, 0.4, 0.4, 3, 1.0, 0.0, 0),
       (0.7, 0.0, 0.2, 0.6, 1, 1.0, 0.0, 0), (0.7, 0.0, 0.8, 0.2, 3, 1.0, 0.0, 0), (0.7, 0.1, 0.6, 0.05, 2, 1.0, 0.0, 0)]
OK_M1 = [(0.7, 0.0, 0.8, 0.2, 1, 1.0, 0.0, 0), (0.7, 0.1, 0.6, 0.05, 1, 1.0, 0.0, 0)]


def as_pattern(row):
    us, ue, ss, se, lm, sg, tg, orig = row
    return dict(pattern="original" if orig else "pcgs", update_start=us, update_end=ue, s_start=ss, s_end=se, local_M=int(lm),
                global_N=1, n_iter=1, start_guidance=sg, stop_guidance=tg)


class _StubNet:
    """model(x, t) of the shape the learned_range variance needs; the loop's control flow is what is observed."""

    def __call__(self, x, t, **kw):
        return torch.zeros(x.shape[0], 2 * x.shape[1], *x.shape[2:])


def reference_schedule(row, T):
    """The reference loop's per-index decisions: guided (the conditioner is called), is_freeze_phi, set_alternate_length; and the
    number of conditioning calls per index (idx = T-1 .. 0)."""
    pat = as_pattern(row)
    sampler = G.R_gd.create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                                    model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False,
                                    rescale_timesteps=False, timestep_respacing=[T])
    calls = {}

    def cond(**kw):
        idx = int(kw["time_index"] * T + 0.5)
        calls[idx] = calls.get(idx, 0) + 1
        return kw["x_t"].detach().clone(), torch.zeros(1), {}, kw["x_t"].detach(), None

    with _DrawLog():
        sampler.p_sample_loop(model=_StubNet(), x_start=torch.zeros(1, 4, 2, 2), measurement=torch.zeros(1, 3, 2, 2),
                              measurement_cond_fn=cond, record=False, save_root=None, pretrain_model="osmosis",
                              rgb_guidance=False, sample_pattern=pat)
    rows = [(int(idx in calls), int(bool(R_utils.is_freeze_phi(pat, idx, T))), int(R_utils.set_alternate_length(pat, idx, T)))
            for idx in range(T - 1, -1, -1)]
    return np.array(rows, dtype=np.int8), np.array([calls.get(idx, 0) for idx in range(T - 1, -1, -1)], dtype=np.int8)


def gen_schedule(out):
    out["sched.pat"] = np.array(GRID, dtype=np.float64)
    for T in (10, 1000):
        rows = [reference_schedule(r, T) for r in GRID]
        out[f"sched.T{T}"] = np.stack([r[0] for r in rows])
        out[f"sched.calls.T{T}"] = np.stack([r[1] for r in rows])
    for row in BAD:
        try:
            R_utils.set_alternate_length(as_pattern(row), 0, 10)
        except AssertionError:
            continue
        raise RuntimeError(f"the reference accepts {row}")
    for row in OK_M1:
        R_utils.set_alternate_length(as_pattern(row), 0, 10)
    out["sched.bad"] = np.array(BAD, dtype=np.float64)
    out["sched.ok"] = np.array(OK_M1, dtype=np.float64)


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    m, _cfg, _sd = G.tiny_model()
    out = {}
    gen_schedule(out)
    gen_chains(m, out)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
