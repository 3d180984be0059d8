"""CPU generator of tests/golden/loop_dynthr.npz: `dynamic_threshold: True` through the REAL reference.

The reference's process_xstart (guided_diffusion/posterior_mean_variance.py:43-50) calls util/img_utils.py:8-15
`dynamic_thresholding(x, s=0.98)` = clip(x * torch.quantile(|x|, 0.98), -1, 1), the quantile over the WHOLE [B,4,H,W] tensor.
Recorded (every torch.quantile call is logged, so each step carries the q it used):
  osmosis.clip{0,1}.*  the 10-step guided Osmosis loop (revised underwater operator, tiny seeded UNet) with dynamic_threshold on and
                       clip_denoised off / on; x_T, y and noise of loop_underwater_physical_revised.npz (asserted): per-step x0, grad,
                       loss, q; final img, x0, phi; drift_1e-6 (how far the reference's own final image moves when x_T is perturbed by
                       1e-6 N(0,1)); x_in (every step's input) when that drift exceeds 1e-3
  ps.{ddpm,ddim}.*     the rgb-guidance chains (DDPM.p_sample / DDIM.p_sample + `ps`) with the draws of loop_ps.npz (asserted): per-step
                       loss and q, final img, drift_1e-6 (x_in as above)
  px.{free,ties}.*     dynamic_thresholding itself on seeded [2,4,16,16] tensors, tie-free and with heavy ties: x, the cotangent w,
                       y = dynamic_thresholding(x, 0.98), q, and the VJP dx = (dy/dx)^T w by torch.autograd

Reuses oracle/tools/gen_golden.py (the reference import set-up, tiny_model, OPERATORS, PATTERN).  Run: python tools/gen_dynthr_golden.py
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))

import gen_golden as G  # noqa: E402  (puts the reference and its stubs on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

from util import img_utils as R_img  # noqa: E402  (the reference's util/img_utils.py)

OUT = os.path.join(REPO, "tests", "golden", "loop_dynthr.npz")
npy = G.npy


class _QuantileLog:
    """Logs every torch.quantile result while active (the reference calls it as torch.quantile)."""

    def __enter__(self):
        self.values, self.orig = [], torch.quantile

        def logged(*a, **k):
            r = self.orig(*a, **k)
            self.values.append(float(r.detach()))
            return r
        torch.quantile = logged
        return self

    def __exit__(self, *exc):
        torch.quantile = self.orig
        return False


def _sampler(name, clip_denoised):
    return G.R_gd.get_sampler(name)(use_timesteps=range(0, 100, 10), betas=G.R_gd.get_named_beta_schedule("linear", 1000),
                                    model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=True,
                                    clip_denoised=clip_denoised, rescale_timesteps=False)


def _draw_log():
    draws, orig = [], torch.randn_like

    def logged(t, **kw):
        r = orig(t, **kw)
        draws.append(r.clone())
        return r
    return draws, orig, logged


def osmosis_chain(m, clip_denoised, perturb=0.0):
    spec = G.OPERATORS["underwater_physical_revised"]
    operator = G.get_operator(device=torch.device("cpu"), batch_size=1, **spec["operator"])
    cond = G.get_conditioning_method("osmosis", operator, G.get_noise(name="clean"), **spec["cond"], **G.PATTERN, **spec["aux"])
    sampler = _sampler("ddpm", clip_denoised)
    x_T = 0.5 * torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(0))
    if perturb:
        x_T = x_T + perturb * torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(77))
    y = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(7)) * 1.6 - 0.8
    trace, orig_cond = [], cond.conditioning

    def traced(**kw):
        rec = {"x_in": kw["x_prev"].detach().clone(), "x0": kw["x_0_hat"].detach().clone()}
        ret = orig_cond(**kw)
        rec["loss"] = np.array(ret[1], dtype=np.float32)
        rec["grad"] = ret[3].clone()
        trace.append(rec)
        return ret

    draws, orig_randn, logged = _draw_log()
    torch.manual_seed(0)
    torch.randn_like = logged
    try:
        with _QuantileLog() as ql:
            img, variables, loss, x0 = sampler.p_sample_loop(
                model=m, x_start=x_T.clone().requires_grad_(), measurement=y, measurement_cond_fn=traced, record=False,
                save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=G.PATTERN)
    finally:
        torch.randn_like = orig_randn
    assert len(trace) == 10 and len(ql.values) == 10, (len(trace), len(ql.values))
    return dict(x_T=x_T, y=y, img=img, x0=x0, variables=variables, trace=trace, q=ql.values,
                noise=[d for d in draws if d.shape[1] == 4])


def ps_chain(m, name, perturb=0.0):
    operator = G.get_operator(name="rgb_guidance", device=torch.device("cpu"), batch_size=1)
    cond = G.get_conditioning_method("ps", operator, G.get_noise(name="gaussian", sigma=0.05), scale="0.6,0.5,0.4,0.0")
    sampler = _sampler(name, False)
    x_T = 0.5 * torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(2))
    if perturb:
        x_T = x_T + perturb * torch.randn(1, 4, 32, 32, generator=torch.Generator().manual_seed(77))
    y = torch.rand(1, 3, 32, 32, generator=torch.Generator().manual_seed(9)) * 1.6 - 0.8
    losses, x_ins, orig_cond = [], [], cond.conditioning

    def traced(**kw):
        x_ins.append(kw["x_prev"].detach().clone())
        ret = orig_cond(**kw)
        losses.append(float(ret[1]))
        return ret

    draws, orig_randn, logged = _draw_log()
    torch.manual_seed(0)
    torch.randn_like = logged
    try:
        with _QuantileLog() as ql:
            img = sampler.p_sample_loop(model=m, x_start=x_T.clone().requires_grad_(), measurement=y, measurement_cond_fn=traced,
                                        record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=True,
                                        sample_pattern=G.PATTERN)
    finally:
        torch.randn_like = orig_randn
    assert len(losses) == 10 and len(ql.values) == 10, (len(losses), len(ql.values))
    return dict(x_T=x_T, y=y, img=img, losses=losses, q=ql.values, x_in=x_ins, draws_x=[d for d in draws if d.shape[1] == 4])


def gen_chains(m, out):
    base = dict(np.load(os.path.join(G.OUT, "loop_underwater_physical_revised.npz")))
    ps = dict(np.load(os.path.join(G.OUT, "loop_ps.npz")))
    for clip in (False, True):
        r = osmosis_chain(m, clip)
        assert np.array_equal(npy(r["x_T"]), base["x_T"]) and np.array_equal(npy(r["y"]), base["y"])
        assert np.array_equal(np.stack([npy(d) for d in r["noise"]]), base["noise"])
        tag = f"osmosis.clip{int(clip)}"
        drift = float((osmosis_chain(m, clip, perturb=1e-6)["img"] - r["img"]).abs().max())
        out[f"{tag}.drift_1e-6"] = np.array(drift)
        if drift > 1e-3:
            out[f"{tag}.x_in"] = np.stack([npy(t["x_in"]) for t in r["trace"]])
        out[f"{tag}.x0"] = np.stack([npy(t["x0"]) for t in r["trace"]])
        out[f"{tag}.grad"] = np.stack([npy(t["grad"]) for t in r["trace"]])
        out[f"{tag}.loss"] = np.stack([t["loss"] for t in r["trace"]])
        out[f"{tag}.q"] = np.array(r["q"], dtype=np.float32)
        out[f"{tag}.final_img"], out[f"{tag}.final_x0"] = npy(r["img"]), npy(r["x0"])
        for k, v in r["variables"].items():
            out[f"{tag}.{k}"] = npy(v)
        print(tag, "q", np.round(r["q"], 4), "final loss", float(out[f"{tag}.loss"][-1].reshape(-1)[0]), "drift", drift)
    for name in ("ddpm", "ddim"):
        r = ps_chain(m, name)
        assert np.array_equal(npy(r["x_T"]), ps[f"{name}.x_T"]) and np.array_equal(npy(r["y"]), ps[f"{name}.y"])
        assert np.array_equal(np.stack([npy(d) for d in r["draws_x"]]), ps[f"{name}.draws_x"])
        tag = f"ps.{name}"
        drift = float((ps_chain(m, name, perturb=1e-6)["img"] - r["img"]).abs().max())
        out[f"{tag}.drift_1e-6"] = np.array(drift)
        if drift > 1e-3:
            out[f"{tag}.x_in"] = np.stack([npy(x) for x in r["x_in"]])
        out[f"{tag}.loss"] = np.array(r["losses"], dtype=np.float32)
        out[f"{tag}.q"] = np.array(r["q"], dtype=np.float32)
        out[f"{tag}.final_img"] = npy(r["img"])
        print(tag, "q", np.round(r["q"], 4), "final loss", r["losses"][-1], "drift", drift)


def gen_vjp(out):
    g = torch.Generator().manual_seed(31)
    x = 1.3 * torch.randn(2, 4, 16, 16, generator=g)
    w = torch.randn(2, 4, 16, 16, generator=g)
    for tag, xv in (("free", x), ("ties", torch.round(x * 4.0) / 4.0)):
        xr = xv.clone().requires_grad_(True)
        with _QuantileLog() as ql:
            y = R_img.dynamic_thresholding(xr, s=0.98)
        (dx,) = torch.autograd.grad((y * w).sum(), xr)
        out[f"px.{tag}.x"], out[f"px.{tag}.w"], out[f"px.{tag}.y"], out[f"px.{tag}.dx"] = npy(xv), npy(w), npy(y), npy(dx)
        out[f"px.{tag}.q"] = np.array(ql.values, dtype=np.float32)
        print(f"px.{tag}", "q", ql.values, "distinct |x|", int(xv.abs().unique().numel()))


def main():
    m, _cfg, _sd = G.tiny_model()
    out = {}
    gen_vjp(out)
    gen_chains(m, out)
    np.savez_compressed(OUT, **out)
    print(OUT, os.path.getsize(OUT))


if __name__ == "__main__":
    main()
