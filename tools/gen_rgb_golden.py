"""CPU generator of tests/golden/loop_rgb.npz: the 3-channel (RGB) model family through the REAL reference.

`create_model` builds a 3 -> 6 network (3 -> 3 without learn_sigma) for any pretrain_model other than "osmosis"
(guided_diffusion/unet.py); such a model takes two branches of `p_sample_loop` (guided_diffusion/gaussian_diffusion.py:232-238,
:298-306): the rgb-guidance one (`p_sample` + `ps`) and the mean-only one (`p_mean_variance`, sample = mean, `ps`, no noise).  The
networks are the tiny architecture of the other fixtures with pretrain_model = "imagenet" and the oracle's seeded weights
(`seeded_state_dict(cfg, 1234)`: the tests rebuild them, nothing is stored).  Recorded:
  unet.<net>.*       <net> = c36 (3 -> 6) | c33 (3 -> 3): x [2,3,32,32], t, y = model(x, t), dx = d sum(y[:, :3]^2) / d x, the weights'
                     abs-sum and parameter count
  <chain>.*          16 x 16, 10 respaced steps (use_timesteps = range(0, 100, 10)), `ps` with scale 0.3 on the `noise` operator with
                     the gaussian noiser (sigma = 0).  <chain> = <branch>.<sampler>.<net>[.clip|.dyn|.m2]:
                       branch  rg (rgb_guidance=True) | mo (mean-only);  sampler ddpm | ddim;  net c36 (learned_range) | c33 (fixed_small)
                       .clip clip_denoised=True, .dyn dynamic_threshold=True, .m2 local_M = 2 in [0, 0.5] (16 calls)
                     x_T, y, per call `loss`, final_img, drift_1e-6 (how far the reference's own final image moves when x_T is
                     perturbed by 1e-6 N(0,1)), x_in (every call's input) when that drift exceeds 1e-3.  `draws_x`: p_sample's
                     randn_like draw of every call, for the rg.ddpm chains only -- DDIM at eta = 0 multiplies its draw by sigma = 0,
                     the mean-only branch draws q_sample's unused noise only.
  prior.*            `osmosis_utils/diffusion.py::inverse(image_channels=3)`, t = 6..1 on the 3 -> 6 network at 32 x 32: x_T, the five
                     noise draws, every network call's input (`x_steps`), x_final, the last predicted x_0's clipped RGB (`x_start_rgb`)

Reuses oracle/tools/gen_golden.py (the reference import set-up, TINY_KW, PATTERN).  Run: python tools/gen_rgb_golden.py [OUT]
"""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(REPO, "oracle", "tools"))

import gen_golden as G  # noqa: E402  (puts the reference and its stubs on sys.path)
import numpy as np  # noqa: E402
import torch  # noqa: E402

OUT = os.path.join(REPO, "tests", "golden", "loop_rgb.npz")
npy = G.npy
HW = 16
NETS = {"c36": dict(G.TINY_KW, pretrain_model="imagenet", learn_sigma=True),
        "c33": dict(G.TINY_KW, pretrain_model="imagenet", learn_sigma=False)}
VAR = {"c36": "learned_range", "c33": "fixed_small"}
# (branch, sampler, net, variant)
CHAINS = [("rg", "ddpm", "c36", ""), ("rg", "ddim", "c36", ""), ("mo", "ddpm", "c36", ""),
          ("rg", "ddpm", "c33", ""), ("rg", "ddim", "c33", ""), ("mo", "ddpm", "c33", ""),
          ("rg", "ddpm", "c36", "clip"), ("mo", "ddpm", "c36", "clip"),
          ("rg", "ddpm", "c36", "dyn"), ("mo", "ddpm", "c33", "dyn"),
          ("rg", "ddpm", "c36", "m2"), ("rg", "ddim", "c36", "m2"), ("mo", "ddpm", "c36", "m2")]


def chain_tag(branch, sampler, net, variant):
    return ".".join(p for p in (branch, sampler, net, variant) if p)


def rgb_model(net):
    kw = NETS[net]
    m = G.R_unet.create_model(**kw)
    cfg = G.UNetConfig.from_create_model_kwargs(**kw)
    sd = G.seeded_state_dict(cfg, seed=1234)
    missing = m.load_state_dict(sd, strict=True)
    assert not missing.missing_keys and not missing.unexpected_keys
    assert (m.in_channels, m.out_channels) == (3, 6 if kw["learn_sigma"] else 3)
    return m.eval(), cfg, sd


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


def pattern(variant):
    return dict(G.PATTERN, local_M=2, s_start=0.5, s_end=0.0) if variant == "m2" else dict(G.PATTERN)


def run_chain(m, branch, sampler_name, net, variant, perturb=0.0):
    operator = G.get_operator(name="noise", device=torch.device("cpu"), sigma=0.0)
    cond = G.get_conditioning_method("ps", operator, G.get_noise(name="gaussian", sigma=0.0), scale="0.3")
    sampler = G.R_gd.get_sampler(sampler_name)(
        use_timesteps=range(0, 100, 10), betas=G.R_gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
        model_var_type=VAR[net], dynamic_threshold=variant == "dyn", clip_denoised=variant == "clip", rescale_timesteps=False)
    x_T = 0.5 * torch.randn(1, 3, HW, HW, generator=torch.Generator().manual_seed(4))
    if perturb:
        x_T = x_T + perturb * torch.randn(1, 3, HW, HW, generator=torch.Generator().manual_seed(77))
    y = torch.rand(1, 3, HW, HW, generator=torch.Generator().manual_seed(11)) * 1.6 - 0.8
    losses, x_ins, orig_cond = [], [], cond.conditioning

    def traced(**kw):
        x_ins.append(kw["x_prev"].detach().clone())
        ret = orig_cond(**kw)
        losses.append(float(ret[1].detach()))
        return ret

    with _DrawLog() as log, np.errstate(divide="ignore"):     # fixed_small takes log(0) at index 0 (unused there)
        img = sampler.p_sample_loop(model=m, x_start=x_T.clone().requires_grad_(), measurement=y, measurement_cond_fn=traced,
                                    record=False, save_root=None, pretrain_model="imagenet", rgb_guidance=branch == "rg",
                                    sample_pattern=pattern(variant))
    # per call: p_sample's draw (rgb-guidance only), then q_sample's; all of them [1,3,HW,HW]
    per = 2 if branch == "rg" else 1
    assert len(log.draws) == per * len(losses), (len(log.draws), len(losses))
    assert torch.isfinite(img).all()
    return dict(x_T=x_T, y=y, img=img.detach(), losses=losses, x_in=x_ins, draws_x=log.draws[0::2] if branch == "rg" else [])


def gen_chains(out):
    models = {net: rgb_model(net)[0] for net in NETS}
    for branch, sampler, net, variant in CHAINS:
        tag = chain_tag(branch, sampler, net, variant)
        r = run_chain(models[net], branch, sampler, net, variant)
        drift = float((run_chain(models[net], branch, sampler, net, variant, perturb=1e-6)["img"] - r["img"]).abs().max())
        out[f"{tag}.x_T"], out[f"{tag}.y"] = npy(r["x_T"]), npy(r["y"])
        out[f"{tag}.drift_1e-6"] = np.array(drift)
        if drift > 1e-3:
            out[f"{tag}.x_in"] = np.stack([npy(x) for x in r["x_in"]])
        out[f"{tag}.loss"] = np.array(r["losses"], dtype=np.float32)
        if branch == "rg" and sampler == "ddpm":
            out[f"{tag}.draws_x"] = np.stack([npy(d) for d in r["draws_x"]])
        out[f"{tag}.final_img"] = npy(r["img"])
        print(tag, "calls", len(r["losses"]), "loss", r["losses"][0], "->", r["losses"][-1], "drift", drift,
              "max |img|", float(r["img"].abs().max()))
    out["chains"] = np.array([chain_tag(*c) for c in CHAINS])


def gen_unets(out):
    for net in NETS:
        m, cfg, sd = rgb_model(net)
        g = torch.Generator().manual_seed(5)
        x = torch.randn(2, 3, 32, 32, generator=g).requires_grad_(True)
        t = torch.tensor([3, 250])
        y = m(x, t)
        (gx,) = torch.autograd.grad((y[:, :3] ** 2).sum(), x)
        out[f"unet.{net}.x"], out[f"unet.{net}.t"], out[f"unet.{net}.y"], out[f"unet.{net}.dx"] = npy(x), npy(t), npy(y), npy(gx)
        out[f"unet.{net}.weight_abs_sum"] = np.array(float(sum(v.double().abs().sum() for v in sd.values())))
        out[f"unet.{net}.n_params"] = np.array(sum(v.numel() for v in sd.values()))
        print("unet", net, tuple(y.shape), "max |y|", float(y.abs().max()), "max |dx|", float(gx.abs().max()))


def gen_prior(out):
    """`inverse(image_channels=3)` as RGBD_prior_sampling.py:80 calls it: t = 6..1 on the 3 -> 6 network.  The reference's return
    statement names `x_depth`, which only its 4-channel branch binds (osmosis_utils/diffusion.py:118-130): the call runs the whole
    chain and then raises UnboundLocalError.  The chain is therefore observed at the network (every call's input and output); the
    final image is the reference's own update expression (:121) applied to the last call (t = 1: z = 0)."""
    from osmosis_utils import diffusion as R_diff
    m, _cfg, _sd = rgb_model("c36")
    diff = R_diff.GaussianDiffusion(T=1000, schedule="linear")
    x_T = 0.3 * torch.randn(1, 3, 32, 32, generator=torch.Generator().manual_seed(3))
    xs, preds = [], []

    def net(x, t):
        xs.append(x.detach().clone())
        o = m(x, t)
        preds.append(o.detach()[:, :3].clone())
        return o

    raised = False
    with _DrawLog() as log:
        try:
            diff.inverse(net=net, shape=(3, 32, 32), image_channels=3, steps=6, x=x_T.clone(), start_t=6, device="cpu")
        except UnboundLocalError:
            raised = True
    assert raised and len(log.draws) == 5 and len(xs) == 6
    at, atbar = diff.alpha[0], diff.alphabar[0]
    x, pred = xs[-1], preds[-1]
    x_final = (1 / np.sqrt(at)) * (x - ((1 - at) / np.sqrt(1 - atbar)) * pred)
    x_start = (1 / np.sqrt(atbar)) * (x - (np.sqrt(1 - atbar) * pred))
    out["prior.x_T"], out["prior.noise"] = npy(x_T), np.stack([npy(d) for d in log.draws])
    out["prior.x_steps"] = np.stack([npy(v) for v in xs])
    out["prior.x_final"] = npy(x_final)
    out["prior.x_start_rgb"] = npy(torch.clamp(0.5 * (x_start.squeeze() + 1)[0:3], 0, 1))
    print("prior", "max |x_final|", float(x_final.abs().max()))


def main():
    path = sys.argv[1] if len(sys.argv) > 1 else OUT
    out = {}
    gen_unets(out)
    gen_chains(out)
    gen_prior(out)
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path))


if __name__ == "__main__":
    main()
