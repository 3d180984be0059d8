"""CPU oracle of the few-step solvers (TEST INFRASTRUCTURE): the step rules of include/osmosis_solver.h restated in numpy float64
from the oracle's own tables, and the oracle's sampling loops with them as the step rule -- a loop over the oracle's
`p_mean_variance` and a guidance object's `conditioning` (oracle.diffusion_ref.OsmosisGuidance or a subclass: masks, the depth
prior, the tiled network), the rule's float64 coefficients applied to the tensors.

Rules, at index i of a (respaced) schedule with ab = alphas_cumprod, ab' = alphas_cumprod_prev, lambda = log(sqrt(ab) / sqrt(1 - ab)):
  ddim      s = eta sqrt((1 - ab') / (1 - ab)) sqrt(1 - ab / ab');  A = sqrt(1 - ab' - s^2) / sqrt(1 - ab);  B0 = sqrt(ab') - A sqrt(ab)
  dpmpp_2m  h = lambda' - lambda;  A = sqrt(1 - ab') / sqrt(1 - ab);  beta = -sqrt(ab') expm1(-h);  r = h_prev / h;
            B0 = beta (1 + 1 / (2 r));  B1 = -beta / (2 r);  first executed index: B0 = beta, B1 = 0
  last index (ab' = 1): x_next = x0
"""
import numpy as np
import torch

from oracle import diffusion_ref as D


def coefs(tb, rule, eta=0.0, first=None):
    """float64 [T][4] = A, B0, B1, S over the oracle's tables `tb`; history is empty at `first` (default T - 1)."""
    ab, abp = np.asarray(tb.alphas_cumprod, dtype=np.float64), np.asarray(tb.alphas_cumprod_prev, dtype=np.float64)
    T = len(ab)
    first = T - 1 if first is None else first
    out = np.zeros((T, 4))
    with np.errstate(divide="ignore", invalid="ignore"):
        lam, lamp = 0.5 * np.log(ab / (1 - ab)), 0.5 * np.log(abp / (1 - abp))
        h = lamp - lam
        if rule == "ddim":
            s = eta * np.sqrt((1 - abp) / (1 - ab)) * np.sqrt(1 - ab / abp)
            out[:, 0] = np.sqrt(1 - abp - s ** 2) / np.sqrt(1 - ab)
            out[:, 1] = np.sqrt(abp) - out[:, 0] * np.sqrt(ab)
            out[:, 3] = s
        elif rule == "dpmpp_2m":
            assert eta == 0.0
            beta = -np.sqrt(abp) * np.expm1(-h)
            r = np.append(h[1:], np.nan) / h                     # h of the index executed before (i + 1) over this one's
            second = np.arange(T) < min(first, T - 1)
            out[:, 0] = np.sqrt(1 - abp) / np.sqrt(1 - ab)
            out[:, 1] = np.where(second, beta * (1 + 1 / (2 * r)), beta)
            out[:, 2] = np.where(second, -beta / (2 * r), 0.0)
        else:
            raise ValueError(rule)
    out[abp == 1.0] = (0.0, 1.0, 0.0, 0.0)
    return out


def gaussian_chain_error(tab, alphas_cumprod, n=64, mu=0.3, s2=0.25, seed=0):
    """The closed-form test bed: data N(mu, s2), exact denoiser mu + alpha s2 / (alpha^2 s2 + sigma^2) (x - alpha mu); the chain of
    rows `tab` from x_T ~ N(0, 1) (n seeded samples) against the probability-flow solution
    mu + sqrt(s2 / (ab_T s2 + 1 - ab_T)) (x_T - sqrt(ab_T) mu).  Max-abs error at the end, float64."""
    ab = np.asarray(alphas_cumprod, dtype=np.float64)
    T = len(ab)
    x_T = np.random.default_rng(seed).standard_normal(n)
    x, hist = x_T.copy(), None
    for i in range(T - 1, -1, -1):
        a, v = np.sqrt(ab[i]), 1.0 - ab[i]
        x0 = mu + a * s2 / (a * a * s2 + v) * (x - a * mu)
        A, B0, B1, S = tab[i]
        assert S == 0.0
        x = A * x + B0 * x0 + (B1 * hist if B1 != 0.0 else 0.0)
        hist = x0
    exact = mu + np.sqrt(s2 / (ab[T - 1] * s2 + 1.0 - ab[T - 1])) * (x_T - np.sqrt(ab[T - 1]) * mu)
    return float(np.abs(x - exact).max())


def _det(row, img, x0, hist):
    A, B0, B1, _ = (float(v) for v in row)
    det = A * img + B0 * x0
    return det + B1 * hist if B1 != 0.0 else det


def osmosis_loop(model, tb, x_T, y, guidance, pattern, noises, rule, eta=0.0, first=None, last=0, trace=None, clip_denoised=False):
    """oracle.diffusion_ref.p_sample_loop with the solver as the step rule: the state handed to `guidance.conditioning` is the
    deterministic part A x + B0 x0 + B1 x0_prev, S noises[k] is added afterwards.  Indices first .. last (history empty at first)."""
    T = tb.num_timesteps
    first = T - 1 if first is None else first
    tab = coefs(tb, rule, eta, first)
    img, hist = x_T.clone(), None
    loss = variables = x0 = None
    for k, idx in enumerate(range(first, last - 1, -1)):
        img = img.detach().requires_grad_(True)
        out = D.p_mean_variance(tb, model(img, torch.tensor([tb.timestep_map[idx]] * img.shape[0])), img, idx,
                                clip_denoised=clip_denoised)
        x_t = _det(tab[idx], img, out["pred_xstart"], hist)
        x_t, loss, variables, grad = guidance.conditioning(img, x_t, out["pred_xstart"], y, D.is_freeze_phi(pattern, idx, T))
        x0 = hist = out["pred_xstart"].detach()
        new = x_t.detach()
        if tab[idx, 3] != 0.0:
            new = new + float(tab[idx, 3]) * noises[k]
        if trace is not None:
            trace.append({"x_in": img.detach().clone(), "x0": x0.clone(), "grad": grad, "loss": np.array(loss), "x_out": new.clone(),
                          "phi": {n: v.clone() for n, v in variables.items()}})
        img = new
    return img, variables, loss, x0


def ps_loop(model, tb, x_T, y, scale, noises, rule, eta=0.0, clip_denoised=False, trace=None):
    """The rgb-guidance ('ps') chain on an identity operator with the solver as the step rule: per index the oracle's
    p_mean_variance, sample = A x + B0 x0 + B1 x0_prev + S noises[k], x = sample - scale d ||y - x0[:, 0:3]|| / d x_prev."""
    T = tb.num_timesteps
    tab = coefs(tb, rule, eta)
    img, hist = x_T.clone(), None
    for k, idx in enumerate(range(T - 1, -1, -1)):
        img = img.detach().requires_grad_(True)
        out = D.p_mean_variance(tb, model(img, torch.tensor([tb.timestep_map[idx]] * img.shape[0])), img, idx,
                                clip_denoised=clip_denoised)
        x0 = out["pred_xstart"]
        sample = _det(tab[idx], img, x0, hist).detach()
        if tab[idx, 3] != 0.0:
            sample = sample + float(tab[idx, 3]) * noises[k]
        loss = torch.linalg.norm(y - x0[:, 0:3])
        (grad,) = torch.autograd.grad(loss, img)
        new = sample - scale * grad
        hist = x0.detach()
        if trace is not None:
            trace.append({"x_in": img.detach().clone(), "x0": hist.clone(), "x_out": new.clone(), "loss": float(loss)})
        img = new
    return img.detach()
