"""The oracle of the robust data term (include/osmosis_robust.h; the reference has no such term, the header is the contract), written
from the definitions in numpy / torch float64:

    e = y - P;  valid = M0 > 0 and e finite;  sigma = max(1.4826 * med2(|e| over valid), sigma_min);  u = |e| / (c sigma);
    omega = huber / tukey / cauchy (u);  M_eff = M0 sqrt(omega)

and its composition with the masked guidance oracle (tests/physgroup_oracle.py): the data term with M_eff in the mask's place, M_eff
computed ONCE per sub-step from the phi the sub-step starts from.  `sigma32` is the float32 restatement of the scale (numpy sort,
every operation one fp32 rounding) that the select kernel is held to bit for bit.
Shared by tests/test_robust_cpu.py and tests/test_robust_gpu.py."""
import numpy as np
import torch

from oracle import diffusion_ref as D
import physgroup_oracle as GO

LOSSES = ("huber", "tukey", "cauchy")
C_DEFAULT = {"huber": 1.345, "tukey": 4.685, "cauchy": 2.385}
SIGMA_MIN = 2.0 / 255.0


def median2(a):
    """The two-rank median of a 1-D array: the mean of the order statistics of rank (n - 1) >> 1 and n >> 1."""
    a = np.sort(np.asarray(a))
    n = a.size
    return 0.5 * (a[(n - 1) >> 1] + a[n >> 1])


def omega_of(u, loss):
    """(omega, sqrt(omega)) of the normalised residual u >= 0, float64."""
    u = np.asarray(u, dtype=np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if loss == "huber":
            w = np.where(u <= 1.0, 1.0, 1.0 / np.where(u <= 1.0, 1.0, u))
            return w, np.sqrt(w)
        if loss == "tukey":
            s = np.where(u < 1.0, 1.0 - u * u, 0.0)
            return s * s, s
        if loss == "cauchy":
            w = 1.0 / (1.0 + u * u)
            return w, np.sqrt(w)
    raise ValueError(loss)


def valid_of(e, M0):
    e = np.asarray(e)
    return np.isfinite(e) & (np.ones(e.shape, bool) if M0 is None else np.asarray(M0) > 0)


def sigma32(e, M0, sigma_min=SIGMA_MIN):
    """(sigma [B] float32, n [B] int) from fp32 e [B,3,hw] and M0 (or None): the contract restated in float32."""
    e = np.asarray(e, dtype=np.float32)
    B = e.shape[0]
    v = valid_of(e, M0)
    sig, n = np.empty(B, np.float32), np.empty(B, np.int64)
    for b in range(B):
        a = np.sort(np.abs(e[b][v[b]]))
        n[b] = a.size
        if a.size == 0:
            sig[b] = np.float32(np.nan)
            continue
        with np.errstate(over="ignore"):
            med = np.float32(0.5) * np.float32(a[(a.size - 1) >> 1] + a[a.size >> 1])
            sig[b] = max(np.float32(1.4826) * med, np.float32(sigma_min))
    return sig, n


def sigma64(e, M0, sigma_min=SIGMA_MIN):
    e = np.asarray(e, dtype=np.float64)
    v = valid_of(e, M0)
    return np.array([max(1.4826 * median2(np.abs(e[b][v[b]])), sigma_min) if v[b].any() else np.nan for b in range(e.shape[0])])


def weights64(e, M0, sigma, loss, c=None, per_pixel=False):
    """(M_eff, omega) float64 [B,3,hw] from e, M0 (None: ones) and sigma [B]."""
    e = np.asarray(e, dtype=np.float64)
    B = e.shape[0]
    m0 = np.ones(e.shape) if M0 is None else np.asarray(M0, dtype=np.float64)
    c = C_DEFAULT[loss] if c is None else float(c)
    sigma = np.asarray(sigma, dtype=np.float64).reshape(B, *([1] * (e.ndim - 1)))
    ok = valid_of(e, M0) & ~np.isnan(sigma)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        a = np.abs(e)
        u = np.where(a == 0, 0.0, a / (c * sigma))
    if per_pixel:
        u = np.broadcast_to(np.where(ok, u, 0.0).max(axis=1, keepdims=True), e.shape)
    w, s = omega_of(np.where(ok, u, 0.0), loss)
    return np.where(ok, m0 * s, m0), np.where(ok, w, 1.0)


def mask64(e, M0, loss, c=None, scale="mad", sigma_min=SIGMA_MIN, per_pixel=False):
    """(M_eff, omega, sigma) in float64 from the residual alone."""
    sigma = sigma64(e, M0, sigma_min) if isinstance(scale, str) else np.full(np.asarray(e).shape[0], float(scale))
    return weights64(e, M0, sigma, loss, c, per_pixel) + (sigma,)


# ----------------------------------------------------------------------------- composition with the masked guidance oracle
def robust_mask_of(opname, okw, x0, y, mask, robust, phi=None, fp32_e=False):
    """M_eff [n,3,H,W] (float64 torch), omega and sigma for images x0 [n,4,H,W], y [n,3,H,W] (float64) at the operator's starting
    phi (`okw`, or `phi`: {name: [1 or n,k,1,1]}).  fp32_e: the residual formed in float32 from float32 operands, as the kernels form
    it (the oracle's own float64-versus-float32 distance)."""
    op = D.PhysOperator(opname, batch_size=1, **okw)
    if phi is not None:
        for k in op.phi:
            op.phi[k] = phi[k].detach().clone()
    with torch.no_grad():
        if fp32_e:
            I = op.forward(x0.float()).float()
            e = (y.float() - (2 * I - 1)).double()
        else:
            I = op.forward(x0.double())
            e = y.double() - (2 * I - 1)
    n, _, H, W = y.shape
    m0 = None if mask is None else np.broadcast_to(mask.double().numpy(), (n, 3, H, W)).reshape(n, 3, H * W)
    meff, om, sigma = mask64(e.numpy().reshape(n, 3, H * W), m0, **robust)
    return torch.from_numpy(meff.reshape(n, 3, H, W).copy()), torch.from_numpy(om.reshape(n, 3, H, W).copy()), sigma


def inner_loop(group_sizes, opname, okw, x0, y, mask, n_iter, optimizer, aux, loss_function, loss_weight, reduce, robust, fp32_e=False):
    """The guided sub-step's data term over a batch of contiguous groups with the robust weights (robust None: the masked oracle as
    it is).  Returns (loss [B], {phi: [B,k,1,1]}, g [B,4,H,W], omega [B,3,H,W] or None, sigma [B] or None)."""
    seps, phis, gs, oms, sigs, lo = [], [], [], [], [], 0
    for n in group_sizes:
        sl = slice(lo, lo + n)
        m = None if mask is None else (mask if mask.shape[0] == 1 else mask[sl])
        if robust is not None:
            m, om, sg = robust_mask_of(opname, okw, x0[sl], y[sl], m, robust, fp32_e=fp32_e)
            oms.append(om)
            sigs.append(sg)
        sep, phi, g = GO.group_inner_loop(opname, okw, None, x0[sl], y[sl], m, n_iter, optimizer, aux, loss_function, loss_weight, reduce)
        seps.append(sep)
        phis.append({k: v.expand(n, *v.shape[1:]) for k, v in phi.items()})
        gs.append(g)
        lo += n
    return (np.concatenate(seps), {k: torch.cat([p[k] for p in phis]) for k in phis[0]}, torch.cat(gs),
            torch.cat(oms) if oms else None, np.concatenate(sigs) if sigs else None)


class RobustGuidance(GO.GroupGuidance):
    """The grouped (masked) guidance with the robust weights: `conditioning` computes M_eff from the phi it starts with and runs the
    masked step with it.  base_mask: M0 or None; robust: dict(loss, c, scale, sigma_min, per_pixel) or None."""
    base_mask = None
    robust = None
    last = None         # (omega, sigma) of the last sub-step

    def conditioning(self, x_prev, x_t, x_0_hat, y, freeze_phi):
        if self.robust is None:
            self.mask = self.base_mask
        else:
            n, _, H, W = y.shape
            with torch.no_grad():
                e = (y.double() - (2 * self.op.forward(x_0_hat.detach().double()) - 1)).numpy().reshape(n, 3, H * W)
            m0 = None if self.base_mask is None else np.broadcast_to(self.base_mask.double().numpy(), (n, 3, H, W)).reshape(n, 3, H * W)
            meff, om, sigma = mask64(e, m0, **self.robust)
            self.mask = torch.from_numpy(meff.reshape(n, 3, H, W).copy()).to(x_0_hat.dtype)
            self.last = (torch.from_numpy(om.reshape(n, 3, H, W).copy()), sigma)
        return super().conditioning(x_prev, x_t, x_0_hat, y, freeze_phi)


def make_guidance(opname, okw, mask, n_iter, aux, loss_function, loss_weight, robust, reduce="mean", optimizer=None, scale="7,7,7,0.9",
                  gradient_clip="False,0"):
    op = D.PhysOperator(opname, batch_size=1, optimizer=optimizer, **okw)
    guide = RobustGuidance(op, n_iter=n_iter, scale=scale, gradient_clip=gradient_clip, aux=aux, loss_function=loss_function,
                           loss_weight=loss_weight)
    guide.A, guide.base_mask, guide.mask, guide.reduce, guide.robust = None, mask, mask, reduce, robust
    return guide


# ----------------------------------------------------------------------------- the effect: phi under outliers
PHI_TRUE = dict(phi_a="1.2,0.6,0.4", phi_b="1.0,0.7,0.5", phi_inf="0.1,0.5,0.6")
PHI_START = dict(phi_a="0.8,0.8,0.8", phi_b="0.8,0.8,0.8", phi_inf="0.3,0.3,0.3")
OPNAME = "underwater_physical_revised"


def effect_problem(seed=0, H=36, W=34, frac=0.05, noise=0.02):
    """x0 [1,4,H,W] float64 held at the truth (J ~ U(0.1, 0.9), d ~ U(0.2, 1.5) under the 'move' conversion with value 0) and
    y = 2 I(phi*) - 1 + N(0, noise) with `frac` of the pixels replaced on all channels by U(0.6, 1.0); the outlier map [1,1,H,W]."""
    g = torch.Generator().manual_seed(seed)
    J = 0.1 + 0.8 * torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    d = 0.2 + 1.3 * torch.rand(1, 1, H, W, generator=g, dtype=torch.float64)
    x0 = torch.cat([2 * J - 1, d], dim=1)
    op = D.PhysOperator(OPNAME, batch_size=1, depth_type="move", value=0.0, **PHI_TRUE)
    y = 2 * op.forward(x0) - 1 + noise * torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
    out = torch.rand(1, 1, H, W, generator=g, dtype=torch.float64) < frac
    y = torch.where(out, 0.6 + 0.4 * torch.rand(1, 3, H, W, generator=g, dtype=torch.float64), y)
    return x0, y, out


def phi_true():
    return {k: torch.tensor([float(s) for s in v.split(",")], dtype=torch.float64) for k, v in PHI_TRUE.items()}


def effect_fit(x0, y, robust, steps, n_iter=20, eta=0.02, trace=None, fp32_e=False, fp32_phi=False):
    """`steps` sub-steps of n_iter sgd iterations on phi from PHI_START, the image held at x0, loss norm, no weight: returns
    ({phi: [3]}, omega of the last sub-step or None, sigma or None).  trace: a list that receives phi after every sub-step.
    fp32_e: the weights' residual formed in float32 (the image rounded to float32, then 2 I - 1 and y - P in float32).
    fp32_phi: phi rounded to float32 after every step, as a float32 parameter tensor holds it (the reference's, and the kernels')."""
    okw = dict(PHI_START, depth_type="move", value=0.0, **{k + "_eta": eta for k in PHI_START})
    op = D.PhysOperator(OPNAME, batch_size=1, **okw)
    for k in op.phi:
        op.phi[k] = op.phi[k].double()
    guide = GO.GroupGuidance(op, n_iter=n_iter, scale="1", gradient_clip="False,0", aux=None, loss_function="norm", loss_weight="none")
    guide.A, guide.mask, guide.reduce = None, None, "mean"
    om = sigma = None
    for _ in range(steps):
        if robust is not None:
            with torch.no_grad():
                if fp32_e:
                    e = (y.float() - (2 * op.forward(x0).float() - 1)).double().numpy().reshape(1, 3, -1)
                else:
                    e = (y - (2 * op.forward(x0) - 1)).numpy().reshape(1, 3, -1)
            meff, om, sigma = mask64(e, None, **robust)
            guide.mask = torch.from_numpy(meff.reshape(y.shape).copy())
        op.set_requires_grad(True)
        for _it in range(n_iter):
            _, loss = guide.loss(x0, y)
            loss.backward(inputs=list(op.phi.values()))
            guide.step(1)
            if fp32_phi:
                with torch.no_grad():
                    for v in op.phi.values():
                        v.copy_(v.float().double())
        op.set_requires_grad(False)
        if trace is not None:
            trace.append({k: v.detach().reshape(-1).clone() for k, v in op.phi.items()})
    return {k: v.detach().reshape(-1).clone() for k, v in op.phi.items()}, om, sigma


def effect_fit_closed_form(x0, y, robust, steps, n_iter=20, eta=1e-3, trace=None, fp32_phi=False):
    """`effect_fit` with the gradient of the norm loss written out (numpy float64, no autograd), for runs of thousands of sub-steps:
    I_c = J_c exp(-a_c d) + inf_c (1 - exp(-b_c d)), r = M (y - (2 I - 1)), L = ||r||, dL/dtheta_c = sum_p (-2 M r / L) dI/dtheta_c.
    tests/test_robust_cpu.py holds it to `effect_fit` (torch autograd over the oracle's operator).  Returns the same triple; `trace`
    receives max |phi - phi*| after every sub-step; fp32_phi as in `effect_fit`."""
    J = (0.5 * (x0[0, 0:3].double() + 1)).numpy().reshape(3, -1)
    d = x0[0, 3].double().numpy().reshape(1, -1)
    yy = y[0].double().numpy().reshape(3, -1)
    a, b, inf = (np.array([float(s) for s in PHI_START[k].split(",")])[:, None] for k in ("phi_a", "phi_b", "phi_inf"))
    true = np.concatenate([phi_true()[k].numpy() for k in ("phi_a", "phi_b", "phi_inf")])
    M = np.ones_like(yy)
    om = sigma = None
    for _ in range(steps):
        if robust is not None:
            ea, eb = np.exp(-a * d), np.exp(-b * d)
            e = yy - (2 * (J * ea + inf * (1 - eb)) - 1)
            meff, om, sigma = mask64(e[None], None, **robust)
            M = meff[0]
        for _it in range(n_iter):
            ea, eb = np.exp(-a * d), np.exp(-b * d)
            r = M * (yy - (2 * (J * ea + inf * (1 - eb)) - 1))
            gI = -2.0 * M * r / np.sqrt((r * r).sum())
            ga = (gI * (-d * J * ea)).sum(axis=1, keepdims=True)
            gb = (gI * (inf * d * eb)).sum(axis=1, keepdims=True)
            gi = (gI * (1 - eb)).sum(axis=1, keepdims=True)
            a, b, inf = a - eta * ga, b - eta * gb, inf - eta * gi
            if fp32_phi:
                a, b, inf = (v.astype(np.float32).astype(np.float64) for v in (a, b, inf))
        if trace is not None:
            trace.append(float(np.abs(np.concatenate([a, b, inf])[:, 0] - true).max()))
    phi = {k: torch.from_numpy(v[:, 0].copy()) for k, v in (("phi_a", a), ("phi_b", b), ("phi_inf", inf))}
    return phi, om, sigma


def phi_error(phi):
    t = phi_true()
    return max(float((phi[k].double() - t[k]).abs().max()) for k in t)
