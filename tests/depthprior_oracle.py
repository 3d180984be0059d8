"""The oracle of the range-map depth prior (include/osmosis_depthprior.h; the reference has no such term): torch float64 on the CPU.

The term is written from the RESIDUALS e = d - (a z + c), not from the moments the kernels reduce; (a, c) go through the
differentiable closed form `fit`, so the envelope gradient (a, c detached) can be checked against autograd through the solve.
Composes with the oracles of the data term (`oracle.diffusion_ref.OsmosisGuidance` through tests/physgroup_oracle.py, which also
carries tests/physlin_oracle.py's linear operator and the mask) by adding weight * sum_b L_depth[b] to their objective.
Shared by tests/test_depthprior_cpu.py and tests/test_depthprior_gpu.py."""
import numpy as np
import torch

from oracle import diffusion_ref as D
import physgroup_oracle as GO

EPS40 = 2.0 ** -40


def fit(d, z, m, align, scale=1.0, scale_min=1e-3, clamp=True):
    """One image: d, z, m 1-D float64 tensors over the pixels with m > 0.  Returns (a, c) as 0-dim tensors (differentiable w.r.t.
    d), or None where a guard of the contract skips the image."""
    Sm, Sz, Sd = m.sum(), (m * z).sum(), (m * d).sum()
    Szz, Szd = (m * z * z).sum(), (m * z * d).sum()
    if not float(Sm) > 0:
        return None
    if align == "none":
        return torch.as_tensor(float(scale), dtype=d.dtype), torch.zeros((), dtype=d.dtype)
    if align == "scale":
        if not float(Szz) > 0:
            return None
        a = Szd / Szz
        if clamp:
            a = torch.clamp(a, min=scale_min)
        return a, torch.zeros((), dtype=d.dtype)
    assert align == "affine", align
    det = Sm * Szz - Sz * Sz
    if not float(det) > EPS40 * float(Sm * Szz):
        return None
    a = (Sm * Szd - Sz * Sd) / det
    if clamp:
        a = torch.clamp(a, min=scale_min)
    return a, (Sd - a * Sz) / Sm


def term(d, z, m, align, loss, scale=1.0, scale_min=1e-3, envelope=True):
    """d [B,1,H,W] (float64, may require grad), z, m [B,1,H,W].  Returns (L [B] differentiable, info): info[b] = dict(a, c, S, Sdd,
    skipped, nan).  envelope: (a, c) detached (the contract); False: autograd goes through the solve."""
    B = d.shape[0]
    Ls, info = [], []
    for b in range(B):
        on = (m[b] > 0).reshape(-1)
        db, zb, mb = d[b].reshape(-1)[on], z[b].reshape(-1)[on].to(d.dtype), m[b].reshape(-1)[on].to(d.dtype)
        rec = dict(a=float("nan"), c=float("nan"), S=0.0, Sdd=0.0, skipped=True, nan=False)
        if align == "none":
            rec.update(a=float(scale), c=0.0)
        zero = torch.zeros((), dtype=d.dtype)
        if on.any() and not bool(torch.isfinite(db).all() and torch.isfinite(zb).all()):
            rec["nan"] = True
            Ls.append(zero + float("nan"))
            info.append(rec)
            continue
        ac = fit(db, zb, mb, align, scale, scale_min) if on.any() else None
        if ac is None:
            Ls.append(zero)
            info.append(rec)
            continue
        a, c = (ac[0].detach(), ac[1].detach()) if envelope else ac
        e = db - (a * zb + c)
        S = (mb * e * e).sum()
        Sdd = float((mb * db.detach() ** 2).sum())
        rec.update(a=float(a.detach()), c=float(c.detach()), S=float(S.detach()), Sdd=Sdd, skipped=False)
        if loss == "norm":
            L = zero if float(S.detach()) <= EPS40 * Sdd else torch.sqrt(S)
        else:
            assert loss == "mse", loss
            L = S / mb.sum()
        Ls.append(L)
        info.append(rec)
    return torch.stack(Ls), info


def conv_depth(D_, depth_type, value):
    """The operator's depth conversion (oracle.diffusion_ref.convert_depth on its parsed value)."""
    return D.convert_depth(D_, depth_type, D.parse_value(value))


def term_and_increment(x0, z, m, prior, depth_type, value, d_override=None):
    """What the kernels add, in float64: (L [B], inc [B,1,H,W] = weight * d sum_b L_b / d x0[:, 3:4], info).  d_override: a
    function D -> d (e.g. the fp32 conversion the kernels evaluate, carried through autograd by its float64 derivative)."""
    Dp = x0[:, 3:4].detach().to(torch.float64).clone().requires_grad_(True)
    d = conv_depth(Dp, depth_type, value) if d_override is None else d_override(Dp)
    L, info = term(d, z.to(torch.float64), m.to(torch.float64), prior["align"], prior["loss"], prior.get("scale", 1.0),
                   prior.get("scale_min", 1e-3))
    live = torch.isfinite(L.detach())
    tot = (prior["weight"] * torch.where(live, L, torch.zeros_like(L))).sum()
    inc = torch.autograd.grad(tot, Dp, allow_unused=True)[0] if tot.requires_grad else None
    inc = torch.zeros_like(Dp) if inc is None else inc
    return L.detach(), inc * (m > 0), info


class Fp32Depth(torch.autograd.Function):
    """d = the conversion evaluated in fp32 on the fp32 D (the kernels' operand, bit for bit for original / move), with the
    float64 derivative of the same formula: feeds the oracle the IDENTICAL d."""
    @staticmethod
    def forward(ctx, Dp, depth_type, value):
        v = D.parse_value(value)
        D32 = Dp.to(torch.float32)
        if depth_type == "move":
            d32, dd = D32 + np.float32(v), torch.ones_like(Dp)
        elif depth_type in (None, "original"):
            d32, dd = np.float32(0.5) * (D32 + np.float32(1.0)), torch.full_like(Dp, 0.5)
        else:
            raise NotImplementedError(depth_type)
        ctx.save_for_backward(dd)
        return d32.to(torch.float64)

    @staticmethod
    def backward(ctx, g):
        return g * ctx.saved_tensors[0], None, None


# ----------------------------------------------------------------------------- composition with the data term's oracles
class _Prior:
    prior = None        # dict(z [n,1,H,W], m [n,1,H,W], weight, align, loss, scale, scale_min); None: no prior
    depth_last = None   # (L [n], info) of the last evaluation

    def loss(self, x0, y):
        sep, total = super().loss(x0, y)
        p = self.prior
        if p is None:
            return sep, total
        d = D.convert_depth(x0[:, 3:4].to(torch.float64), self.op.depth_type, self.op.value)
        L, info = term(d, p["z"].to(torch.float64), p["m"].to(torch.float64), p["align"], p["loss"], p.get("scale", 1.0),
                       p.get("scale_min", 1e-3))
        self.depth_last = (L.detach().clone(), info)
        live = torch.isfinite(L.detach())
        return sep, total + (p["weight"] * torch.where(live, L, torch.zeros_like(L))).sum()


class PriorGuidance(_Prior, GO.GroupGuidance):
    pass


class PriorLinGuidance(_Prior, GO.GroupLinGuidance):
    pass


def make_guidance(opname, okw, deg, H, W, mask, n_iter, aux, loss_function, loss_weight, prior, reduce="mean", optimizer=None,
                  scale="7,7,7,0.9", gradient_clip="False,0"):
    """tests/physgroup_oracle.make_guidance with the prior in the objective: ONE group (one image is a group of one)."""
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    op = D.PhysOperator(opname, batch_size=1, optimizer=optimizer, **okw)
    cls = PriorGuidance if deg is None else PriorLinGuidance
    guide = cls(op, n_iter=n_iter, scale=scale, gradient_clip=gradient_clip, aux=aux, loss_function=loss_function, loss_weight=loss_weight)
    guide.A = None if deg is None else (GO.dense_operator(deg, H, W) if isinstance(deg, M.GRID_OPERATORS) else deg)
    guide.mask, guide.reduce, guide.prior = mask, reduce, prior
    return guide


def rows(prior, lo, hi):
    """The prior of the images lo .. hi - 1 of a batch."""
    if prior is None:
        return None
    return dict(prior, z=prior["z"][lo:hi], m=prior["m"][lo:hi])


def inner_loop(group_sizes, opname, okw, deg, x0, y, mask, n_iter, aux, loss_function, loss_weight, prior, reduce="mean"):
    """The guided sub-step's data term with the prior over a batch of contiguous groups (all ones: independent images), float64:
    n_iter x (total, backward, phi step), the last backward also into x0.  Returns (data loss [B], {phi: [B,k,1,1]}, g [B,4,H,W],
    depth loss [B], [info])."""
    seps, phis, gs, Ld, infos, lo = [], [], [], [], [], 0
    for n in group_sizes:
        mk = None if mask is None else (mask if mask.shape[0] == 1 else mask[lo:lo + n])
        guide = make_guidance(opname, okw, deg, x0.shape[-2], x0.shape[-1], mk, n_iter, aux, loss_function, loss_weight,
                              rows(prior, lo, lo + n), reduce)
        op = guide.op
        xb = x0[lo:lo + n].clone().requires_grad_(True)
        op.set_requires_grad(True)
        for it in range(n_iter):
            sep, loss = guide.loss(xb, y[lo:lo + n])
            a = guide.group_aux(xb)
            total = loss if a is None else loss + a
            total.backward(inputs=([xb] if it == n_iter - 1 else []) + list(op.phi.values()))
            guide.step(n)
        seps.append(np.asarray(sep, dtype=np.float64))
        phis.append({k: p.detach().clone().expand(n, *p.shape[1:]) for k, p in op.phi.items()})
        gs.append(xb.grad.detach().clone())
        if guide.depth_last is not None:
            Ld.append(guide.depth_last[0])
            infos += guide.depth_last[1]
        lo += n
    return (np.concatenate(seps), {k: torch.cat([p[k] for p in phis]) for k in phis[0]}, torch.cat(gs),
            torch.cat(Ld) if Ld else None, infos)


def problem(B, H, W, seed, frac=1.0, fractional=False, a=0.8, c=0.15, noise=0.08):
    """Inputs whose oracle cancellation factor S_dd / S stays small: x0 [B,4,H,W] fp32, z [B,1,H,W] with the depth plane roughly
    a z + c plus `noise`, m in {0, 1} (or fractional confidences) on about `frac` of the pixels, NaN in z wherever m = 0."""
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g)).clamp(-1.0, 1.0)
    z = torch.rand(B, 1, H, W, generator=g) * 4.0 + 0.5
    d = a * z / 4.5 + c + noise * torch.randn(B, 1, H, W, generator=g)
    x0[:, 3:4] = (2.0 * d - 1.0).clamp(-0.95, 0.95)
    m = (torch.rand(B, 1, H, W, generator=g) < frac).to(torch.float32)
    if fractional:
        m = m * (0.1 + 0.9 * torch.rand(B, 1, H, W, generator=g))
    z = torch.where(m > 0, z, torch.full_like(z, float("nan")))
    return x0.contiguous(), z.contiguous(), m.contiguous()
