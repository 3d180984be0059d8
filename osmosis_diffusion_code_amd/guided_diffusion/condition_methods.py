"""Conditioning (guidance) methods -- registry surface of the reference's
guided_diffusion/condition_methods.py (register/get_conditioning_method :11-24).

`PosteriorSamplingOsmosis` ('osmosis', reference :61-231) is re-designed around three fused HIP
kernels (csrc/guidance.hip):
    osm_phys_reduce    forward model + weighted residual + all per-image reductions   (:109-144)
    osm_phys_finalize  loss value, dL/dphi, in-place SGD on phi                        (:185-197)
    osm_phys_grad      analytic dL/dx0 (data term + auxiliary losses)                  (:176-194)
so the n_iter(=20) inner phi-optimisation runs back-to-back on the device with no host sync (the
reference copies the residual to the host every inner iteration, :130).  Reductions are per image,
which equals the reference at its only working batch size (1) and defines B>1 as independent images.

Two ways in:
  * `loss_grad_x0(x0, y, freeze_phi)` -- used by the fused sampler step
    (gaussian_diffusion.GaussianDiffusion.p_sample_loop fast path);
  * `conditioning(x_prev=, x_t=, x_0_hat=, measurement=, ...)` -- the reference signature and
    5-tuple; works with any autograd graph from x_prev to x_0_hat (our UNet is an autograd.Function).
"""
from abc import ABC, abstractmethod
from functools import partial
from operator import index

import os
import numpy as np
import torch

from .. import ops
from .._lib import PhysDesc
from ..osmosis_utils import losses as losseso
from ..osmosis_utils import utils as utilso

__CONDITIONING_METHOD__ = {}


def register_conditioning_method(name: str):
    def wrapper(cls):
        if __CONDITIONING_METHOD__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __CONDITIONING_METHOD__[name] = cls
        return cls
    return wrapper


def get_conditioning_method(name: str, operator, noiser, **kwargs):
    if __CONDITIONING_METHOD__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined!")
    return __CONDITIONING_METHOD__[name](operator=operator, noiser=noiser, **kwargs)


def _parse_scale(s):
    try:
        return torch.tensor([float(s)])
    except ValueError:
        return torch.tensor([float(p.strip()) for p in s.split(",")])


def validate_measurement_mask(mask, batch=None):
    """A validity mask of the measurement as fp32 [B or 1, 3, H, W]: rank 4, [B,3,H,W] / [B,1,H,W] / [1,3,H,W] / [1,1,H,W],
    finite, within [0, 1] (0 ignore, 1 trust fully, fractions are confidences).  batch: the chain's batch size, when known."""
    mask = torch.as_tensor(mask)
    if mask.dim() != 4:
        raise ValueError(f"measurement mask must have rank 4 ([B,3,H,W], [B,1,H,W], [1,3,H,W] or [1,1,H,W]), got {tuple(mask.shape)}")
    if mask.shape[1] not in (1, 3):
        raise ValueError(f"measurement mask must have 1 or 3 channels, got {tuple(mask.shape)}")
    if batch is not None and mask.shape[0] not in (1, int(batch)):
        raise ValueError(f"measurement mask has batch {mask.shape[0]}, the chain has {int(batch)} images (1 broadcasts)")
    mask = mask.detach().to(torch.float32)
    if not bool(torch.isfinite(mask).all()):
        raise ValueError("measurement mask must be finite")
    if mask.numel() and (float(mask.min()) < 0.0 or float(mask.max()) > 1.0):
        raise ValueError(f"measurement mask must lie within [0, 1], got [{float(mask.min())}, {float(mask.max())}]")
    return mask


DEPTH_ALIGNS = ("none", "scale", "affine")
DEPTH_LOSSES = ("norm", "mse")


def validate_depth_prior(z, confidence=None, batch=None):
    """A range map and its confidence as fp32 [B or 1, 1, H, W] each.  z: [B,1,H,W], [1,1,H,W] or [B,H,W], any unit; confidence: the
    same shape within [0, 1] (None: 1 wherever the range is valid).  A range that is not finite or <= 0 is invalid: m = 0 and z = 0
    there."""
    z = torch.as_tensor(z)
    if z.dim() == 3:
        z = z[:, None]
    if z.dim() != 4 or z.shape[1] != 1:
        raise ValueError(f"depth prior must be [B,1,H,W], [1,1,H,W] or [B,H,W], got {tuple(z.shape)}")
    if batch is not None and z.shape[0] not in (1, int(batch)):
        raise ValueError(f"depth prior has batch {z.shape[0]}, the chain has {int(batch)} images (1 broadcasts)")
    z = z.detach().to(torch.float32)
    valid = torch.isfinite(z) & (z > 0)
    if confidence is None:
        m = valid.to(torch.float32)
    else:
        m = torch.as_tensor(confidence)
        if m.dim() == 3:
            m = m[:, None]
        if tuple(m.shape) != tuple(z.shape):
            raise ValueError(f"depth confidence {tuple(m.shape)} must have the shape of the depth prior {tuple(z.shape)}")
        m = m.detach().to(torch.float32)
        if not bool(torch.isfinite(m).all()):
            raise ValueError("depth confidence must be finite")
        if m.numel() and (float(m.min()) < 0.0 or float(m.max()) > 1.0):
            raise ValueError(f"depth confidence must lie within [0, 1], got [{float(m.min())}, {float(m.max())}]")
        m = torch.where(valid.to(m.device), m, torch.zeros_like(m))
    z = torch.where(m > 0, z, torch.zeros_like(z))
    return z, m


def depth_prior_fit(d, z, m, align, scale=1.0, scale_min=1e-3):
    """The closed-form fit d ~ a z + c of include/osmosis_depthprior.h on torch tensors [B,1,H,W] (any float dtype): (a [B], c [B],
    ok [B] bool -- False where a guard skips the image, finite [B] bool -- False where a moment is not finite).  Differentiable;
    callers that want the step's constants detach."""
    dims = (1, 2, 3)
    on = m > 0
    z = torch.where(on, z, torch.zeros_like(z))
    d0 = torch.where(on, d, torch.zeros_like(d))
    Sm, Sz, Sd = m.sum(dims), (m * z).sum(dims), (m * d0).sum(dims)
    Szz, Szd = (m * z * z).sum(dims), (m * z * d0).sum(dims)
    finite = torch.isfinite(Sm + Sz + Sd + Szz + Szd + (m * d0 * d0).sum(dims))
    ok = (Sm > 0) & finite
    one = torch.ones_like(Sm)
    if align == "none":
        return scale * one, 0 * one, ok, finite
    if align == "scale":
        ok = ok & (Szz > 0)
        a = torch.clamp(Szd / torch.where(ok, Szz, one), min=scale_min)
        return a, 0 * one, ok, finite
    if align != "affine":
        raise ValueError(f"depth prior: align must be one of {DEPTH_ALIGNS}, got {align!r}")
    det = Sm * Szz - Sz * Sz
    ok = ok & (det > 2.0 ** -40 * Sm * Szz)
    a = torch.clamp((Sm * Szd - Sz * Sd) / torch.where(ok, det, one), min=scale_min)
    return a, (Sd - a * Sz) / torch.where(ok, Sm, one), ok, finite


def depth_prior_term(d, z, m, align, loss, scale=1.0, scale_min=1e-3):
    """(L [B], reported L [B], a [B], c [B]) of the range-map prior on torch tensors; L is differentiable w.r.t. d with (a, c) as
    constants of the step (they minimise the residual, so this IS the gradient: the envelope theorem).  A guarded image has L = 0
    and no gradient; the REPORTED loss of an image with a non-finite moment is NaN, as the kernels report it (it stays out of L, so
    the data term's gradient survives)."""
    a, c, ok, finite = depth_prior_fit(d.detach(), z, m, align, scale, scale_min)
    a, c = a.detach(), c.detach()
    on = (m > 0) & ok[:, None, None, None]
    e = torch.where(on, d - (a[:, None, None, None] * z + c[:, None, None, None]), torch.zeros_like(d))
    S = (m * e * e).sum((1, 2, 3))
    if loss == "norm":
        Sdd = torch.where(on, m * d.detach() ** 2, torch.zeros_like(d)).sum((1, 2, 3))
        live = S.detach() > 2.0 ** -40 * Sdd
        L = torch.where(live, torch.sqrt(torch.where(live, S, torch.ones_like(S))), torch.zeros_like(S))
    elif loss == "mse":
        L = S / torch.where(ok, m.sum((1, 2, 3)), torch.ones_like(S))
    else:
        raise ValueError(f"depth prior: loss must be one of {DEPTH_LOSSES}, got {loss!r}")
    nan = torch.full_like(a, float("nan"))
    return (L, torch.where(finite, L.detach(), nan), (a if align == "none" else torch.where(ok, a, nan)),
            (c if align == "none" else torch.where(ok, c, nan)))


ROBUST_LOSSES = ("huber", "tukey", "cauchy")


def robust_weights_torch(e, M0, loss, c, scale="mad", sigma_min=2.0 / 255.0, per_pixel=False):
    """include/osmosis_robust.h on torch tensors, in e's dtype: e [B,3,...] the raw residual, M0 of its shape or None (ones) ->
    (M_eff like e, omega like e, sigma [B], n_valid [B] int64), all constants of the step (nothing is differentiated through them).
    The two-rank median by torch.sort over the valid entries (M0 > 0 and e finite)."""
    e = e.detach()
    B = e.shape[0]
    ef = e.reshape(B, -1)
    m0 = torch.ones_like(ef) if M0 is None else M0.detach().to(e.dtype).expand(e.shape).reshape(B, -1)
    a = ef.abs()
    valid = (m0 > 0) & torch.isfinite(ef)
    n = valid.sum(dim=1)
    if isinstance(scale, str):
        srt = torch.sort(torch.where(valid, a, torch.full_like(a, float("inf"))), dim=1).values      # the valid entries come first
        nn = n.clamp(min=1)
        lo, hi = srt.gather(1, ((nn - 1) >> 1)[:, None])[:, 0], srt.gather(1, (nn >> 1)[:, None])[:, 0]
        sigma = torch.clamp(1.4826 * (0.5 * (lo + hi)), min=float(sigma_min))
        sigma = torch.where(n > 0, sigma, torch.full_like(sigma, float("nan")))
    else:
        sigma = torch.full((B,), float(scale), device=e.device, dtype=e.dtype)
    u = torch.where(a == 0, torch.zeros_like(a), a / (float(c) * sigma)[:, None])
    ok = valid & ~torch.isnan(sigma)[:, None]
    if per_pixel:
        u3 = torch.where(ok, u, torch.zeros_like(u)).view(B, 3, -1)
        u = u3.amax(dim=1, keepdim=True).expand(B, 3, u3.shape[2]).reshape(B, -1)
    one = torch.ones_like(u)
    if loss == "huber":
        w = torch.where(u <= 1, one, 1.0 / torch.where(u <= 1, one, u))
        s = torch.sqrt(w)
    elif loss == "tukey":
        s = torch.where(u < 1, 1.0 - u * u, torch.zeros_like(u))
        w = s * s
    elif loss == "cauchy":
        w = 1.0 / (1.0 + u * u)
        s = torch.sqrt(w)
    else:
        raise ValueError(f"robust: loss must be one of {ROBUST_LOSSES}, got {loss!r}")
    return (torch.where(ok, m0 * s, m0).view(e.shape), torch.where(ok, w, one).view(e.shape), sigma, n)


def gain_hats(H, W, gh, gw, device, dtype=torch.float64):
    """The hat matrices (Hy [H,gh], Hx [W,gw]) of include/osmosis_gain.h from the fp32 tables: G = Hy n Hx^T."""
    iy0, fy, ix0, fx = (torch.from_numpy(a) for a in ops.gain_tables_host(H, W, gh, gw))

    def hat(i0, f, g):
        n = i0.shape[0]
        Hm = torch.zeros(n, g, dtype=torch.float64)
        rows = torch.arange(n)
        Hm[rows, i0.long()] += 1.0 - f.double()
        Hm[rows, i0.long() + 1] += f.double()
        return Hm.to(device=device, dtype=dtype)
    return hat(iy0, fy, gh), hat(ix0, fx, gw)


def gain_learn_torch(nodes, F, w, y, M0, loss_function, eta, n_iter, smooth, g_min):
    """include/osmosis_gain.h's n_iter x (node gradient, step) on torch tensors, in float64 whatever the inputs are: nodes
    [B,gh,gw], F and y [B,3,H,W], w [B,1,H,W] or a number, M0 like y or None.  Returns the new nodes (float64); constants of the
    sub-step, nothing is differentiated through them."""
    n = nodes.detach().double().clone()
    F, y = F.detach().double(), y.detach().double()
    B, _, H, W = y.shape
    w = w.detach().double() if torch.is_tensor(w) else float(w)
    M = 1.0 if M0 is None else M0.detach().double()
    Hy, Hx = gain_hats(H, W, n.shape[1], n.shape[2], y.device)
    for _ in range(int(n_iter)):
        G = (Hy @ n @ Hx.T)[:, None]
        r = (y - (2 * G * F - 1)) * w * M
        q = (r * (-2 * F * w * M)).sum(dim=1)
        S = (r * r).sum(dim=(1, 2, 3))
        c_raw = Hy.T @ q @ Hx
        gscale = 1.0 / torch.sqrt(S) if loss_function == "norm" else torch.full_like(S, 2.0 / (3 * H * W))
        Ln = torch.zeros_like(n)
        Ln[:, 1:, :] += n[:, 1:, :] - n[:, :-1, :]
        Ln[:, :-1, :] += n[:, :-1, :] - n[:, 1:, :]
        Ln[:, :, 1:] += n[:, :, 1:] - n[:, :, :-1]
        Ln[:, :, :-1] += n[:, :, :-1] - n[:, :, 1:]
        v = n - float(eta) * (gscale[:, None, None] * c_raw + float(smooth) * Ln)
        gm = torch.full_like(v, float(g_min))
        u = torch.where(v < gm, gm, v)                          # (a NaN survives into max(u))
        um = u.flatten(1).max(dim=1).values
        um = torch.where(torch.isnan(u).flatten(1).any(dim=1), torch.full_like(um, float("nan")), um)
        ok = torch.isfinite(S) & torch.isfinite(um)
        if loss_function == "norm":
            ok = ok & (S != 0)
        nn = u / um[:, None, None]
        nn = torch.where(nn < gm, gm, nn)
        n = torch.where(ok[:, None, None], nn, n).float().double()     # stored as fp32, as the kernels store them
    return n


class ConditioningMethod(ABC):
    _gain = None            # the learnt vignetting gain field (`PosteriorSamplingOsmosis.set_gain_field`); class default: none
    _gain_hold = None       # the autograd route's G while it walks the inner iterations of ONE sub-step
    _gain_freeze = False    # that sub-step freezes phi: the field is not stepped either
    _depth = None           # the range-map depth prior (`PosteriorSamplingOsmosis.set_depth_prior`); class default: none
    _mask = None            # [B or 1, 3, HW] fp32 (`set_measurement_mask`); class default: conditioners without one are unmasked
    _mask_hw = None
    _robust = None          # the robust data term's setting and per-batch state (`set_robust`); class default: plain least squares
    _robust_hold = None     # the autograd route's M_eff while it walks the inner iterations of ONE sub-step
    _robust_holding = False
    _batch = None           # the open batch (`open_batch`): (B0, the image's grid, the measurement's grid, the device)

    def __init__(self, operator, noiser, **kwargs):
        self.operator = operator
        self.noiser = noiser

    # ---------------------------------------------------------------- the batch, and the rows of it that a call is
    def open_batch(self, B, image_grid, measurement_grid, device):
        """What a loop calls once per chain, before its first data-term call: fixes the batch size B0 = B that `rows=` ranges count
        in, puts the mask rows [B0,3,hw] on `device` and creates the per-batch state of the robust term, the depth prior and the
        gain field at its initial values, so that `*_values()` read NaN / 0 / a flat field until the first guided sub-step.  State
        that fits these shapes is kept; the routings that are not built are refused here.  A `set_*` call closes the batch."""
        self._robust_refuse()
        self._gain_refuse()
        nb = getattr(self.operator, "weight_sets", (1, 1))[0]
        if nb > 1 and int(B) != nb:      # one point-spread function per image (`per_image`): the weight rows ARE the batch's
            raise ValueError(f"per_image: the operator carries one point-spread function per image of a batch of {nb}; the chain's "
                             f"batch has {int(B)} images")
        (H, W), (h, w) = (int(v) for v in image_grid), (int(v) for v in measurement_grid)
        self.measurement_mask(B, h * w, device)
        if self._robust is not None:
            self._robust_state(B, h * w, device)
        if self._depth is not None:
            self.depth_prior_rows(B, H, W, device)
        if self._gain is not None:
            self.gain_open(B, H, W, device)
        self._batch = (int(B), (H, W), (h, w), torch.device(device))

    def _batch_rows(self, rows, x0, y):
        """(r0, r1): which images of the open batch a call on x0 [B,C,H,W], y [B,3,h,w] is.  Every per-batch store is sliced [r0:r1],
        and the kernels write the optimizer, fit, sigma and node rows of every image they are handed: this is the ONE check between
        a wrong chunk and an out-of-bounds device write, made before anything is allocated or launched.  rows=None: the whole
        batch -- one is opened at the call's own shapes (state that fits is kept)."""
        if x0.dim() != 4 or y.dim() != 4:
            raise ValueError(f"expected x0 [B,C,H,W] and measurement [B,3,h,w], got {tuple(x0.shape)} and {tuple(y.shape)}")
        B, grids = x0.shape[0], (tuple(x0.shape[2:]), tuple(y.shape[2:]))
        if rows is None:
            self.open_batch(B, *grids, x0.device)
            return 0, B
        bt = self._batch
        if bt is None or bt[1:3] != grids or bt[3].type != x0.device.type or bt[3].index not in (None, x0.device.index):
            raise ValueError(f"rows={rows!r}: no batch with this call's grids {grids} on {x0.device} is open (`open_batch`)")
        try:
            r0, r1 = (index(r) for r in rows)
            ok = 0 <= r0 < r1 <= bt[0] and r1 - r0 == B
        except (TypeError, ValueError):         # no pair, or not of integers
            ok = False
        if not ok:
            raise ValueError(f"rows must be ints (r0, r1) with 0 <= r0 < r1 <= {bt[0]} (the open batch) and r1 - r0 = {B} (this call's "
                             f"images), got {rows!r}")
        return r0, r1

    def _mask_rows(self, mask, r0, r1, hw):
        """The mask rows [r1-r0,3,hw] of a call: the caller's own (`mask=`) in the stored mask's place, else rows [r0:r1] of the stored
        mask; None without either."""
        if mask is None:
            return None if self._mask is None else self._mask[r0:r1]
        if mask.numel() != (r1 - r0) * 3 * hw or not mask.is_contiguous():
            raise ValueError(f"expected mask rows [{r1 - r0},3,{hw}], got {tuple(mask.shape)}")
        return mask

    # ---------------------------------------------------------------- robust data term (include/osmosis_robust.h)
    ROBUST_CHAIN_KEYS = ("loss", "c", "scale", "sigma_min", "per_pixel")       # what `set_robust` takes from a chain (`p_sample_loop(robust=)`)

    def set_robust(self, loss="tukey", c=None, scale="mad", sigma_min=2.0 / 255.0, per_pixel=False):
        """Make the data term robust to outliers in the measurement (marine snow, highlights, caustics, a fish): per guided sub-step
        and per image, the raw residual e = y - prediction (osmosis: 2 I - 1 at the phi the sub-step starts from; 'ps': x0) gives a
        scale sigma = max(1.4826 median |e|, sigma_min) over the valid entries (mask > 0, e finite; the three channels pooled), the
        weights omega(|e| / (c sigma)) of `loss` 'huber' | 'tukey' | 'cauchy', and the data term runs its masked route with
        M sqrt(omega) in the mask's place (iteratively re-weighted least squares: omega is a constant of the sub-step; the reported
        loss is the weighted one).  c: the tuning constant (None: 1.345 / 4.685 / 2.385, 95 % efficiency at the normal); scale: 'mad'
        or a fixed sigma > 0; per_pixel: one weight per pixel from its worst valid channel.  `set_robust(None)` clears the setting;
        with none set nothing changes.  Three small kernels (csrc/robust.hip), outside the phi loop, no host sync."""
        self._batch = None      # (the per-batch state changes: `open_batch` again)
        if loss is None:
            self._robust = None
            return None
        if loss not in ROBUST_LOSSES:
            raise ValueError(f"robust: loss must be one of {ROBUST_LOSSES}, got {loss!r}")
        d = ops.robust_desc(loss, c, scale, sigma_min, per_pixel, 1, 1)       # (the host-side range checks; nothing launches)
        self._robust = {"loss": loss, "c": float(d.c), "scale": "mad" if d.scale_mode == 0 else float(d.scale),
                        "sigma_min": float(d.sigma_min), "per_pixel": bool(per_pixel), "state": None}
        self._robust_refuse()
        self._gain_refuse()
        return self._robust

    def _gain_refuse(self):
        """What the gain field is not routed through: the robust term, a degradation inside the physical operator."""
        if self._gain is None:
            return
        if self._robust is not None:
            raise NotImplementedError("gain_field: the gain field together with the robust data term (`set_robust`) is not built -- both "
                                      "claim the mask of the masked route")
        if getattr(self.operator, "degradation", None) is not None:
            raise NotImplementedError("gain_field: the gain field is not routed through a physical operator with a `degradation` (the "
                                      "field would live on the degradation's grid)")

    def _robust_refuse(self):
        """The routings that are not built: the residual on a linear operator's grid."""
        if self._robust is None:
            return
        from .measurements import GRID_OPERATORS
        if getattr(self.operator, "degradation", None) is not None:
            raise NotImplementedError("robust: the robust data term is not routed through a physical operator with a `degradation` "
                                      "(the residual would live on the degradation's grid)")
        if isinstance(self.operator, GRID_OPERATORS):
            raise NotImplementedError(f"robust: the robust data term is not routed through a 'ps' grid operator "
                                      f"({type(self.operator).__name__}); the identity operator is")

    def _robust_kw(self):
        rb = self._robust
        return dict(loss=rb["loss"], c=rb["c"], scale=rb["scale"], sigma_min=rb["sigma_min"], per_pixel=rb["per_pixel"])

    def _robust_state(self, B0, hw, device):
        """The per-BATCH state: e, M_eff, omega [B0,3,hw], sigma [B0] (NaN) and n_valid [B0] int32 (0) until a guided sub-step writes
        them.  A call on a chunk writes the chunk's rows."""
        rb = self._robust
        st = rb["state"]
        if st is None or st["key"] != (B0, hw, str(device)):
            f32 = dict(device=device, dtype=torch.float32)
            st = rb["state"] = {"key": (B0, hw, str(device)), "e": torch.zeros(B0, 3, hw, **f32), "meff": torch.zeros(B0, 3, hw, **f32),
                                "omega": torch.zeros(B0, 3, hw, **f32),
                                "sigma": torch.full((B0,), float("nan"), **f32),
                                "n": torch.zeros(B0, device=device, dtype=torch.int32), "desc": {}}
        return st

    def _robust_mask_rows(self, pred, pa, pb, y, M0, r0, r1):
        """The sub-step's M_eff rows [B,3,hw] from the prediction `pred` [B,P>=3,hw] (its first three planes) and the base-mask rows
        M0 (None: ones, which the entry points take as a null pointer): the three launches of include/osmosis_robust.h from one call,
        or singly with OSM_PHYS_PY_LOOP=1."""
        st = self._robust["state"]
        B, hw = r1 - r0, st["key"][1]
        d = st["desc"].get(B)
        if d is None:
            d = st["desc"][B] = ops.robust_desc(B=B, hw=hw, **self._robust_kw())
        e, meff, omega, sigma, n = (st[k][r0:r1] for k in ("e", "meff", "omega", "sigma", "n"))
        if d.scale_mode == 1:           # a fixed scale: the kernels write neither; the reported sigma is the scale, nothing is counted
            sigma.fill_(float(d.scale))
        if os.environ.get("OSM_PHYS_PY_LOOP", "0") != "1":
            ops.robust_mask(d, pred, pa, pb, y, M0, e, sigma, n, meff, omega)
            return meff
        ops.robust_resid(d, pred, pa, pb, y, e)
        if d.scale_mode == 0:
            ops.robust_scale(d, e, M0, sigma, n)
        ops.robust_weights(d, e, M0, sigma, meff, omega)
        return meff

    def _robust_torch(self, e, measurement):
        """M_eff shaped like the measurement [B,3,H,W] on the torch routes (the same contract by torch.sort) over the whole batch,
        kept for `robust_values`."""
        B, _, H, W = measurement.shape
        st = self._robust_state(B, H * W, measurement.device)
        meff, omega, sigma, n = robust_weights_torch(e.to(torch.float32), self._mask_like(measurement), **self._robust_kw())
        with torch.no_grad():
            st["meff"].copy_(meff.reshape(B, 3, H * W))
            st["omega"].copy_(omega.reshape(B, 3, H * W))
            st["sigma"].copy_(sigma)
            st["n"].copy_(n if isinstance(self._robust["scale"], str) else torch.zeros_like(n))
        return meff.to(e.dtype)

    def robust_values(self):
        """{'scale': sigma [B], 'n_valid': [B] int32, 'weight': omega [B,3,hw]} over the whole batch (device tensors, no sync), each
        image's from the last guided sub-step that covered it -- also when the batch was walked in chunks.  Before the first guided
        sub-step: scale NaN, n_valid 0, weight 0.  With a fixed scale nothing is selected or counted: scale is the fixed value once a
        guided sub-step has run, and n_valid stays 0.
        None with robust unset or before the state exists."""
        rb = self._robust
        if rb is None or rb["state"] is None:
            return None
        st = rb["state"]
        return {"scale": st["sigma"], "n_valid": st["n"], "weight": st["omega"]}

    # ---------------------------------------------------------------- per-pixel validity mask of the measurement
    def set_measurement_mask(self, mask, batch=None, device=None):
        """Weigh the data term per pixel: the residual of channel c becomes (y_c - A(x0)_c) w M_c (osmosis; w the none / depth weight)
        or M_c (y_c - x0_c) ('ps', which makes the data term inpainting).  mask: [B,3,H,W], [B,1,H,W], [1,3,H,W] or [1,1,H,W] in
        [0, 1] (0 ignore, 1 trust fully, fractions are confidences); None clears it.  Stored as contiguous [B,3,HW] on `device`
        (default: the mask's own), the layout of the measurement; a batch-1 mask serves every image of a batch.  The losses keep
        their normalisation: mse still divides by 3 HW, so a mask of ones IS the unmasked loss; the auxiliary losses act on the
        prediction and are not masked.  An image that is masked out entirely has loss 0, no data-term gradient and (norm) no phi
        step."""
        self._batch = None      # (the per-batch state changes: `open_batch` again)
        if mask is None:
            self._mask = self._mask_hw = None
            return None
        mask = validate_measurement_mask(mask, batch)
        B0 = mask.shape[0] if batch is None else int(batch)
        H, W = mask.shape[2], mask.shape[3]
        if device is not None:
            mask = mask.to(device)
        self._mask = mask.expand(B0, 3, H, W).reshape(B0, 3, H * W).contiguous()
        self._mask_hw = (H, W)
        return self._mask

    def measurement_mask(self, B, HW, device):
        """The stored mask as [B,3,HW] rows on `device` (None: no mask)."""
        m = self._mask
        if m is None:
            return None
        if m.shape[2] != HW or m.shape[0] not in (1, B):
            raise ValueError(f"measurement mask [{m.shape[0]},3,{m.shape[2]}] does not fit a measurement [{B},3,{HW}]")
        if m.shape[0] != B or m.device != torch.device(device):
            m = m.to(device).expand(B, 3, HW).contiguous()
            self._mask = m
        return m

    def _mask_like(self, measurement):
        """The stored mask shaped like the measurement [B,3,H,W] (autograd paths), or None."""
        if self._mask is None:
            return None
        B, _, H, W = measurement.shape
        return self.measurement_mask(B, H * W, measurement.device).view(B, 3, H, W)

    def project(self, data, noisy_measurement, **kwargs):
        return self.operator.project(data=data, measurement=noisy_measurement, **kwargs)

    def grad_and_value(self, x_prev, x_0_hat, measurement, **kwargs):
        """DPS data term for the rgb-guidance variant (reference :35-53); torch autograd."""
        self._robust_refuse()
        if self.noiser.__name__ == "gaussian":
            diff = measurement - self.operator.forward(x_0_hat[:, 0:3], **kwargs)
            if self._robust is not None:        # the robust term: M sqrt(omega) from the raw residual, a constant of the step
                m = self._robust_torch(diff, measurement)
            else:
                m = self._mask_like(measurement)
            if m is not None:
                diff = diff * m
            loss = torch.linalg.norm(diff)
        elif self.noiser.__name__ == "poisson":
            if self._robust is not None:
                raise NotImplementedError("robust: the robust data term is defined on the gaussian data term only; the poisson noiser's "
                                          "is not weighted")
            diff = measurement - self.operator.forward(x_0_hat, **kwargs)
            loss = (torch.linalg.norm(diff) / measurement.abs()).mean()
        else:
            raise NotImplementedError
        return torch.autograd.grad(outputs=loss, inputs=x_prev)[0], loss

    @abstractmethod
    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        pass


@register_conditioning_method(name="osmosis")
class PosteriorSamplingOsmosis(ConditioningMethod):
    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.scale = _parse_scale(kwargs.get("scale", 1.0))
        self.gradient_x_prev = kwargs.get("gradient_x_prev", False)
        self.pattern_name = kwargs.get("pattern", "original")
        self.global_N = kwargs.get("global_N", 1)
        self.local_M = kwargs.get("local_M", 1)
        self.n_iter = kwargs.get("n_iter", 1)
        self.update_start = kwargs.get("update_start", 1.0)

        aux = kwargs.get("aux_loss", None)
        if aux is not None:
            self.aux_loss = losseso.AuxiliaryLoss({k: float(v) for k, v in aux.items()})
        else:
            self.aux_loss = None

        self.loss_function = kwargs.get("loss_function", "norm")
        self.loss_weight = kwargs.get("loss_weight", None)
        self.weight_function = kwargs.get("weight_function", None)

        clip = [p for p in kwargs.get("gradient_clip", "False").split(",")]
        self.gradient_clip = utilso.str2bool(clip[0])
        self.gradient_clip_value = float(clip[1].strip()) if self.gradient_clip else None
        self._state = None
        self._states = {}       # per (chunk size, HW, device): a batch walked in chunks of two sizes keeps both
        self._opt = None        # optimizer state of the operator's WHOLE phi block (chunks take their rows)

    # ---------------------------------------------------------------- device state
    @property
    def clip_value(self) -> float:
        """Clamp bound handed to osm_guide_update: < 0 = no clipping.  The reference clamps only in its
        gradient_x_prev branch (condition_methods.py:213-221); `gradient_clip: "True,0"` clamps to zero there."""
        return float(self.gradient_clip_value) if (self.gradient_clip and self.gradient_x_prev) else -1.0

    def scale4(self, device):
        s = self.scale.to(torch.float32)
        if s.numel() == 1:
            s = s.repeat(4)
        if s.numel() != 4:
            raise ValueError("scale must have 1 or 4 entries (RGBD)")
        return s.to(device).contiguous()

    # ---------------------------------------------------------------- learnt vignetting gain field (include/osmosis_gain.h)
    GAIN_FIELD_CHAIN_KEYS = ("grid", "eta", "n_iter", "smooth", "g_min", "init", "learn")      # what `set_gain_field` takes from a chain

    def set_gain_field(self, grid=(5, 5), eta=0.01, n_iter=1, smooth=0.0, g_min=0.05, init=None, learn=True):
        """Model the photo as G F(x0; phi) with one smooth gain G(p) <= 1 per pixel (lens vignetting, the fall-off of a strobe): G is
        the bilinear interpolation of `grid` = (gh, gw) nodes on the image corners, 2 <= gh, gw <= 32.  Per guided sub-step that does
        not freeze phi and per image, `n_iter` projected gradient steps of size `eta` on the nodes at the phi the sub-step starts
        from (`smooth` weighs the 4-neighbour Laplacian; the nodes stay >= `g_min` and are scaled to max = 1, since a global gain is
        a scaling of J and phi_inf), then the data term runs its masked route on y' = (y + 1) / G - 1 with the mask M G -- which IS
        the residual of G F, so the phi loop and dL/dx0 are the existing kernels'.  init: nodes [gh,gw] or [B,gh,gw] (scaled to
        max = 1 per image), default a flat field; `learn=False` keeps them: the way in for a measured flat field.
        `set_gain_field(None)` clears the setting; with none set nothing changes.  Three small kernels (csrc/gainfield.hip) before
        the phi loop, no host sync.  The per-batch state starts afresh with every call."""
        self._batch = None      # (the per-batch state changes: `open_batch` again)
        if grid is None:
            self._gain = None
            return None
        gh, gw, eta, n_iter, smooth, g_min = ops.gain_check(grid, eta, n_iter, smooth, g_min)
        if init is not None:
            init = torch.as_tensor(np.asarray(init.detach().cpu() if torch.is_tensor(init) else init, dtype=np.float64))
            if init.dim() == 2:
                init = init[None]
            if init.dim() != 3 or tuple(init.shape[1:]) != (gh, gw):
                raise ValueError(f"gain_field: init must be nodes [{gh},{gw}] or [B,{gh},{gw}], got {tuple(init.shape)}")
            if not bool(torch.isfinite(init).all()) or not bool((init > 0).all()):
                raise ValueError("gain_field: init must be finite and > 0 everywhere")
            init = (init / init.flatten(1).max(dim=1).values[:, None, None]).clamp(min=g_min).to(torch.float32)
        self._gain = {"grid": (gh, gw), "eta": eta, "n_iter": n_iter, "smooth": smooth, "g_min": g_min, "learn": bool(learn),
                      "init": init, "state": None}
        self._gain_refuse()
        return self._gain

    def gain_open(self, B, H, W, device):
        """What `open_batch` creates: the per-BATCH state (nodes [B,gh,gw], field [B,1,HW], the rows y' and M' [B,3,HW]) at
        its initial values, so that `gain_values` reads them until the first guided sub-step.  A call on a chunk writes its rows."""
        gn = self._gain
        self._gain_refuse()
        st = gn["state"]
        key = (int(B), int(H), int(W), str(device))
        if st is not None and st["key"] == key:
            return st
        gh, gw = gn["grid"]
        if gh > H or gw > W:
            raise ValueError(f"gain_field: grid {gh} x {gw} has more nodes than the image has pixels ({H} x {W})")
        init = gn["init"]
        if init is not None and init.shape[0] not in (1, B):
            raise ValueError(f"gain_field: init [{init.shape[0]},{gh},{gw}] does not fit a batch of {B}")
        f32 = dict(device=device, dtype=torch.float32)
        nodes = torch.ones(B, gh, gw, **f32) if init is None else init.to(device).expand(B, gh, gw).contiguous()
        Hy, Hx = gain_hats(H, W, gh, gw, device)
        st = gn["state"] = {"key": key, "nodes": nodes, "field": (Hy @ nodes.double() @ Hx.T).to(torch.float32).reshape(B, 1, H * W),
                            "y_eff": torch.zeros(B, 3, H * W, **f32), "m_eff": torch.zeros(B, 3, H * W, **f32), "ws": {}}
        return st

    def _gain_prepare(self, d, x0c, yc, M0, phi, freeze_phi, r0, r1):
        """The sub-step's (y' rows, M' rows) [B,3,HW]: osm_phys_forward at the starting phi, then the 2 n_iter + 1 launches of
        include/osmosis_gain.h from one call, or singly with OSM_PHYS_PY_LOOP=1."""
        gn = self._gain
        B, _, H, W = x0c.shape
        st = gn["state"]
        ws = st["ws"].get((B, d.loss_type, d.weight_type))
        if ws is None:
            P = ops.phys_lin_planes(d)
            gd = ops.gain_desc(gn["grid"], gn["eta"], gn["n_iter"], gn["smooth"], gn["g_min"], gn["learn"], d.loss_type, P, B, H, W)
            ws = st["ws"][(B, d.loss_type, d.weight_type)] = {
                "desc": gd, "F": torch.empty(B, P, H * W, device=x0c.device, dtype=torch.float32), "tsc": ops.gain_workspace(gd, x0c.device)}
        gd, F, (t, s, cs) = ws["desc"], ws["F"], ws["tsc"]
        tabs = ops.gain_tables(H, W, gd.gh, gd.gw, x0c.device)
        nodes, field, y_eff, m_eff = (st[k][r0:r1] for k in ("nodes", "field", "y_eff", "m_eff"))
        learn = gn["learn"] and not freeze_phi
        if learn:
            ops.phys_forward(d, x0c, phi, F)
        if os.environ.get("OSM_PHYS_PY_LOOP", "0") != "1":
            ops.gain_prepare(gd, tabs, F, yc, M0, nodes, t, s, cs, y_eff, m_eff, field, freeze_phi=freeze_phi)
            return y_eff, m_eff
        if learn:
            for _ in range(gd.n_iter):
                ops.gain_rows(gd, tabs, nodes, F, yc, M0, t, s)
                ops.gain_step(gd, tabs, t, s, nodes, cs)
        ops.gain_expand(gd, tabs, nodes, yc, M0, y_eff, m_eff, field)
        return y_eff, m_eff

    def _gain_torch(self, image, w, measurement):
        """G [B,1,H,W] on the torch routes, in the measurement's dtype: the same gradient and step (`gain_learn_torch`) at the phi the
        sub-step starts from, the state kept for `gain_values`."""
        gn = self._gain
        B, _, H, W = measurement.shape
        st = self.gain_open(B, H, W, measurement.device)
        if gn["learn"] and not self._gain_freeze:
            n = gain_learn_torch(st["nodes"], image, w, measurement, self._mask_like(measurement), self.loss_function, gn["eta"],
                                 gn["n_iter"], gn["smooth"], gn["g_min"])
            st["nodes"].copy_(n)
        Hy, Hx = gain_hats(H, W, gn["grid"][0], gn["grid"][1], measurement.device)
        G = (Hy @ st["nodes"].double() @ Hx.T)[:, None]
        st["field"].copy_(G.reshape(B, 1, H * W))
        return G.to(measurement.dtype)

    def gain_values(self):
        """{'nodes': [B,gh,gw], 'field': G [B,1,HW]} over the whole batch (device tensors, no sync), each image's from the last guided
        sub-step that covered it -- also when the batch was walked in chunks; the initial values until the first guided sub-step.
        None with no gain field set or before a loop has opened the state."""
        gn = self._gain
        if gn is None or gn["state"] is None:
            return None
        return {"nodes": gn["state"]["nodes"], "field": gn["state"]["field"]}

    # ---------------------------------------------------------------- range-map depth prior (include/osmosis_depthprior.h)
    _depth_serial = 0
    DEPTH_PRIOR_CHAIN_KEYS = ("z", "confidence", "weight", "align", "loss", "scale", "scale_min")     # what `set_depth_prior` takes from a chain

    def set_depth_prior(self, z, confidence=None, weight=1.0, align="affine", loss="norm", scale=1.0, scale_min=1e-3, batch=None,
                        device=None):
        """Hand a range map to the data term: with d the operator's converted depth (what phi multiplies) and (a, c) the per-image
        least-squares fit d ~ a z + c over the pixels with confidence m > 0, the objective of a guided sub-step becomes
        data + auxiliary + weight * L_depth, L_depth = sqrt(sum m (d - a z - c)^2) ('norm') or that sum / sum m ('mse').
        z: [B,1,H,W], [1,1,H,W] or [B,H,W] on the network's grid, any unit (metres make phi * a an attenuation per metre);
        confidence: the same shape in [0, 1]; a range that is not finite or <= 0 is invalid (m = 0, z = 0 there).  align 'affine' |
        'scale' (c = 0) | 'none' (a = `scale`, c = 0); `scale_min` > 0 bounds a from below.  None clears the prior.  The term does not
        depend on phi: it is added to dL/dx0 once, after the route's inner loop, by three small kernels (csrc/depthprior.hip)."""
        self._batch = None      # (the per-batch state changes: `open_batch` again)
        if z is None:
            self._depth = None
            return None
        if align not in DEPTH_ALIGNS:
            raise ValueError(f"depth prior: align must be one of {DEPTH_ALIGNS}, got {align!r}")
        if loss not in DEPTH_LOSSES:
            raise ValueError(f"depth prior: loss must be one of {DEPTH_LOSSES}, got {loss!r}")
        weight, scale, scale_min = float(weight), float(scale), float(scale_min)
        if not (weight >= 0.0 and weight < float("inf")):
            raise ValueError(f"depth prior: weight must be finite and >= 0, got {weight}")
        if not (scale_min > 0.0 and scale_min < float("inf")) or not (abs(scale) < float("inf")):
            raise ValueError(f"depth prior: scale must be finite and scale_min finite and > 0, got {scale} and {scale_min}")
        z, m = validate_depth_prior(z, confidence, batch)
        B0 = z.shape[0] if batch is None else int(batch)
        H, W = z.shape[2], z.shape[3]
        if device is not None:
            z, m = z.to(device), m.to(device)
        self._depth = {"z": z.expand(B0, 1, H, W).reshape(B0, 1, H * W).contiguous(),
                       "m": m.expand(B0, 1, H, W).reshape(B0, 1, H * W).contiguous(), "grid": (H, W), "weight": weight, "align": align,
                       "loss": loss, "scale": scale, "scale_min": scale_min, "ver": PosteriorSamplingOsmosis._depth_serial + 1}
        PosteriorSamplingOsmosis._depth_serial += 1     # (a workspace built for an earlier prior's parameters is rebuilt)
        self._depth_store(self._depth)
        return self._depth

    @staticmethod
    def _depth_store(dp):
        """The prior's per-BATCH results, beside its rows: fit [B0,4] float64 = a, c, gs, L and loss [B0] fp32, NaN until a guided
        sub-step has written them.  A call on a chunk writes the chunk's rows (`rows=`), so a batch walked in chunks ends with
        every image's own fit -- the counterpart of the data term's `loss_out` rows."""
        z = dp["z"]
        dp["out_fit"] = torch.full((z.shape[0], 4), float("nan"), device=z.device, dtype=torch.float64)
        dp["out_loss"] = torch.full((z.shape[0],), float("nan"), device=z.device, dtype=torch.float32)

    def depth_prior_rows(self, B, H, W, device):
        """The stored prior as ([B,1,HW] range rows, [B,1,HW] confidence rows) on `device`, or None without a prior."""
        dp = self._depth
        if dp is None:
            return None
        z, m = dp["z"], dp["m"]
        if dp["grid"] != (int(H), int(W)) or z.shape[0] not in (1, B):
            raise ValueError(f"depth prior [{z.shape[0]},1,{dp['grid'][0]},{dp['grid'][1]}] does not fit an image batch [{B},4,{H},{W}] "
                             "(the prior lives on the image's grid)")
        if z.shape[0] != B or z.device != torch.device(device):
            dp["z"] = z = z.to(device).expand(B, 1, H * W).contiguous()
            dp["m"] = m = m.to(device).expand(B, 1, H * W).contiguous()
            self._depth_store(dp)
        return z, m

    def _apply_depth_prior(self, st, x0c, g, r0, r1):
        """The prior's launches on the g the route has just written: g[:, 3] += weight * d L_depth / d x0[:, 3] where m > 0, with
        rows [r0:r1] of the prior and of its per-batch results."""
        dp = self._depth
        B, _, H, W = x0c.shape
        HW = H * W
        z, m, fit, loss = (dp[k][r0:r1] for k in ("z", "m", "out_fit", "out_loss"))
        if not g.is_contiguous() or g.numel() != B * 4 * HW:
            raise ValueError("the depth prior adds into a contiguous [B,4,HW] gradient")
        ws = st.get("depth")
        if ws is None or ws["ver"] != dp["ver"]:
            d = st["desc"]
            ws = {"ver": dp["ver"],
                  "desc": ops.depth_desc(dp["align"], dp["loss"], dp["weight"], dp["scale"], dp["scale_min"], d.depth_type, d.dval, B, HW),
                  "part": torch.empty(B * ops.depth_nblk(HW) * 8, device=x0c.device, dtype=torch.float64)}
            st["depth"] = ws
        if os.environ.get("OSM_PHYS_PY_LOOP", "0") != "1":
            ops.depth_loss_grad(ws["desc"], x0c, z, m, ws["part"], fit, loss, g)
            return
        ops.depth_reduce(ws["desc"], x0c, z, m, ws["part"])
        ops.depth_fit(ws["desc"], ws["part"], fit, loss)
        ops.depth_grad(ws["desc"], x0c, z, m, fit, g)

    def depth_prior_values(self):
        """{'loss': [B], 'scale': [B], 'shift': [B]} over the prior's whole batch (device tensors, no sync), each image's from the last
        guided sub-step that covered it -- also when the batch was walked in chunks: L_depth without its weight, and the fit's a and
        c (NaN where a guard skipped the image; everything NaN before the first guided sub-step).  None without a prior."""
        dp = self._depth
        return None if dp is None else {"loss": dp["out_loss"], "scale": dp["out_fit"][:, 0], "shift": dp["out_fit"][:, 1]}

    def _depth_torch(self, D):
        """The operator's depth conversion on a torch tensor (the kernels' conv_depth; an operator without one: 'original')."""
        code, v = getattr(self.operator, "depth_code", 0), getattr(self.operator, "depth_vals", (0.0, 1.0, 1.0))
        if code == 1:
            base = (D + v[0]) * v[1]
            return base if v[2] == 1.0 else torch.pow(base, v[2])
        return D + v[0] if code == 2 else 0.5 * (D + 1.0)

    def _depth_autograd(self, x_0_hat):
        """weight * sum_b L_depth[b] on torch tensors (the autograd routes), or None without a prior; keeps the values for
        `depth_prior_values`."""
        dp = self._depth
        if dp is None:
            return None
        B, _, H, W = x_0_hat.shape
        z, m = self.depth_prior_rows(B, H, W, x_0_hat.device)
        L, reported, a, c = depth_prior_term(self._depth_torch(x_0_hat[:, 3:4]), z.view(B, 1, H, W).to(x_0_hat.dtype),
                                             m.view(B, 1, H, W).to(x_0_hat.dtype), dp["align"], dp["loss"], dp["scale"], dp["scale_min"])
        with torch.no_grad():
            dp["out_loss"].copy_(reported)
            dp["out_fit"][:, 0].copy_(a)
            dp["out_fit"][:, 1].copy_(c)
        return dp["weight"] * L.sum()

    def _degradation(self):
        """The operator's `degradation` when the composed kernels serve it (a blur / super-resolution / PSF operator), else None."""
        from .measurements import GRID_OPERATORS
        deg = getattr(self.operator, "degradation", None)
        return deg if isinstance(deg, GRID_OPERATORS) else None

    def _prepare(self, B, HW, device, grid=None):
        """The descriptor and buffers of a (B, HW, device) batch; grid = (H, W) with a degradation: keyed by (B, H, W, device), with
        the operator's descriptor and the workspaces of the composed route (include/osmosis_physlin.h)."""
        key = (B, HW, str(device)) if grid is None else (B, HW, str(device), int(grid[0]), int(grid[1]))
        st = self._states.get(key)
        if st is not None:
            self._state = st
            return st
        op = self.operator
        if not hasattr(op, "fill_desc"):
            raise NotImplementedError(f"operator {type(op).__name__} has no HIP physics kernels")
        if self.loss_function not in ("norm", "mse"):
            raise NotImplementedError
        d = PhysDesc()
        op.fill_desc(d)
        if self.loss_weight in (None, "none"):
            d.weight_type, d.wdepth_type = 0, 0
        elif self.loss_weight == "depth":
            fn, value = utilso.parse_weight_function(self.weight_function)
            code, vals = utilso.depth_code_and_values(fn if fn != "none" else None, value)
            d.weight_type, d.wdepth_type = 1, code
            for i in range(3):
                d.wval[i] = vals[i]
        else:
            raise NotImplementedError
        d.loss_type = 0 if self.loss_function == "norm" else 1
        coefs = self.aux_loss.kernel_coefficients() if self.aux_loss is not None else {"gamma_avrg": 0.0, "gamma_val": 0.0}
        d.gamma_avrg, d.gamma_val = coefs["gamma_avrg"], coefs["gamma_val"]
        d.B, d.HW = B, HW
        from .measurements import optimizer_code
        d.optimizer = optimizer_code(getattr(op, "optimizer", ""))
        lm = d.optimizer == 9   # the Levenberg-Marquardt solver: its reduce writes 32 floats per workgroup (include/osmosis_hip.h)
        nblk = ops.phys_nblk(HW)
        if d.optimizer != 0 and (self._opt is None or self._opt.shape[0] != op.phi.shape[0] or self._opt.device != op.phi.device):
            # optimizer state (Adam: moments + step) of the operator's phi (torch.optim state lives with the optimizer = with the operator,
            # which the driver rebuilds per image: osmosis_sampling.py:142-155)
            self._opt = torch.zeros(op.phi.shape[0], 20, device=device, dtype=torch.float32)
            if lm:
                self._opt[:, 10] = float(getattr(op, "lm_lambda", 1.0))     # the solver's initial damping
        st = {"key": key, "desc": d,
              "part": torch.empty(B * nblk * (32 if lm else 16), device=device, dtype=torch.float32),
              "red": torch.zeros(B * 16, device=device, dtype=torch.float32),
              "loss": torch.zeros(B, device=device, dtype=torch.float32),
              "g": torch.empty(B, 4, HW, device=device, dtype=torch.float32)}
        if grid is not None:
            lin = ops.lin_desc(self._degradation(), grid[0], grid[1], device)
            hw, P = lin.h * lin.w, ops.phys_lin_planes(d)
            f32 = dict(device=device, dtype=torch.float32)
            if lm:
                raise NotImplementedError("optimizer 'lm' (the Levenberg-Marquardt phi solver) is not routed through a `degradation`")
            st.update(lin=lin, hw=hw, F=torch.empty(B, P, HW, **f32), AF=torch.empty(B, P, hw, **f32), u=torch.empty(B, 3, hw, **f32),
                      v=torch.empty(B, 3, HW, **f32), part_r=torch.empty(B * ops.phys_nblk(hw), **f32))
        if lm:      # the plain 16-sum reduce of the solver's closing evaluation and of freeze_phi, for the single-launch schedule
            d0 = PhysDesc.from_buffer_copy(d)
            d0.optimizer = 0
            st["desc_plain"] = d0
        while len(self._states) >= 4:          # a walk uses at most two chunk sizes; older shapes give their buffers back
            self._states.pop(next(iter(self._states)))
        self._states[st["key"]] = st
        self._state = st
        return st

    def _group(self, r0, r1):
        """The group descriptor of an operator with shared water parameters (`phi_groups`), None without.  A group's members are
        pooled inside ONE launch, so the call must be the whole batch."""
        sizes = getattr(self.operator, "group_sizes", None)
        if sizes is None:
            return None
        if (r0, r1) != (0, self._batch[0]):
            raise ValueError(f"phi_groups: a water group spans chunks -- the data term got rows {r0}:{r1} of the batch's "
                             f"{self._batch[0]}; a grouped batch takes ONE call over all its images")
        key = (sizes, self.operator.phi_reduce)
        if getattr(self, "_grp_key", None) != key:
            self._grp, self._grp_key = ops.group_desc(sizes, self.operator.phi_reduce), key
        return self._grp

    def loss_grad_x0(self, x0, y, freeze_phi=False, g_out=None, loss_out=None, mask=None, rows=None):
        """Inner phi-optimisation + dL/dx0.  x0 [B,4,H,W], y [B,3,H,W] contiguous device fp32.
        Returns (g [B,4,H,W] view of an internal buffer (or g_out), per-image data loss [B] (device)).
        `rows` = (r0, r1): which images of the open batch (`open_batch`) x0 / y / g_out / loss_out are, when the caller walks a batch
        in chunks of independent images; every per-batch store -- the operator's phi [B0][9], the optimizer state, the stored mask,
        the robust / depth-prior / gain-field state -- is read and written at its rows [r0:r1].  None: the call is the whole batch.
        `mask`: mask rows [B,3,HW] for exactly this call's images, in the place of the one of `set_measurement_mask`.
        An operator with `phi_groups`: the same launches with ONE phi step per group and inner iteration (osm_phys_optimize_g); loss
        and g stay per image, and the call must be the whole batch.
        With a range-map prior (`set_depth_prior`) g's depth plane also carries weight * d L_depth / d x0, added after the inner
        loop; the returned loss stays the data loss (`depth_prior_values` has the prior's).
        With a gain field (`set_gain_field`) the nodes are stepped first (not when `freeze_phi`), and the route runs masked on
        (y', M G) of include/osmosis_gain.h."""
        r0, r1 = self._batch_rows(rows, x0, y)
        if getattr(self.operator, "degradation", None) is not None:
            return self._loss_grad_x0_lin(x0, y, freeze_phi, g_out, loss_out, mask, r0, r1)
        B, HW = x0.shape[0], x0.shape[2] * x0.shape[3]
        if y.shape[0] != B or y.shape[1] != 3 or x0.shape[1] != 4:
            raise ValueError("expected x0 [B,4,H,W] and measurement [B,3,H,W]")
        grp = self._group(r0, r1)               # (refuses a chunk of a grouped batch before anything else)
        st = self._prepare(B, HW, x0.device)
        d, part, red = st["desc"], st["part"], st["red"]
        phi, opt = self._phi_rows(d, r0, r1)
        loss = st["loss"] if loss_out is None else loss_out
        g = g_out if g_out is not None else st["g"]
        x0c, yc = x0.contiguous(), y.contiguous()
        mask = self._mask_rows(mask, r0, r1, HW)
        if self._gain is not None:
            # the gain field: the nodes learnt at the phi this sub-step starts from, then (y', M G) rows in the place of (y, mask) --
            # the masked residual on them is the residual of the model G F, so everything below is what it was
            yc, mask = self._gain_prepare(d, x0c, yc, mask, phi, freeze_phi, r0, r1)
        elif self._robust is not None:
            # the robust term: the model image at the phi this sub-step starts from, the raw residual's MAD scale and the IRLS weights
            # folded into the mask -- M_eff rows in the mask's place, constants of the inner loop below
            F = st.get("F_robust")
            if F is None:
                F = st["F_robust"] = torch.empty(B, ops.phys_lin_planes(d), HW, device=x0.device, dtype=torch.float32)
            ops.phys_forward(d, x0c, phi, F)
            mask = self._robust_mask_rows(F, 2.0, -1.0, yc, mask, r0, r1)
        # the route's four calls: reduce, finalize, grad, optimize (the schedule: _inner_loop)
        if grp is not None and d.optimizer == 9:
            raise NotImplementedError("optimizer 'lm' (the Levenberg-Marquardt phi solver) with phi_groups is not built")
        if grp is not None:         # shared water parameters: the grouped finalize in the place of the plain one
            route = (partial(ops.phys_reduce_m, d, x0c, yc, mask, phi, part),
                     partial(ops.phys_finalize_g, d, grp, part, red, phi, masked=mask is not None),
                     partial(ops.phys_grad_m, d, x0c, yc, mask, phi, red, g),
                     partial(ops.phys_optimize_g, d, grp, x0c, yc, mask, phi, part, red, loss, g))
        elif mask is not None:      # the same launches with the mask in the residual (osm_phys_*_m)
            route = (partial(ops.phys_reduce_m, d, x0c, yc, mask, phi, part), partial(ops.phys_finalize_m, d, part, red, phi),
                     partial(ops.phys_grad_m, d, x0c, yc, mask, phi, red, g),
                     partial(ops.phys_optimize_m, d, x0c, yc, mask, phi, part, red, loss, g))
        else:
            route = (partial(ops.phys_reduce, d, x0c, yc, phi, part), partial(ops.phys_finalize, d, part, red, phi),
                     partial(ops.phys_grad, d, x0c, yc, phi, red, g),
                     partial(ops.phys_optimize, d, x0c, yc, phi, part, red, loss, g))
        if d.optimizer == 9:        # the solver's schedule also needs the plain reduce (the fifth call of its route)
            route += (partial(ops.phys_reduce_m, st["desc_plain"], x0c, yc, mask, phi, part),)
        self._inner_loop(route, 1 if freeze_phi else self.n_iter, freeze_phi, loss, opt)
        if self._depth is not None:
            self._apply_depth_prior(st, x0c, g, r0, r1)
        return g.view(x0.shape), loss

    def _phi_rows(self, d, r0, r1):
        """Rows [r0:r1] of the operator's [B0][9] phi block and of the optimizer state beside it (None with plain SGD)."""
        full = self.operator.phi
        if full.shape[0] != self._batch[0] or not full.is_contiguous():
            raise ValueError(f"phi must be a contiguous [B][9] block over the batch's {self._batch[0]} images, got {tuple(full.shape)}")
        return full[r0:r1], (self._opt[r0:r1] if d.optimizer != 0 else None)

    @staticmethod
    def _inner_loop(route, n_inner, freeze_phi, loss, rows):
        """The inner-loop schedule of every data-term route: n_inner x { reduce; finalize + phi step }; loss and dL/dx0 use the phi of
        the LAST iteration, which is stepped afterwards.  `route`: its four calls (reduce, finalize, grad, optimize); `optimize` is
        the ONE C call that enqueues all 2 n_inner + 2 launches (one Python call per launch left the GPU idle between them).
        OSM_PHYS_PY_LOOP=1 walks the same launches through the single-launch entry points instead (A/B measurements, tests of the
        entry points)."""
        reduce, finalize, grad, optimize = route[:4]
        if os.environ.get("OSM_PHYS_PY_LOOP", "0") != "1":
            optimize(n_inner, freeze_phi, opt_state=rows)
            return
        if len(route) > 4:
            # The Levenberg-Marquardt solver (optimizer 9): n_inner x { LM reduce; LM finalize that decides and steps (do_update 2 on
            # the first iteration, then 1) }, then the closing evaluation -- the plain reduce at the trial phi, the LM finalize in close
            # mode (3), which puts the base back on a reject -- and the gradient: 2 n_inner + 3 launches.  freeze_phi: the plain three.
            reduce_plain = route[4]
            if freeze_phi:
                reduce_plain()
                finalize(0, loss)
                grad()
                return
            for it in range(n_inner):
                reduce()
                finalize(2 if it == 0 else 1, loss, opt_state=rows)
            reduce_plain()
            finalize(3, loss, opt_state=rows)
            grad()
            return
        for it in range(n_inner):
            reduce()
            if it < n_inner - 1:
                finalize(True, loss, opt_state=rows)
                continue
            finalize(False, loss)
            grad()
            if not freeze_phi:
                finalize(True, None, opt_state=rows)

    def _loss_grad_x0_lin(self, x0, y, freeze_phi, g_out, loss_out, mask, r0, r1):
        """`loss_grad_x0` with the operator's `degradation` A between the image-formation model and the photo: y and the mask live on
        A's grid (h, w) = A.out_shape(H, W).  Per inner iteration: the image (and the depth weight) materialised, A, the residual on
        the measurement's grid, A^T, then the phi reductions and step with v = A^T u where the plain route forms -2 w r inline -- all
        enqueued by one C call (osm_phys_optimize_lin), no host sync; OSM_PHYS_PY_LOOP=1 walks the single-launch entry points."""
        deg = self._degradation()
        if deg is None:
            raise NotImplementedError(f"degradation {type(self.operator.degradation).__name__} has no HIP kernels (autograd conditioning "
                                      "serves it)")
        if x0.dim() != 4 or x0.shape[1] != 4:
            raise ValueError(f"expected x0 [B,4,H,W], got {tuple(x0.shape)}")
        B, _, H, W = x0.shape
        h, w = deg.out_shape(H, W)
        if tuple(y.shape) != (B, 3, h, w):
            raise ValueError(f"expected the measurement [{B},3,{h},{w}] (the degradation's grid for a {H} x {W} image), got {tuple(y.shape)}")
        HW, hw = H * W, h * w
        grp = self._group(r0, r1)
        st = self._prepare(B, HW, x0.device, grid=(H, W))
        d, lin, part, red = st["desc"], st["lin"], st["part"], st["red"]
        F, AF, u, v, part_r = st["F"], st["AF"], st["u"], st["v"], st["part_r"]
        phi, opt = self._phi_rows(d, r0, r1)
        loss = st["loss"] if loss_out is None else loss_out
        g = g_out if g_out is not None else st["g"]
        x0c, yc = x0.contiguous(), y.contiguous()
        mask = self._mask_rows(mask, r0, r1, hw)        # (the mask lives on the measurement's grid)
        P, masked = ops.phys_lin_planes(d), mask is not None

        def reduce():
            ops.phys_forward(d, x0c, phi, F)
            ops.phys_lin_apply(lin, F, AF, B, P)
            ops.phys_resid(d, hw, AF, yc, mask, u, part_r)
            ops.phys_lin_apply(lin, u, v, B, 3, adjoint=True)
            ops.phys_reduce_lin(d, x0c, phi, v, part)
        grad = partial(ops.phys_grad_lin, d, hw, x0c, phi, v, red, g, masked=masked)
        if grp is not None:         # shared water parameters: the grouped finalize in the place of the plain one
            route = (reduce, partial(ops.phys_finalize_lin_g, d, grp, hw, part, part_r, red, phi, masked=masked), grad,
                     partial(ops.phys_optimize_lin_g, d, grp, lin, x0c, yc, mask, phi, F, AF, u, v, part_r, part, red, loss, g))
        else:
            route = (reduce, partial(ops.phys_finalize_lin, d, hw, part, part_r, red, phi, masked=masked), grad,
                     partial(ops.phys_optimize_lin, d, lin, x0c, yc, mask, phi, F, AF, u, v, part_r, part, red, loss, g))
        self._inner_loop(route, 1 if freeze_phi else self.n_iter, freeze_phi, loss, opt)
        if self._depth is not None:                             # the prior lives on the image's grid [H, W], not the measurement's
            self._apply_depth_prior(st, x0c, g, r0, r1)
        return g.view(x0.shape), loss

    def aux_values(self):
        """{'avrg_loss': [B], 'val_loss': [B]} from the last reduction (device tensors, no sync)."""
        st = self._state
        if st is None or self.aux_loss is None:
            return None
        B, HW = st["key"][0], st["key"][1]
        red = st["red"].view(B, 16)
        out = {}
        for name in self.aux_loss.losses_dictionary:
            if name == "avrg_loss":
                out[name] = (red[:, 10:13] / HW).abs().sum(dim=1)
            elif name == "val_loss":
                out[name] = red[:, 13] / (3 * HW)
        return out

    # ---------------------------------------------------------------- reference API
    def _has_kernels(self) -> bool:
        """Everything of this step is something osm_phys_* evaluates: one of the three image-formation models (the package's own
        operators), norm / mse, no weight or the depth weight, auxiliary losses with a kernel slot.  Anything else -- an operator or an
        auxiliary loss a user registered with `register_operator` / `register_loss` -- goes through torch.autograd below."""
        if not hasattr(self.operator, "fill_desc") or self.loss_function not in ("norm", "mse"):
            return False
        if self.loss_weight not in (None, "none", "depth"):
            return False
        if getattr(self.operator, "degradation", None) is not None and self._degradation() is None:
            return False            # a degradation the composed kernels do not know: `_conditioning_autograd`
        return self.aux_loss is None or all(getattr(m, "kernel_slot", None) is not None for m in self.aux_loss.losses_list)

    hip_ok = _has_kernels

    def _loss_autograd(self, x_0_hat, measurement, **kwargs):
        """condition_methods.py:109-144 on torch tensors, for operators the kernels do not know: (sep_loss ndarray[B], loss, image)."""
        self._robust_refuse()
        deg = getattr(self.operator, "degradation", None)
        # with a degradation A the photo is A I on A's grid (`observe`); the weight plane goes through A too (a constant of the step)
        image = self.operator.forward(x_0_hat, **kwargs) if deg is None else self.operator.observe(x_0_hat, **kwargs)
        w = utilso.set_loss_weight(loss_weight_type=self.loss_weight, weight_function=self.weight_function,
                                   degraded_image=image.detach(), x_0_hat=x_0_hat.detach())
        if deg is not None and torch.is_tensor(w):
            w = deg.forward(w.detach().contiguous())
        if self._gain is not None:
            # the gain field: the model is G image, G from the nodes stepped at the phi the sub-step starts from
            # (`_conditioning_autograd` holds it over its inner iterations), a constant of the step
            self._gain_refuse()
            G = self._gain_hold
            if G is None:
                G = self._gain_torch(image.detach(), w, measurement)
                if self._robust_holding:
                    self._gain_hold = G
            image = G * image
        raw = measurement - (2 * image - 1)
        diff = raw * w
        if self._robust is not None:
            # the robust term: M_eff from the raw residual at the phi the sub-step starts from (`_conditioning_autograd` holds it
            # over its inner iterations), a constant of the step
            m = self._robust_hold
            if m is None:
                m = self._robust_torch(raw, measurement)
                if self._robust_holding:
                    self._robust_hold = m
        else:
            m = self._mask_like(measurement)
        if m is not None:           # (mse below keeps its 3 HW denominator: a mask of ones is the unmasked loss)
            diff = diff * m
        # the range-map prior, weight * sum_b L_depth[b] (None without one): part of the objective, not of the reported data loss
        prior = self._depth_autograd(x_0_hat)

        def total(data_loss):
            return data_loss if prior is None else data_loss + prior
        if self.loss_function == "norm":
            sep = torch.norm(diff.detach().cpu(), p=2, dim=[1, 2, 3]).numpy()
            if getattr(self.operator, "group_sizes", None) is not None:
                # shared water parameters: a group's objective is the SUM of its members' per-image norms (what the kernels pool),
                # not the norm over the batch
                return sep, total(torch.linalg.vector_norm(diff, dim=(1, 2, 3)).sum()), image.detach()
            return sep, total(torch.linalg.norm(diff)), image.detach()
        if self.loss_function == "mse":
            mse = (diff ** 2).mean(dim=(1, 2, 3))
            return mse.detach().cpu().numpy(), total(mse.sum()), image.detach()
        raise NotImplementedError

    def _conditioning_autograd(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        """The reference's step (:146-231) through torch.autograd, for a third-party operator: n_iter x (loss + auxiliary losses,
        backward into the operator's parameter tensors, `operator.optimize`), the last one also into x_prev; then the update of x_t."""
        freeze_phi = kwargs.get("freeze_phi", False)
        if not self.gradient_x_prev:
            raise NotImplementedError("gradient_x_prev=False raises in the reference too (backward(inputs=[x_prev]) on a tensor whose "
                                      "requires_grad it has just switched off, condition_methods.py:152-157, :186-191)")
        self._robust_hold, self._robust_holding = None, True        # the robust weights: the first iteration's, for all of them
        self._gain_hold, self._gain_freeze = None, bool(freeze_phi)  # the gain field alike; a frozen sub-step does not step it
        try:
            with torch.enable_grad():
                self.operator.set_variable_gradients(value=not freeze_phi)
                n = 1 if freeze_phi else self.n_iter
                for it in range(n):
                    sep_loss, loss, _ = self._loss_autograd(x_0_hat, measurement, time_index=kwargs.get("time_index", None))
                    aux_dict = None
                    if self.aux_loss is not None:
                        aux, aux_dict = self.aux_loss.forward(x_0_hat)
                        loss = loss + aux
                    phis = [] if freeze_phi else list(self.operator.get_variable_list())
                    last = it == n - 1
                    loss.backward(inputs=([x_prev] if last else []) + phis, retain_graph=not last)
                    variables = self.operator.optimize(freeze_phi=freeze_phi)
        finally:                        # (also when an iteration raises: a later call must not meet stale weights)
            self._robust_hold, self._robust_holding = None, False
            self._gain_hold, self._gain_freeze = None, False
        with torch.no_grad():
            grads = x_prev.grad
            if self.gradient_clip:
                grads = torch.clamp(grads, min=-self.gradient_clip_value, max=self.gradient_clip_value)
            x_t -= self.scale[None, ..., None, None].to(x_prev.device) * grads
        return x_t, sep_loss, variables, x_prev.grad.cpu(), aux_dict

    def grad_and_value(self, x_prev, x_0_hat, measurement, **kwargs):
        if not self._has_kernels():
            self._robust_hold, self._robust_holding = None, False
            self._gain_hold, self._gain_freeze = None, True         # (an evaluation, as freeze_phi=True below: nothing is stepped)
            try:
                return self._loss_autograd(x_0_hat, measurement, **kwargs)
            finally:
                self._gain_freeze = False
        g, loss = self.loss_grad_x0(x_0_hat.detach(), measurement, freeze_phi=True)
        I = self.operator.forward(x_0_hat.detach())
        return loss.detach().cpu().numpy(), loss.sum(), I

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        if not self._has_kernels():
            return self._conditioning_autograd(x_prev, x_t, x_0_hat, measurement, **kwargs)
        freeze_phi = kwargs.get("freeze_phi", False)
        self.operator.set_variable_gradients(value=not freeze_phi)
        g, loss = self.loss_grad_x0(x_0_hat.detach(), measurement, freeze_phi=freeze_phi)
        with torch.no_grad():
            scale = self.scale4(x_t.device)[None, :, None, None]
        if self.gradient_x_prev:
            if x_prev.grad is not None:
                x_prev.grad = None
            x_0_hat.backward(gradient=g.clone(), inputs=[x_prev])
            grad = x_prev.grad
        else:
            grad = g
        with torch.no_grad():
            # the reference clamps in the gradient_x_prev branch only (:213-221); the x0-gradient branch is unclipped
            clip = self.gradient_clip and self.gradient_x_prev
            gc = torch.clamp(grad, -self.gradient_clip_value, self.gradient_clip_value) if clip else grad
            x_t -= scale * gc
        aux = self.aux_values()
        aux = {k: v.detach().cpu().sum() for k, v in aux.items()} if aux is not None else None
        return x_t, loss.detach().cpu().numpy(), self.operator.optimize(freeze_phi=freeze_phi), grad.detach().cpu(), aux


@register_conditioning_method(name="ps")
class PosteriorSampling(ConditioningMethod):
    """rgb-guidance DPS variant (reference :234-251).  With an identity operator ('noise' / 'rgb_guidance') and the gaussian
    noiser the data term is ||y - x0[:, 0:3]|| (:35-41): `loss_grad_x0` evaluates it and its x0-gradient with the physics
    kernels' identity operator (osm_phys_desc.kind 3), which is what the fused sampler loop calls; `conditioning` keeps the
    reference's autograd form for third-party operators / noisers."""

    def __init__(self, operator, noiser, **kwargs):
        super().__init__(operator, noiser)
        self.scale = _parse_scale(kwargs.get("scale", 1.0))
        self._states = {}

    def set_depth_prior(self, z, *args, **kwargs):
        if z is None:
            return None
        raise NotImplementedError("the 'ps' branch has no depth model (its data term is y - A x0[:, 0:3]): a range-map depth prior "
                                  "needs the 'osmosis' conditioner")

    def set_gain_field(self, grid=(5, 5), *args, **kwargs):
        if grid is None:
            return None
        raise NotImplementedError("gain_field: the 'ps' branch has no image-formation model to put a gain field in (its data term is "
                                  "y - A x0[:, 0:3]); the 'osmosis' conditioner has one")

    def _blind(self):
        """The operator when it is a `blind_blur` that learns its PSF, or a `blind_field_blur` that learns its field (the data term steps
        the weights and couples the batch), else None."""
        from .measurements import BlindBlurOperator, BlindFieldOperator
        return self.operator if isinstance(self.operator, (BlindBlurOperator, BlindFieldOperator)) and self.operator.learn else None

    def _blind_field(self):
        """The operator when it is a `blind_field_blur` that learns its field, else None."""
        from .measurements import BlindFieldOperator
        return self.operator if isinstance(self.operator, BlindFieldOperator) and self.operator.learn else None

    def hip_ok(self, channels: int = 4) -> bool:
        from .measurements import GRID_OPERATORS, _IdentityOperator
        if self._blind() is not None and getattr(self.noiser, "__name__", None) == "poisson":
            if self._blind_field() is not None:
                raise NotImplementedError("blind_field_blur learns its field on the gaussian data term only: the poisson noiser is not supported")
            raise NotImplementedError("blind_blur learns its PSF on the gaussian data term only: the poisson noiser is not supported")
        return isinstance(self.operator, (_IdentityOperator,) + GRID_OPERATORS) and \
            getattr(self.noiser, "__name__", None) == "gaussian" and self.scale.numel() in (1, channels)

    def scale4(self, device, channels: int = 4):
        """The per-channel step size as a device vector of `channels` entries (1 entry: the same for every channel)."""
        s = self.scale.to(torch.float32)
        if s.numel() not in (1, channels):
            raise ValueError(f"scale must have 1 or {channels} entries")
        return (s.repeat(channels) if s.numel() == 1 else s).to(device).contiguous()

    def loss_grad_x0(self, x0, y, g_out=None, loss_out=None, mask=None, rows=None):
        """loss[b] = ||y[b] - x0[b, 0:3]||_2 and g = d loss / d x0 (zero on any channel beyond the colours), per image (B = 1: the
        reference's batch-global norm).  x0 [B,C,H,W] with C = 4 (RGBD) or 3 (the RGB model family), y [B,3,H,W] contiguous device
        fp32.  `rows` = (r0, r1): which images of the open batch (`open_batch`) these are -- the stored mask and the robust state are
        taken at their rows [r0:r1]; None: the whole batch.  With a mask M (`mask`: [B,3,HW] rows for exactly this call's images,
        default the one of `set_measurement_mask`): loss[b] = ||M (y - x0[0:3])||,
        g = -M^2 (y - x0) / loss, and g = 0 for an image that is masked out entirely.
        With a `SeparableOperator` A (blur, super-resolution) the measurement y [B,3,h,w] lives on A's own grid, and so does the mask:
        loss[b] = ||M (y - A x0[b, 0:3])||, g[:, 0:3] = A^T d loss / d (A x0) (`_loss_grad_x0_separable`); a `PSFOperator` (motion blur, a
        measured point-spread function) goes the same way with its own kernel."""
        from .measurements import GRID_OPERATORS
        r0, r1 = self._batch_rows(rows, x0, y)
        mask = self._mask_rows(mask, r0, r1, y.shape[2] * y.shape[3])
        if self._blind_field() is not None:
            if (r0, r1) != (0, self._batch[0]):
                raise ValueError(f"blind_field_blur: the learnt field is shared by the batch -- the data term got rows {r0}:{r1} of the "
                                 f"batch's {self._batch[0]}; it takes ONE call over all its images")
            return self._loss_grad_x0_blind_field(x0, y, g_out, loss_out, mask)
        if self._blind() is not None:
            if self.operator.couples_batch and (r0, r1) != (0, self._batch[0]):
                raise ValueError(f"blind_blur: the learnt PSF is shared by the batch -- the data term got rows {r0}:{r1} of the batch's "
                                 f"{self._batch[0]}; it takes ONE call over all its images")
            return self._loss_grad_x0_blind(x0, y, g_out, loss_out, mask, r0)
        if isinstance(self.operator, GRID_OPERATORS):
            return self._loss_grad_x0_separable(x0, y, g_out, loss_out, mask, r0)
        B, C, HW = x0.shape[0], x0.shape[1], x0.shape[2] * x0.shape[3]
        if y.shape[0] != B or y.shape[1] != 3 or C not in (3, 4):
            raise ValueError("expected x0 [B,4,H,W] or [B,3,H,W] and measurement [B,3,H,W]")
        key = (B, HW, str(x0.device)) if C == 4 else (B, HW, str(x0.device), C)
        st = self._states.get(key)
        if st is None:
            f32 = dict(device=x0.device, dtype=torch.float32)
            if C == 4:
                d = PhysDesc()
                d.kind, d.depth_type, d.weight_type, d.wdepth_type, d.loss_type, d.optimizer = 3, 0, 0, 0, 0, 0
                d.gamma_avrg = d.gamma_val = 0.0
                d.B, d.HW = B, HW
                st = {"desc": d, "part": torch.empty(B * ops.phys_nblk(HW) * 16, **f32), "red": torch.zeros(B * 16, **f32),
                      "loss": torch.zeros(B, **f32), "g": torch.empty(B, 4, HW, **f32), "phi": torch.zeros(B, 9, **f32)}
            else:
                st = {"part": torch.empty(B * ops.phys_nblk(HW), **f32), "loss": torch.zeros(B, **f32),
                      "g": torch.empty(B, C, HW, **f32)}
            while len(self._states) >= 4:
                self._states.pop(next(iter(self._states)))
            self._states[key] = st
        g = g_out if g_out is not None else st["g"]
        loss = loss_out if loss_out is not None else st["loss"]
        if self._robust is not None:    # the robust term: e = y - x0[:, 0:3], its MAD scale, M_eff rows in the mask's place
            mask = self._robust_mask_rows(x0.contiguous(), 1.0, 0.0, y.contiguous(), mask, r0, r1)
        if mask is not None and C == 4:
            ops.phys_optimize_m(st["desc"], x0.contiguous(), y.contiguous(), mask, st["phi"], st["part"], st["red"], loss, g, 1, True)
        elif mask is not None:
            ops.ps_loss_grad_mc(x0.contiguous(), y.contiguous(), mask, st["part"], loss, g, B, C, HW)
        elif C == 4:
            ops.phys_optimize(st["desc"], x0.contiguous(), y.contiguous(), st["phi"], st["part"], st["red"], loss, g, 1, True)
        else:
            ops.ps_loss_grad_c(x0.contiguous(), y.contiguous(), st["part"], loss, g, B, C, HW)
        return g.view(x0.shape), loss

    @staticmethod
    def _weight_rows(w, r0, B):
        """The weight sets of a call on the B images from row r0 of the open batch: those rows of w [nb,nc,T] with one set per image,
        else w."""
        return w[r0:r0 + B] if w.shape[0] > 1 else w

    def _loss_grad_x0_separable(self, x0, y, g_out=None, loss_out=None, mask=None, r0=0):
        """The data term through a separable linear operator, three stream-ordered launches and no host sync:
        Ax = A x0[:, 0:3] (osm_linop_apply, P = 3, image stride C HW); loss[b] = ||M (y - Ax)|| and r = d loss / d Ax (the identity
        term's own reduction, osm_ps_loss_grad_c / _mc at C = 3 on the measurement's h w); g[:, 0:3] = A^T r with the transposed
        tables, any channel beyond the colours written as 0 by the same launch (zero_planes = C - 3).
        A `PSFOperator`: the same three launches with osm_psf_apply in the place of osm_linop_apply, `adjoint` set for A^T; with more
        than one weight set (`per_image` / `per_channel`) osm_psf_apply_s on the weight rows [r0:r0 + B] of the open batch.
        A `PSFFieldOperator` (`field_blur`): the same three launches with osm_psf_field_apply for A and A^T; the field is shared by
        the batch, so a chunk needs no rows of it."""
        from .measurements import PSFFieldOperator, PSFOperator
        B, C, H, W = x0.shape
        h, w = self.operator.out_shape(H, W)
        if C not in (3, 4) or tuple(y.shape) != (B, 3, h, w):
            raise ValueError(f"expected x0 [B,4,H,W] or [B,3,H,W] and measurement [B,3,{h},{w}], got {tuple(x0.shape)} and {tuple(y.shape)}")
        HW, hw = H * W, h * w
        key = ("separable", B, H, W, str(x0.device), C)
        st = self._states.get(key)
        if st is None:
            f32 = dict(device=x0.device, dtype=torch.float32)
            st = {"part": torch.empty(B * ops.phys_nblk(hw), **f32), "loss": torch.zeros(B, **f32), "g": torch.empty(B, C, HW, **f32),
                  "Ax": torch.empty(B, 3, hw, **f32), "r": torch.empty(B, 3, hw, **f32)}
            while len(self._states) >= 4:
                self._states.pop(next(iter(self._states)))
            self._states[key] = st
        g = g_out if g_out is not None else st["g"]
        loss = loss_out if loss_out is not None else st["loss"]
        Ax, r = st["Ax"], st["r"]
        sets = isinstance(self.operator, PSFOperator) and self.operator.weight_sets != (1, 1)
        if isinstance(self.operator, PSFFieldOperator):       # a field is never read as one PSF: its own kernel, same three launches
            taps, (Ry, Rx) = self.operator.taps(x0.device), self.operator.radius()
            tabs = self.operator.field_tables(H, W, x0.device)
            ops.psf_field_apply(x0.contiguous(), Ax, *taps, tabs, Ry, Rx, B, 3, C * HW, 3 * hw, H, W)
        elif isinstance(self.operator, PSFOperator):
            taps, (Ry, Rx) = self.operator.taps(x0.device), self.operator.radius()
            if sets:
                taps = (taps[0], taps[1], self._weight_rows(taps[2], r0, B))
            psf = ops.psf_apply_s if sets else ops.psf_apply
            psf(x0.contiguous(), Ax, *taps, Ry, Rx, B, 3, C * HW, 3 * hw, H, W)
        else:
            tabs = self.operator.tables(H, W, x0.device)
            ops.linop_apply(x0.contiguous(), Ax, *tabs["fwd"], B, 3, C * HW, 3 * hw, H, W)
        if mask is not None:
            ops.ps_loss_grad_mc(Ax, y.contiguous(), mask, st["part"], loss, r, B, 3, hw)
        else:
            ops.ps_loss_grad_c(Ax, y.contiguous(), st["part"], loss, r, B, 3, hw)
        if isinstance(self.operator, PSFFieldOperator):
            ops.psf_field_apply(r, g, *taps, tabs, Ry, Rx, B, 3, 3 * hw, C * HW, H, W, adjoint=True, zero_planes=C - 3)
        elif isinstance(self.operator, PSFOperator):
            psf(r, g, *taps, Ry, Rx, B, 3, 3 * hw, C * HW, H, W, adjoint=True, zero_planes=C - 3)
        else:
            ops.linop_apply(r, g, *tabs["adj"], B, 3, 3 * hw, C * HW, h, w, zero_planes=C - 3)
        return g.view(x0.shape), loss

    def _loss_grad_x0_blind(self, x0, y, g_out=None, loss_out=None, mask=None, r0=0):
        """The data term through a `blind_blur` operator that learns its PSF: ONE call over the whole batch (the PSF is shared) -- or,
        with `per_image`, over any rows [r0:r0 + B] of it, each image stepping its own weight row (osm_ps_blind_optimize_s and the `_s`
        single launches, include/osmosis_psfset.h; `per_channel`: one set per colour plane) -- the
        operator's n_iter inner iterations of  Ax = A(w) x0[:, 0:3];  loss, r = d loss / d Ax;  the tap gradient c = corr(r, x0);
        on the last iteration g[:, 0:3] = A(w)^T r;  the projected step of w  -- enqueued by one C call (osm_ps_blind_optimize,
        5 n_iter + 1 launches, no host sync); OSM_PHYS_PY_LOOP=1 walks the single-launch entry points.  loss and g are those before
        the last step of w, as the Osmosis conditioner treats phi."""
        op = self.operator
        B, C, H, W = x0.shape
        op.out_shape(H, W)
        if C not in (3, 4) or tuple(y.shape) != (B, 3, H, W):
            raise ValueError(f"expected x0 [B,4,H,W] or [B,3,H,W] and measurement [B,3,{H},{W}], got {tuple(x0.shape)} and {tuple(y.shape)}")
        HW = H * W
        dy, dx, w = op.taps(x0.device)
        Ry, Rx = op.radius()
        sets = op.weight_sets != (1, 1)
        if sets:
            w = self._weight_rows(w, r0, B)
        T, nparts = int(dy.numel()), ops.tap_grad_nparts(3, H, W)
        key = ("blind", B, H, W, str(x0.device), C)
        st = self._states.get(key)
        if st is None or st["tpart"].numel() < B * nparts * T:
            f32 = dict(device=x0.device, dtype=torch.float32)
            st = {"part": torch.empty(B * ops.phys_nblk(HW), **f32), "loss": torch.zeros(B, **f32), "g": torch.empty(B, C, HW, **f32),
                  "Ax": torch.empty(B, 3, HW, **f32), "r": torch.empty(B, 3, HW, **f32), "tpart": torch.empty(B * nparts * T, **f32)}
            self._states.pop(key, None)
            while len(self._states) >= 4:
                self._states.pop(next(iter(self._states)))
            self._states[key] = st
        g = g_out if g_out is not None else st["g"]
        loss = loss_out if loss_out is not None else st["loss"]
        x0, y = x0.contiguous(), y.contiguous()
        Ax, r, tpart = st["Ax"], st["r"], st["tpart"]
        if sets:
            apply, fused = ops.psf_apply_s, ops.ps_blind_optimize_s
        else:
            apply, fused = ops.psf_apply, ops.ps_blind_optimize
        if os.environ.get("OSM_PHYS_PY_LOOP", "0") != "1":
            fused(x0, y, mask, dy, dx, w, Ry, Rx, B, C, H, W, Ax, r, st["part"], tpart, loss, g, op.n_iter, op.eta, op.l1)
            return g.view(x0.shape), loss
        for it in range(op.n_iter):
            apply(x0, Ax, dy, dx, w, Ry, Rx, B, 3, C * HW, 3 * HW, H, W)
            if mask is not None:
                ops.ps_loss_grad_mc(Ax, y, mask, st["part"], loss, r, B, 3, HW)
            else:
                ops.ps_loss_grad_c(Ax, y, st["part"], loss, r, B, 3, HW)
            ops.psf_tap_grad(x0, r, dy, dx, Ry, Rx, B, 3, C * HW, 3 * HW, H, W, tpart)
            if it == op.n_iter - 1:
                apply(r, g, dy, dx, w, Ry, Rx, B, 3, 3 * HW, C * HW, H, W, adjoint=True, zero_planes=C - 3)
            if sets:
                ops.psf_tap_step_s(w, tpart, loss, B, 3, nparts // 3, 3 * HW, op.eta, op.l1, per_image=w.shape[0] > 1,
                                   per_channel=w.shape[1] > 1)
            else:
                ops.psf_tap_step(w, tpart, loss, B, nparts, 3 * HW, op.eta, op.l1)
        return g.view(x0.shape), loss

    def _loss_grad_x0_blind_field(self, x0, y, g_out=None, loss_out=None, mask=None):
        """The data term through a `blind_field_blur` operator that learns its field: ONE call over the whole batch (the field is
        shared), the operator's n_iter inner iterations of  Ax = A(w) x0[:, 0:3] (osm_psf_field_apply);  loss, r = d loss / d Ax
        (osm_ps_loss_grad_c / _mc);  the per-node tap partials of (r, x0) (osm_field_tap_grad);  on the last iteration
        g[:, 0:3] = A(w)^T r, planes beyond the colours written as 0;  the projected step of every node (osm_field_tap_step).  The
        sub-step has no entry point of its own: it is enqueued here, stream-ordered, no host sync (include/osmosis_blindfield.h).
        loss and g are those before the last step of w, as the Osmosis conditioner treats phi."""
        op = self.operator
        B, C, H, W = x0.shape
        op.out_shape(H, W)
        if C not in (3, 4) or tuple(y.shape) != (B, 3, H, W):
            raise ValueError(f"expected x0 [B,4,H,W] or [B,3,H,W] and measurement [B,3,{H},{W}], got {tuple(x0.shape)} and {tuple(y.shape)}")
        HW = H * W
        dy, dx, w = op.taps(x0.device)
        Ry, Rx = op.radius()
        gh, gw = op.grid
        tabs = op.field_tables(H, W, x0.device)
        lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, 3, x0.device)
        T = int(dy.numel())
        key = ("blind_field", B, H, W, str(x0.device), C)
        st = self._states.get(key)
        if st is None or st["tpart"].numel() < B * NP * T or st["w_new"].shape != w.shape:
            f32 = dict(device=x0.device, dtype=torch.float32)
            st = {"part": torch.empty(B * ops.phys_nblk(HW), **f32), "loss": torch.zeros(B, **f32), "g": torch.empty(B, C, HW, **f32),
                  "Ax": torch.empty(B, 3, HW, **f32), "r": torch.empty(B, 3, HW, **f32), "tpart": torch.empty(B * NP * T, **f32),
                  "w_new": torch.empty_like(w)}
            self._states.pop(key, None)
            while len(self._states) >= 4:
                self._states.pop(next(iter(self._states)))
            self._states[key] = st
        g = g_out if g_out is not None else st["g"]
        loss = loss_out if loss_out is not None else st["loss"]
        x0, y = x0.contiguous(), y.contiguous()
        Ax, r, tpart = st["Ax"], st["r"], st["tpart"]
        for it in range(op.n_iter):
            ops.psf_field_apply(x0, Ax, dy, dx, w, tabs, Ry, Rx, B, 3, C * HW, 3 * HW, H, W)
            if mask is not None:
                ops.ps_loss_grad_mc(Ax, y, mask, st["part"], loss, r, B, 3, HW)
            else:
                ops.ps_loss_grad_c(Ax, y, st["part"], loss, r, B, 3, HW)
            ops.field_tap_grad(x0, r, dy, dx, tabs, lay, NP, gh, gw, Ry, Rx, B, 3, C * HW, 3 * HW, H, W, tpart)
            if it == op.n_iter - 1:
                ops.psf_field_apply(r, g, dy, dx, w, tabs, Ry, Rx, B, 3, 3 * HW, C * HW, H, W, adjoint=True, zero_planes=C - 3)
            ops.field_tap_step(w, st["w_new"], tpart, loss, lay, NP, B, 3 * HW, op.eta, op.l1, op.smooth)
        return g.view(x0.shape), loss

    def conditioning(self, x_prev, x_t, x_0_hat, measurement, **kwargs):
        if self._blind() is not None:
            # the PSF is stepped by kernels, not by autograd: the data term's x0-gradient from `loss_grad_x0`, pulled back through
            # the network by autograd (the form the Osmosis conditioner uses)
            self.hip_ok(x_0_hat.shape[1])
            g, loss = self.loss_grad_x0(x_0_hat.detach(), measurement)
            if x_prev.grad is not None:
                x_prev.grad = None
            x_0_hat.backward(gradient=g.clone(), inputs=[x_prev])
            with torch.no_grad():
                x_t -= x_prev.grad * self.scale[None, ..., None, None].to(x_prev.device)
            return x_t, loss.detach().clone()
        norm_grad, norm = self.grad_and_value(x_prev=x_prev, x_0_hat=x_0_hat, measurement=measurement, **kwargs)
        with torch.no_grad():
            x_t -= norm_grad * self.scale[None, ..., None, None].to(x_prev.device)
        return x_t, norm
