"""The oracle of the Levenberg-Marquardt phi solver (`optimizer: lm`, osm_phys_desc.optimizer = 9; include/osmosis_hip.h and the
DESIGN section "Levenberg-Marquardt phi solver").  The reference has no such solver: this file restates the contract -- the 32
per-image sums, the assembly of the normal equations per operator kind, the damped Cholesky step, the state machine over the
[20]-float state row and the schedule of one call -- in torch / numpy, in float64 (`dtype=torch.float64`) or as a float32
restatement (`dtype=torch.float32`: fp32 pixel math and fp32 sums per 1024-pixel block, fp64 from there on, as the kernels do it).

The state row and phi are float32 in both (they ARE float32 on the device: the contract rounds there), so the two differ only by
the sums.  Every decision is recorded with its margin |S - S_base| / S_base (None where there is no base to compare with).

`LMGuidance` is a subclass of `oracle.diffusion_ref.OsmosisGuidance` for chains (as tests/physgroup_oracle.py does it): the inner
loop is the solver's schedule, the loss and dL/dx0 come from autograd at the accepted phi.
Shared by tests/test_philm_cpu.py and tests/test_philm_gpu.py."""
import math

import numpy as np
import torch

from oracle import diffusion_ref as D

PPB = 1024                       # pixels per reduce workgroup
S_BASE, LAMBDA, RETRY = 9, 10, 11
LAMBDA0, LAMBDA_MIN, LAMBDA_MAX, FACTOR = 1.0, 1e-6, 1e6, 10.0
ACCEPT_SLACK = 1e-5
DIAG_EPS = 1e-12
KINDS = {"underwater_physical_revised": 0, "underwater_physical": 1, "haze_physical": 2}


def live_slots(kind, eta3):
    """The phi slots the solver steps: those of `phys_param_lr` with a non-zero eta (kinds 1, 2 have no phi_b)."""
    ea, eb, ei = eta3
    a = {0: [0, 1, 2], 1: [0, 1, 2], 2: [0]}[kind] if ea != 0 else []
    b = [3, 4, 5] if (kind == 0 and eb != 0) else []
    return a + b + ([6, 7, 8] if ei != 0 else [])


def _depth(Dp, depth_type, value):
    if isinstance(value, np.ndarray):
        value = [float(v) for v in value]
    if depth_type == "gamma" and value[2] == 1.0:
        return (Dp + value[0]) * value[1]
    return D.convert_depth(Dp, depth_type, value)


def lm_sums(kind, phi9, x0, y, mask, depth, weight, dtype=torch.float64):
    """The 32 sums of one image at phi9 (float32 [9]): x0 [4,H,W], y [3,H,W], mask [3,H,W] or [1,H,W] or None; depth = (depth_type,
    value), weight = None or (depth_type, value).  Slots 0..13 as osm_phys_reduce leaves them, 14 + 6 c + (aa, ab, ai, bb, bi, ii).
    float32: the sums of every 1024-pixel block in float32, the blocks added in float64.  Returns float64 [32]."""
    x = x0.to(dtype).reshape(4, -1)
    yy = y.to(dtype).reshape(3, -1)
    rgb, Dp = x[0:3], x[3:4]
    d = _depth(Dp, *depth)
    w = torch.ones_like(d) if weight is None else _depth(Dp, *weight)
    wm = w.expand(3, -1) if mask is None else w * mask.to(dtype).reshape(mask.shape[0], -1).expand(3, -1)
    ph = torch.as_tensor(np.asarray(phi9, dtype=np.float32)).to(dtype)
    pa = (ph[0:1].expand(3) if kind == 2 else ph[0:3]).reshape(3, 1)
    pb = ph[3:6].reshape(3, 1) if kind == 0 else pa
    pinf = ph[6:9].reshape(3, 1)
    Ea, Eb, J = torch.exp(-pa * d), torch.exp(-pb * d), 0.5 * (rgb + 1.0)
    I = J * Ea + pinf * (1.0 - Eb)
    r = (yy - (2.0 * I - 1.0)) * wm
    k2 = -2.0 * wm * r
    ca, cb, ci = -d * J * Ea, pinf * d * Eb, 1.0 - Eb
    e = torch.clamp(rgb.abs() - 0.7, min=0.0)
    w4 = 4.0 * wm * wm
    rows = [(r * r).sum(0)] + [(k2 * ca)[c] for c in range(3)] + [(k2 * cb)[c] for c in range(3)] + [(k2 * ci)[c] for c in range(3)] \
        + [rgb[c] for c in range(3)] + [(e * e).sum(0)]
    for c in range(3):
        rows += [(w4 * ca * ca)[c], (w4 * ca * cb)[c], (w4 * ca * ci)[c], (w4 * cb * cb)[c], (w4 * cb * ci)[c], (w4 * ci * ci)[c]]
    T = torch.stack(rows)                                        # [32, HW]
    if dtype == torch.float64:
        return T.sum(dim=1).numpy()
    HW = T.shape[1]
    pad = (-HW) % PPB
    T = torch.nn.functional.pad(T, (0, pad)).reshape(32, -1, PPB)
    return T.sum(dim=2).double().sum(dim=1).numpy()             # fp32 per block, fp64 across the blocks


def assemble(kind, tot):
    """A [9,9] over the phi slots and g = J^T r [9] from the totals (fp64)."""
    A, g = np.zeros((9, 9)), np.zeros(9)
    for c in range(3):
        aa, ab, ai, bb, bi, ii = (float(v) for v in tot[14 + 6 * c:20 + 6 * c])
        pi = 6 + c
        if kind == 0:
            pa, pb = c, 3 + c
            A[pa, pa] = aa
            A[pa, pb] = A[pb, pa] = ab
            A[pa, pi] = A[pi, pa] = ai
            A[pb, pb] = bb
            A[pb, pi] = A[pi, pb] = bi
            g[pa], g[pb] = tot[1 + c], tot[4 + c]
        else:
            pa = c if kind == 1 else 0
            A[pa, pa] += aa + 2.0 * ab + bb
            A[pa, pi] += ai + bi
            A[pi, pa] = A[pa, pi]
            g[pa] += tot[1 + c] + tot[4 + c]
        A[pi, pi] = ii
        g[pi] = tot[7 + c]
    return A, g


def solve(kind, tot, live, lam):
    """delta [9] of (A + lam (diag A + eps max diag A)) delta = -J^T r over the live slots, by Cholesky; None on a non-positive pivot
    or a non-finite result."""
    A, g = assemble(kind, tot)
    A, g = A[np.ix_(live, live)], g[live]
    dg = np.diag(A).copy()
    A = A + lam * np.diag(dg + DIAG_EPS * dg.max())
    n = len(live)
    L = np.zeros((n, n))
    for k in range(n):
        dk = A[k, k] - float(L[k, :k] @ L[k, :k])
        if not (dk > 0.0) or not math.isfinite(dk):
            return None
        L[k, k] = math.sqrt(dk)
        for r in range(k + 1, n):
            L[r, k] = (A[r, k] - float(L[r, :k] @ L[k, :k])) / L[k, k]
    z = np.zeros(n)
    for k in range(n):
        z[k] = (-g[k] - float(L[k, :k] @ z[:k])) / L[k, k]
    dl = np.zeros(n)
    for k in range(n - 1, -1, -1):
        dl[k] = (z[k] - float(L[k + 1:, k] @ dl[k + 1:])) / L[k, k]
    if not np.isfinite(dl).all():
        return None
    delta = np.zeros(9)
    delta[live] = dl
    return delta


def new_state(lm_lambda=None):
    st = np.zeros(20, dtype=np.float32)
    if lm_lambda is not None:
        st[LAMBDA] = lm_lambda
    return st


def finalize(kind, live, phi9, st, tot, mode, record=None):
    """One LM finalize on the totals `tot` (fp64) at phi9: mode 2 the first decision of a call, 1 a later one, 3 the close (decide
    only).  phi9 (float32 [9]) and st (float32 [20]) are updated in place.  Returns S as the call reports it (S_base after a close that
    rejected)."""
    S = float(tot[0])
    used = list(range(0, 10)) + ([] if mode == 3 else list(range(14, 32)))
    finite = bool(np.isfinite(np.asarray(tot)[used]).all())
    if finite and S == 0.0:
        return S
    lam = float(st[LAMBDA])
    if not (lam > 0.0) or not math.isfinite(lam):
        lam = LAMBDA0
    lam = min(max(lam, LAMBDA_MIN), LAMBDA_MAX)
    nobase = mode == 2 or not (st[S_BASE] > 0)
    retry = st[RETRY] != 0
    reject = True if not finite else not (nobase or S <= (1.0 + ACCEPT_SLACK) * float(st[S_BASE]))
    rec = {"mode": mode, "S": S, "S_base": None if nobase else float(st[S_BASE]), "lambda": lam, "accept": not reject, "retry": bool(retry),
           "margin": None if (nobase or not finite) else abs(S - float(st[S_BASE])) / float(st[S_BASE])}
    restored = False
    if not reject:
        st[0:9] = phi9
        st[S_BASE] = S
        if not retry:
            lam = max(lam / FACTOR, LAMBDA_MIN)
        st[RETRY] = 0
        if mode != 3 and any(float(tot[k]) != 0.0 for k in range(1, 10)):
            delta = solve(kind, tot, live, lam)
            new = None if delta is None else (phi9.astype(np.float64) + delta).astype(np.float32)
            if new is not None and np.isfinite(new).all():
                phi9[:] = new
                if kind == 2:
                    phi9[1] = phi9[2] = phi9[0]
            else:
                lam = min(lam * FACTOR, LAMBDA_MAX)
                st[RETRY] = 1
    elif nobase:
        st[0:9] = phi9
        st[S_BASE] = -1
        st[RETRY] = 0
    else:
        lam = min(lam * FACTOR, LAMBDA_MAX)
        phi9[:] = st[0:9]
        st[RETRY] = 1
        restored = True
    st[LAMBDA] = lam
    rec["lambda_out"] = float(st[LAMBDA])
    if record is not None:
        record.append(rec)
    return float(st[S_BASE]) if (mode == 3 and restored) else S


def lm_call(kind, live, phi9, st, x0, y, mask, depth, weight, n_iter, dtype=torch.float64, record=None):
    """The schedule of one call on one image: n_iter x { sums; finalize that decides and steps }, then the closing evaluation.  phi9
    and st are updated in place; returns the S the loss is taken from (at the accepted phi)."""
    for it in range(n_iter):
        finalize(kind, live, phi9, st, lm_sums(kind, phi9, x0, y, mask, depth, weight, dtype), 2 if it == 0 else 1, record)
    return finalize(kind, live, phi9, st, lm_sums(kind, phi9, x0, y, mask, depth, weight, dtype), 3, record)


def pack_phi(op, B):
    """[B,9] float32 = phi_a | phi_b | phi_inf from a `D.PhysOperator` (kinds 1, 2: phi_ab in both places, haze's repeated)."""
    out = np.zeros((B, 9), dtype=np.float32)
    for b in range(B):
        if op.kind == "underwater_physical_revised":
            a, bb = op.phi["phi_a"][b].reshape(-1), op.phi["phi_b"][b].reshape(-1)
        else:
            a = bb = op.phi["phi_ab"][b].reshape(-1).expand(3)
        out[b] = np.concatenate([a.detach().numpy(), bb.detach().numpy(), op.phi["phi_inf"][b].reshape(-1).detach().numpy()])
    return out


class LMGuidance(D.OsmosisGuidance):
    """The oracle's guidance with the LM solver in the place of the first-order inner loop, per image: `n_iter` decide-and-step
    iterations and the closing evaluation on x_0_hat (detached: phi is solved for, not back-propagated through), then the total
    = sum over the images of (L_b + aux(x0[b])) at the accepted phi and its gradient into x_prev by autograd.  `mask` [B,3,H,W] or
    broadcastable (None: no mask); `state` [B,20] float32 and `phi9` [B,9] float32 persist across calls; `records[b]` collects every
    decision.  `dtype`: what the sums are taken in."""

    def __init__(self, operator, lm_lambda=None, mask=None, dtype=torch.float64, **kw):
        super().__init__(operator, **kw)
        B = next(iter(operator.phi.values())).shape[0]
        self.kind = KINDS[operator.kind]
        eta = operator.eta
        self.eta3 = (eta["phi_a"], eta["phi_b"], eta["phi_inf"]) if self.kind == 0 else (eta["phi_ab"], 0.0, eta["phi_inf"])
        self.live = live_slots(self.kind, self.eta3)
        self.mask, self.dtype = mask, dtype
        self.phi9 = pack_phi(operator, B)
        self.state = np.stack([new_state(lm_lambda) for _ in range(B)])
        self.records = [[] for _ in range(B)]
        self.depth = (operator.depth_type, operator.value)
        if self.loss_weight in (None, "none"):
            self.weight = None
        else:
            parts = self.weight_function.split(",")
            self.weight = (parts[0], [float(v) for v in parts[1:]])

    def _sync(self):
        with torch.no_grad():
            p = torch.from_numpy(self.phi9.copy())
            if self.kind == 0:
                self.op.phi["phi_a"].copy_(p[:, 0:3, None, None])
                self.op.phi["phi_b"].copy_(p[:, 3:6, None, None])
            else:
                n = self.op.phi["phi_ab"].shape[1]
                self.op.phi["phi_ab"].copy_(p[:, 0:n, None, None])
            self.op.phi["phi_inf"].copy_(p[:, 6:9, None, None])

    def _mask_of(self, b, B):
        if self.mask is None:
            return None
        return self.mask[b] if self.mask.shape[0] == B else self.mask[0]

    def solve_phi(self, x0, y):
        B = x0.shape[0]
        for b in range(B):
            lm_call(self.kind, self.live, self.phi9[b], self.state[b], x0[b], y[b], self._mask_of(b, B), self.depth, self.weight,
                    self.n_iter, self.dtype, self.records[b])
        self._sync()

    def loss(self, x0, y):
        I = self.op.forward(x0)
        diff = (y.to(I.dtype) - (2 * I - 1)) * self._weight(x0)
        if self.mask is not None:
            diff = diff * self.mask.to(I.dtype)
        if self.loss_function == "norm":
            per = torch.linalg.vector_norm(diff, dim=(1, 2, 3))
        else:
            per = (diff ** 2).mean(dim=(1, 2, 3))
        return per.detach().numpy(), per.sum()

    def total(self, x0, y):
        sep, loss = self.loss(x0, y)
        if self.aux:
            loss = loss + sum(D.aux_loss(x0[b:b + 1], self.aux) for b in range(x0.shape[0]))
        return sep, loss

    def conditioning(self, x_prev, x_t, x_0_hat, y, freeze_phi):
        self.op.set_requires_grad(False)
        if not freeze_phi:
            self.solve_phi(x_0_hat.detach(), y)
        sep, total = self.total(x_0_hat, y)
        total.backward(inputs=[x_prev])
        with torch.no_grad():
            g = x_prev.grad
            gc = torch.clamp(g, -self.clip, self.clip) if self.clip is not None else g
            x_t -= self.scale[None, :, None, None] * gc
        return x_t, sep, self.op.variables(), g.detach().clone()

    def loss_grad_x0(self, x0, y, freeze_phi=False):
        """One call on x0 [B,4,H,W] (float64): (per-image loss [B], dL/dx0 [B,4,H,W]); phi9 / state / records move on."""
        xb = x0.clone().requires_grad_(True)
        if not freeze_phi:
            self.solve_phi(x0, y)
        sep, total = self.total(xb, y)
        total.backward(inputs=[xb])
        return np.asarray(sep, dtype=np.float64), xb.grad.detach().clone()


def make_guidance(opname, okw, n_iter, B=1, lm_lambda=None, mask=None, aux=None, loss_function="norm", loss_weight="depth",
                  dtype=torch.float64, scale="7,7,7,0.9", gradient_clip="False,0"):
    op = D.PhysOperator(opname, batch_size=B, **okw)
    return LMGuidance(op, lm_lambda=lm_lambda, mask=mask, dtype=dtype, n_iter=n_iter, scale=scale, gradient_clip=gradient_clip, aux=aux,
                      loss_function=loss_function, loss_weight=loss_weight)


# ---------------------------------------------------------------------------------------------------------------- the seeded scene
SCENE_OKW = {
    "underwater_physical_revised": dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8",
                                        phi_inf="0.14, 0.29, 0.49"),
    "underwater_physical": dict(depth_type="gamma", value="1.4,1.4,1", phi_ab="1.1,0.95,0.95", phi_inf="0.14, 0.29, 0.49"),
    "haze_physical": dict(depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_inf="0.14, 0.29, 0.49"),
}
SCENE_TRUTH = {
    "underwater_physical_revised": dict(phi_a="0.8,0.6,0.5", phi_b="0.7,0.5,0.45", phi_inf="0.10,0.35,0.55"),
    "underwater_physical": dict(phi_ab="0.8,0.6,0.5", phi_inf="0.10,0.35,0.55"),
    "haze_physical": dict(phi_ab="0.7", phi_inf="0.20,0.35,0.55"),
}


def scene(opname, seed, H=36, W=34, B=1, noise=0.02, masked=False):
    """A synthetic scene: a smooth-ish clean image and depth, the photo rendered at SCENE_TRUTH with `noise` (in [0, 1] units) added.
    Returns (x0 [B,4,H,W], y [B,3,H,W] in [-1, 1], mask or None), float64."""
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)
    x0[:, 3] = (torch.rand(B, H, W, generator=g, dtype=torch.float64) * 1.8 - 0.9)
    op = D.PhysOperator(opname, batch_size=B, depth_type="gamma", value="1.4,1.4,1", **SCENE_TRUTH[opname])
    I = op.forward(x0) + noise * torch.randn(B, 3, H, W, generator=g, dtype=torch.float64)
    y = 2.0 * I - 1.0
    mask = None
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * (torch.rand(B, 1, H, W, generator=g) > 0.3).double()
    return x0, y, mask


def data_S(opname, phi_kw, x0, y, mask, loss_weight="depth"):
    """Sum r^2 per image at the parameters `phi_kw`, fp64."""
    B = x0.shape[0]
    gd = make_guidance(opname, dict(depth_type="gamma", value="1.4,1.4,1", **phi_kw), 1, B=B, mask=mask, loss_weight=loss_weight)
    return np.array([lm_sums(gd.kind, gd.phi9[b], x0[b], y[b], gd._mask_of(b, B), gd.depth, gd.weight)[0] for b in range(B)])


# ---------------------------------------------------------------------------------------------------------------- the parity cases
# What tests/test_philm_gpu.py compares the device with, and what tests/test_philm_cpu.py checks the oracle alone on: every compared
# decision of a case (one with a base, outside the re-evaluation that follows a reject) must have a margin >= MIN_MARGIN in the
# fp64 oracle, so that no rounding of a sum can flip it.  The re-evaluation after a reject is exempt BY CONSTRUCTION: it evaluates
# at phi_base itself, S equals S_base up to the float32 rounding of the stored S_base (6e-8), and the accept slack of 1e-5 decides it
# the same way on every implementation -- the tie the slack exists for.
MIN_MARGIN = 1e-3
AUX = {"avrg_loss": 0.5, "val_loss": 20}


def case(name, opname, loss_function, loss_weight, masked, aux, seed, B=2, H=36, W=34, n_iter=4, lm_lambda=None, calls=1, **eta):
    return dict(name=name, opname=opname, loss_function=loss_function, loss_weight=loss_weight, masked=masked, aux=aux, seed=seed, B=B,
                H=H, W=W, n_iter=n_iter, lm_lambda=lm_lambda, calls=calls, eta=eta)


def case_inputs(c, call=0):
    """(x0, y, mask) of a case's call: the seeded scene of its operator, B distinct images; a later call draws another x0 (the
    sub-step's prediction has moved) for the same photo and mask."""
    x0, y, mask = scene(c["opname"], c["seed"], c["H"], c["W"], c["B"], masked=c["masked"])
    if call > 0:
        g = torch.Generator().manual_seed(7000 + 13 * c["seed"] + call)
        x0 = (x0 + 0.25 * torch.randn(x0.shape, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)
    # (float32 values: what the device is handed)
    return x0.float().double(), y.float().double(), None if mask is None else mask.float().double()


def case_okw(c):
    return dict(SCENE_OKW[c["opname"]], **c["eta"])


def run_case(c, dtype=torch.float64):
    """The oracle on a case: [(loss [B], g [B,4,H,W], phi9 [B,9], state [B,20]) per call] and the guidance (its records)."""
    gd, out = None, []
    for k in range(c["calls"]):
        x0, y, mask = case_inputs(c, k)
        if gd is None:
            gd = make_guidance(c["opname"], case_okw(c), c["n_iter"], B=c["B"], lm_lambda=c["lm_lambda"], mask=mask,
                               aux=AUX if c["aux"] else None, loss_function=c["loss_function"], loss_weight=c["loss_weight"], dtype=dtype)
        sep, g = gd.loss_grad_x0(x0, y)
        out.append((sep, g, gd.phi9.copy(), gd.state.copy()))
    return out, gd


def compared_margins(gd):
    """The margins of every compared decision of a guidance's records (see MIN_MARGIN)."""
    return [r["margin"] for rs in gd.records for r in rs if r["margin"] is not None and not r["retry"]]


_R, _U, _HZ = "underwater_physical_revised", "underwater_physical", "haze_physical"
# The three kinds x norm / mse x no weight / depth weight x mask / none, cycled; B = 2 distinct images at 36 x 34 (two reduce
# workgroups, a ragged tail of 200 pixels, an odd count per wave) and one case at 74 x 58 (five workgroups).  n_iter = 4.  lm_lambda:
# the default 1 where the margins of the fp64 oracle allow it; 100 where the operator has so few parameters that a start at
# lambda = 1 has converged by the fourth decision (its last decisions would be ties, margins 1e-8 .. 1e-5); seeds likewise.
PARITY_CASES = [
    case("revised.norm.depth.aux", _R, "norm", "depth", False, True, 0),
    case("uw.mse.none.mask", _U, "mse", "none", True, False, 0, lm_lambda=100.0),
    case("haze.norm.depth.mask.aux", _HZ, "norm", "depth", True, True, 2, lm_lambda=100.0),
    case("revised.mse.none.mask", _R, "mse", "none", True, False, 3),
    case("uw.norm.depth.aux", _U, "norm", "depth", False, True, 0, lm_lambda=100.0),
    case("haze.mse.none", _HZ, "mse", "none", False, False, 0, lm_lambda=100.0),
    case("revised.74x58.mask.aux", _R, "norm", "depth", True, True, 2, B=1, H=74, W=58),
    case("revised.frozen_phi_b", _R, "norm", "depth", False, False, 0, lm_lambda=100.0, phi_b_eta=0.0),
    case("revised.reject_path", _R, "norm", "depth", False, False, 2, lm_lambda=1e-3, n_iter=8),
]
# two consecutive calls (lambda and the base carry over; the second call's x0 has moved and its second step is rejected)
TWO_CALLS = case("revised.two_calls.mask", _R, "norm", "depth", True, False, 3, lm_lambda=10.0, n_iter=2, calls=2)
