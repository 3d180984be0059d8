"""The oracle of the learnt vignetting gain field (include/osmosis_gain.h; the reference has no such term, the header is the
contract), torch / numpy float64 round the project's masked guidance oracle (tests/physgroup_oracle.py), from the same fp32 tables:

    G = Hy n Hx^T  (the bilinear interpolation of the nodes);  r_c = (y_c - (2 G F_c - 1)) w M0_c;  S = sum r^2
    c_raw = Hy^T (sum_c r_c (-2 F_c w M0_c)) Hx;  c = gscale c_raw;  the projected step with the gauge max n = 1
    the data term: the masked oracle on y' = (y + 1) / G - 1 with the mask M0 G

`expand32` / `field32` are the float32 restatements of the stated operation order that the expand kernel is held to bit for bit.
Shared by tests/test_gain_cpu.py and tests/test_gain_gpu.py."""
import numpy as np
import torch

from oracle import diffusion_ref as D
import physgroup_oracle as GO

U23 = 2.0 ** -23


# ----------------------------------------------------------------------------- tables and the field
def tables(H, W, gh, gw):
    """(iy0 [H] int32, fy [H] fp32, ix0 [W] int32, fx [W] fp32): positions in float64, fractions rounded to fp32."""
    def axis(n, g):
        pos = np.arange(n, dtype=np.float64) * (g - 1) / (n - 1)
        i0 = np.minimum(np.floor(pos), g - 2).astype(np.int32)
        return i0, (pos - i0).astype(np.float32)
    return axis(H, gh) + axis(W, gw)


def hat_matrix(i0, f, g, fp32=False):
    """[n, g] float64: row x holds 1 - f at column i0[x] and f at i0[x] + 1; 1 - f exact in float64 from the fp32 f, or with `fp32`
    rounded to fp32 first, as the kernels hold the hat weights."""
    n = i0.shape[0]
    Hm = np.zeros((n, g), dtype=np.float64)
    Hm[np.arange(n), i0] += (np.float32(1.0) - f).astype(np.float64) if fp32 else 1.0 - f.astype(np.float64)
    Hm[np.arange(n), i0 + 1] += f.astype(np.float64)
    return Hm


def hats(tabs, gh, gw):
    iy0, fy, ix0, fx = tabs
    return torch.from_numpy(hat_matrix(iy0, fy, gh)), torch.from_numpy(hat_matrix(ix0, fx, gw))


def field64(nodes, tabs):
    """G [B,1,H,W] float64 (differentiable) from nodes [B,gh,gw]."""
    Hy, Hx = hats(tabs, nodes.shape[1], nodes.shape[2])
    return (Hy @ nodes.double() @ Hx.T)[:, None]


def field32(nodes, tabs):
    """G [B,H,W] in float32, the header's operation order, every product and sum rounded once."""
    iy0, fy, ix0, fx = tabs
    n = np.asarray(nodes, dtype=np.float32)
    one = np.float32(1.0)
    a, b = (one - fx)[None, None, :], (one - fy)[None, :, None]
    f, g = fx[None, None, :], fy[None, :, None]
    iy, ix = iy0[:, None], ix0[None, :]
    n00, n01, n10, n11 = n[:, iy, ix], n[:, iy, ix + 1], n[:, iy + 1, ix], n[:, iy + 1, ix + 1]
    top = a * n00 + f * n01
    bot = a * n10 + f * n11
    return (b * top + g * bot).astype(np.float32)


def expand32(nodes, tabs, y, M0):
    """(y' [B,3,H,W], M' [B,3,H,W], G [B,H,W]) float32 restatement of the expand (numpy float32 arithmetic rounds every operation)."""
    G = field32(nodes, tabs)
    y = np.asarray(y, dtype=np.float32)
    one = np.float32(1.0)
    with np.errstate(all="ignore"):
        ye = (y + one) / G[:, None] - one
        me = np.broadcast_to(G[:, None], y.shape).copy() if M0 is None else np.asarray(M0, dtype=np.float32) * G[:, None]
    return ye.astype(np.float32), me.astype(np.float32), G


# ----------------------------------------------------------------------------- gradient and step
def grad64(nodes, tabs, F, w, y, M0, loss_function):
    """float64 (c [B,gh,gw], c_raw, S [B], bound_c [B,gh,gw], bound_S [B]) from nodes [B,gh,gw], F [B,3,H,W], w [B,1,H,W] or 1,
    y [B,3,H,W], M0 [B,3,H,W] or None; the bounds are the header's."""
    nodes, F, y = (torch.as_tensor(v).double() for v in (nodes, F, y))
    B, _, H, W = y.shape
    gh, gw = nodes.shape[1:]
    w = torch.ones(B, 1, H, W, dtype=torch.float64) if not torch.is_tensor(w) else w.double().expand(B, 1, H, W)
    M = torch.ones_like(y) if M0 is None else torch.as_tensor(M0).double().expand_as(y)
    Hy, Hx = hats(tabs, gh, gw)
    G = field64(nodes, tabs)
    e = y - (2 * G * F - 1)
    r = e * w * M
    dd = -2 * F * w * M
    q = (r * dd).sum(dim=1)
    S = (r * r).sum(dim=(1, 2, 3))
    c_raw = Hy.T @ q @ Hx
    gscale = 1.0 / torch.sqrt(S) if loss_function == "norm" else torch.full((B,), 2.0 / (3 * H * W), dtype=torch.float64)
    c = gscale[:, None, None] * c_raw
    dr = w * M * (14 * (G * F).abs() + (2 * G * F - 1).abs() + 3 * e.abs())
    Kx = int(max(((tabs[2] == j) | (tabs[2] == j - 1)).sum() for j in range(gw)))
    bc = U23 * (Hy.T @ (dd.abs() * dr + (Kx + 8) * (r * dd).abs()).sum(dim=1) @ Hx)
    bS = U23 * (2 * r.abs() * dr + (3 * ((W + 63) // 64) + 7) * r * r).sum(dim=(1, 2, 3))
    return c, c_raw, S, bc, bS


def laplacian(n):
    """Ln [.., gh, gw]: the gradient of 1/2 sum_edges (n_i - n_j)^2 on the 4-neighbour graph."""
    L = np.zeros_like(n)
    L[..., 1:, :] += n[..., 1:, :] - n[..., :-1, :]
    L[..., :-1, :] += n[..., :-1, :] - n[..., 1:, :]
    L[..., :, 1:] += n[..., :, 1:] - n[..., :, :-1]
    L[..., :, :-1] += n[..., :, :-1] - n[..., :, 1:]
    return L


def step64(nodes, c_raw, S, loss_function, HW, eta, lam, g_min):
    """The header's step per image in numpy float64: nodes [B,gh,gw] (float32 values), c_raw [B,gh,gw], S [B] -> nodes float64."""
    n = np.asarray(nodes, dtype=np.float64).copy()
    c_raw, S = np.asarray(c_raw, dtype=np.float64), np.asarray(S, dtype=np.float64)
    eta, lam, g_min = (float(np.float32(v)) for v in (eta, lam, g_min))
    for b in range(n.shape[0]):
        if not np.isfinite(S[b]) or (loss_function == "norm" and S[b] == 0.0):
            continue
        gscale = 1.0 / np.sqrt(S[b]) if loss_function == "norm" else 2.0 / (3.0 * HW)
        with np.errstate(all="ignore"):
            v = n[b] - eta * (gscale * c_raw[b] + lam * laplacian(n[b]))
        u = np.where(v < g_min, g_min, v)
        m = u.max() if not np.isnan(u).any() else np.nan
        if not np.isfinite(m):
            continue
        nn = u / m
        n[b] = np.where(nn < g_min, g_min, nn)
    return n


def learn64(nodes, tabs, F, w, y, M0, loss_function, eta=0.01, n_iter=1, smooth=0.0, g_min=0.05, fp32_nodes=True, with_raw=False):
    """One sub-step's n_iter x (gradient, step) in float64; fp32_nodes: the nodes rounded to float32 after every step, as the
    kernels store them.  Returns nodes [B,gh,gw] float64; with_raw: (nodes, the last step's nodes before that rounding)."""
    n = raw = np.asarray(nodes, dtype=np.float64)
    H, W = y.shape[-2:]
    for _ in range(n_iter):
        _, c_raw, S, _, _ = grad64(torch.from_numpy(n), tabs, F, w, y, M0, loss_function)
        n = raw = step64(n, c_raw.numpy(), S.numpy(), loss_function, H * W, eta, smooth, g_min)
        if fp32_nodes:
            n = n.astype(np.float32).astype(np.float64)
    return (n, raw) if with_raw else n


# ----------------------------------------------------------------------------- composition with the masked guidance oracle
GAIN_DEFAULT = dict(grid=(5, 5), eta=0.01, n_iter=1, smooth=0.0, g_min=0.05, learn=True)


def model_image(opname, okw, x0, loss_weight, weight_function="gamma,1.4,1.4,1", phi=None, dtype=torch.float64):
    """(F [n,3,H,W], w [n,1,H,W] or 1) of the operator at its starting phi (`okw`, or `phi`: {name: tensor})."""
    op = D.PhysOperator(opname, batch_size=1, **okw)
    if phi is not None:
        for k in op.phi:
            op.phi[k] = phi[k].detach().clone()
    guide = D.OsmosisGuidance(op, loss_weight=loss_weight, weight_function=weight_function)
    with torch.no_grad():
        x = x0.to(dtype)
        return op.forward(x).to(dtype), (guide._weight(x) if loss_weight == "depth" else 1)


def substep_nodes(nodes, tabs, F, w, y, mask, loss_function, gain, freeze_phi=False, fp32=False, with_raw=False):
    """The nodes after the sub-step's learning (unchanged with learn off or freeze_phi).  fp32: F, w, y rounded to float32 first and
    the residual formed from float32 operands (the oracle's own float64-versus-float32 distance).  with_raw: as `learn64`."""
    if freeze_phi or not gain.get("learn", True):
        n = np.asarray(nodes, dtype=np.float64)
        return (n, n) if with_raw else n
    if fp32:
        F, y = F.float().double(), y.float().double()
        w = w.float().double() if torch.is_tensor(w) else w
    return learn64(nodes, tabs, F, w, y, mask, loss_function, gain["eta"], gain["n_iter"], gain["smooth"], gain["g_min"], with_raw=with_raw)


def inner_loop(group_sizes, opname, okw, x0, y, mask, n_iter, optimizer, aux, loss_function, loss_weight, reduce, gain, nodes, fp32=False):
    """The guided sub-step's data term over a batch of contiguous groups with the gain field: per image the nodes learnt at the
    starting phi, then the masked oracle on (y', M G).  nodes [B,gh,gw].  Returns (loss [B], {phi: [B,k,1,1]}, g [B,4,H,W], nodes
    [B,gh,gw] float64 (fp32 values, as stored), G [B,1,H,W], the nodes before the last step's rounding to fp32)."""
    B, _, H, W = y.shape
    gh, gw = gain["grid"]
    tabs = tables(H, W, gh, gw)
    F, w = model_image(opname, okw, x0, loss_weight)
    m0 = None if mask is None else mask.double().expand(B, 3, H, W)
    new, raw = substep_nodes(nodes, tabs, F, w, y.double(), m0, loss_function, gain, fp32=fp32, with_raw=True)
    G = field64(torch.from_numpy(new.astype(np.float32).astype(np.float64)), tabs)
    ye = (y.double() + 1) / G - 1
    me = (torch.ones(B, 3, H, W, dtype=torch.float64) if m0 is None else m0) * G
    sep, phi, g = GO.grouped_inner_loop(group_sizes, opname, okw, None, x0, ye, me, n_iter, optimizer, aux, loss_function, loss_weight,
                                        reduce)
    return sep, phi, g, new, G, raw


def direct_inner_loop(opname, okw, x0, y, mask, G, n_iter, aux, loss_function, loss_weight):
    """One image's (or one group's) inner loop with the model I = G F written out: r = (y - (2 G F - 1)) w M.  Returns what
    `physgroup_oracle.group_inner_loop` returns."""
    guide = GO.make_guidance(opname, okw, None, x0.shape[-2], x0.shape[-1], mask, n_iter, None, aux, loss_function, loss_weight, "mean")
    op = guide.op
    fwd = op.forward
    op.forward = lambda data: G * fwd(data)
    xb = x0.clone().requires_grad_(True)
    op.set_requires_grad(True)
    for it in range(n_iter):
        sep, loss = guide.loss(xb, y)
        a = guide.group_aux(xb)
        total = loss if a is None else loss + a
        total.backward(inputs=([xb] if it == n_iter - 1 else []) + list(op.phi.values()))
        guide.step(x0.shape[0])
    return np.asarray(sep, dtype=np.float64), {n: p.detach().clone() for n, p in op.phi.items()}, xb.grad.detach().clone()


class GainGuidance(GO.GroupGuidance):
    """The grouped (masked) guidance with a learnt gain field: `conditioning` learns the nodes at the phi it starts with, then runs
    the masked step on (y', M G).  base_mask: M0 or None; gain: the setting; nodes [B,gh,gw] float64 carried over the chain."""
    base_mask = None
    gain = None
    nodes = None

    def conditioning(self, x_prev, x_t, x_0_hat, y, freeze_phi):
        if self.gain is None:
            self.mask = self.base_mask
            return super().conditioning(x_prev, x_t, x_0_hat, y, freeze_phi)
        B, _, H, W = y.shape
        tabs = tables(H, W, *self.gain["grid"])
        with torch.no_grad():
            x = x_0_hat.detach().double()
            F = self.op.forward(x)
            w = self._weight(x)
        m0 = None if self.base_mask is None else self.base_mask.double().expand(B, 3, H, W)
        self.nodes = substep_nodes(self.nodes, tabs, F, w, y.double(), m0, self.loss_function, self.gain, freeze_phi)
        self.nodes = self.nodes.astype(np.float32).astype(np.float64)
        G = field64(torch.from_numpy(self.nodes), tabs)
        self.mask = ((torch.ones(B, 3, H, W, dtype=torch.float64) if m0 is None else m0) * G).to(x_0_hat.dtype)
        return super().conditioning(x_prev, x_t, x_0_hat, ((y.double() + 1) / G - 1).to(y.dtype), freeze_phi)


def make_guidance(opname, okw, mask, n_iter, aux, loss_function, loss_weight, gain, nodes, reduce="mean", optimizer=None,
                  scale="7,7,7,0.9", gradient_clip="False,0"):
    op = D.PhysOperator(opname, batch_size=1, optimizer=optimizer, **okw)
    guide = GainGuidance(op, n_iter=n_iter, scale=scale, gradient_clip=gradient_clip, aux=aux, loss_function=loss_function,
                         loss_weight=loss_weight)
    guide.A, guide.base_mask, guide.mask, guide.reduce, guide.gain = None, mask, mask, reduce, gain
    guide.nodes = None if nodes is None else np.asarray(nodes, dtype=np.float64)
    return guide


# ----------------------------------------------------------------------------- the effect: a cos^4 vignette
PHI_TRUE = dict(phi_a="1.2,0.6,0.4", phi_b="1.0,0.7,0.5", phi_inf="0.1,0.5,0.6")
OPNAME = "underwater_physical_revised"


def vignette(H, W, k=0.7):
    """G* = cos^4(atan(k rho)) over its maximum, rho the radius in pixel-centre coordinates normalised to [-1, 1] per axis."""
    yy, xx = np.meshgrid((2 * np.arange(H) + 1) / H - 1, (2 * np.arange(W) + 1) / W - 1, indexing="ij")
    rho = np.sqrt(xx ** 2 + yy ** 2)
    g = np.cos(np.arctan(k * rho)) ** 4
    return g / g.max()


def effect_problem(seed=0, H=36, W=34, noise=0.01, k=0.7):
    """x0 [1,4,H,W] float64 held at the truth and y = 2 G* F(phi*) - 1 + N(0, noise); returns (x0, y, G* [H,W], F [1,3,H,W])."""
    g = torch.Generator().manual_seed(seed)
    J = 0.1 + 0.8 * torch.rand(1, 3, H, W, generator=g, dtype=torch.float64)
    d = 0.2 + 1.3 * torch.rand(1, 1, H, W, generator=g, dtype=torch.float64)
    x0 = torch.cat([2 * J - 1, d], dim=1)
    op = D.PhysOperator(OPNAME, batch_size=1, depth_type="move", value=0.0, **PHI_TRUE)
    F = op.forward(x0)
    Gs = vignette(H, W, k)
    y = 2 * torch.from_numpy(Gs)[None, None] * F - 1 + noise * torch.randn(1, 3, H, W, generator=g, dtype=torch.float64)
    return x0, y, Gs, F


def effect_fit(F, y, grid=(5, 5), steps=200, loss_function="norm", eta=0.01, smooth=0.0, g_min=0.05):
    """`steps` sub-steps of one (gradient, step) from a flat field, image and phi held at the truth: G [H,W] float64."""
    H, W = y.shape[-2:]
    tabs = tables(H, W, *grid)
    n = np.ones((1,) + tuple(grid))
    for _ in range(steps):
        n = learn64(n, tabs, F, 1, y, None, loss_function, eta, 1, smooth, g_min, fp32_nodes=False)
    return field64(torch.from_numpy(n), tabs)[0, 0].numpy()
