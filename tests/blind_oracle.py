"""The oracle of blind deblurring (operator `blind_blur`, include/osmosis_blind.h): torch on the CPU, float64 unless told otherwise.
The reference has no such operator; the definition is the header's.

  A(k) x     = F.conv2d(F.pad(x, reflect), k) per plane, k a leaf tensor                         (`conv_reflect`)
  loss_b, r  = ||rho_b||, rho_b = M_b (y_b - A(k) x0_b[0:3]);  r_b = -M_b rho_b / loss_b (0 for a fully masked image)
  c_b        = d <r_b, A(k) x0_b> / d k            by autograd                                   (`tap_corr`; `tap_corr_direct`: a double loop)
  g          = A(k)^T r                            by autograd
  step       = the header's, numpy float64, sums over t in the header's order (`sum_t`)         (`step`)
`inner_loop` runs n_iter of them as osm_ps_blind_optimize does (loss and g before the last step); `ps_chain` drives a DDPM 'ps'
chain over `oracle.diffusion_ref.p_mean_variance` with the oracle's UNet (fp32, as everywhere in the suite) and this data term."""
import numpy as np
import torch
import torch.nn.functional as F

LANES = 1024            # lanes of osm_psf_tap_step's one workgroup: the shape of its sums over t


def refl(c, n):
    return -c if c < 0 else (2 * (n - 1) - c if c >= n else c)


def conv_reflect(x, k):
    kh, kw = k.shape
    P = x.shape[1]
    return F.conv2d(F.pad(x, (kw // 2, kw // 2, kh // 2, kh // 2), mode="reflect"), k.expand(P, 1, kh, kw).contiguous(), groups=P)


def dense_taps(k):
    """(dy, dx) int32 [k^2] of the dense k x k support, row-major."""
    iy, ix = np.divmod(np.arange(k * k), k)
    return (iy - k // 2).astype(np.int32), (ix - k // 2).astype(np.int32)


def loss_and_r(Ax, y, mask=None):
    """loss [B] and r = d loss / d Ax [B,3,H,W], as osm_ps_loss_grad_c / _mc define them."""
    rho = y - Ax
    if mask is not None:
        rho = rho * mask
    loss = (rho ** 2).sum(dim=(1, 2, 3)).sqrt()
    safe = torch.where(loss > 0, loss, torch.ones_like(loss))
    r = -(rho if mask is None else rho * mask) / safe[:, None, None, None]
    r = torch.where((loss > 0)[:, None, None, None], r, torch.zeros_like(r))
    return loss, r


def tap_corr(r, x, kh, kw):
    """c [B, kh, kw]: c_b[a, e] = sum_p sum_ij r[b,p,i,j] x[b,p,refl(i + a - kh//2), refl(j + e - kw//2)], by autograd w.r.t. the kernel."""
    out = []
    for b in range(x.shape[0]):
        k = torch.zeros(kh, kw, dtype=x.dtype, requires_grad=True)
        (c,) = torch.autograd.grad((r[b:b + 1] * conv_reflect(x[b:b + 1], k)).sum(), k)
        out.append(c)
    return torch.stack(out)


def tap_corr_direct(r, x, dy, dx):
    """c [B, T] by the definition: a double loop over pixels per tap (small images only)."""
    B, P, H, W = x.shape
    c = np.zeros((B, len(dy)))
    rn, xn = r.numpy().astype(np.float64), x.numpy().astype(np.float64)
    for t, (a, e) in enumerate(zip(dy, dx)):
        rows = [refl(i + int(a), H) for i in range(H)]
        cols = [refl(j + int(e), W) for j in range(W)]
        c[:, t] = (rn * xn[:, :, rows][:, :, :, cols]).sum(axis=(1, 2, 3))
    return c


def sum_t(a):
    """SUM_t of the header: lane l sums t = l, l + LANES, ... ascending, then a halving tree over the lanes."""
    a = np.asarray(a, dtype=np.float64)
    rows = -(-a.size // LANES)
    pad = np.zeros(rows * LANES)
    pad[:a.size] = a
    pad = pad.reshape(rows, LANES)
    lane = np.zeros(LANES)
    for row in pad:
        lane = lane + row
    h = LANES // 2
    while h >= 1:
        lane[:h] = lane[:h] + lane[h:2 * h]
        h //= 2
    return float(lane[0])


def step(w, c, loss, hw3, eta, l1=0.0):
    """One projected step: w fp32 [T], c float64 [B, T], loss [B] (fp32 values) -> (w_new fp32 [T], u float64 [T], S)."""
    w = np.asarray(w, dtype=np.float32)
    c = np.asarray(c, dtype=np.float64)
    loss = np.asarray(loss, dtype=np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = np.zeros(w.size)
        for b in range(c.shape[0]):
            s = s + loss[b] * c[b]
        g = s / float(hw3)
        gbar = sum_t(g) / w.size
        v = (w.astype(np.float64) - eta * (g - gbar)) - eta * l1
        u = np.where(v > 0, v, 0.0)
        S = sum_t(u)
    if not (S > 0) or np.isinf(S):
        return w.copy(), u, S
    return (u / S).astype(np.float32), u, S


def inner_loop(x0, y, mask, w0, kh, kw, n_iter, eta, l1=0.0, dtype=torch.float64):
    """n_iter iterations as osm_ps_blind_optimize enqueues them.  x0 [B,C,H,W], y [B,3,H,W], mask [B,3,H,W] or None, w0 fp32 [kh kw]
    (dense, row-major).  The image side (A, loss, r, c, g) in `dtype`, the step always in float64 from fp32-rounded losses.
    Returns dict(loss [B], g [B,C,H,W], w fp32 [T], c [B,T], first_loss)."""
    x0 = x0.to(dtype)
    y = y.to(dtype)
    mask = None if mask is None else mask.to(dtype)
    w = np.asarray(w0, dtype=np.float32).copy()
    B, C, H, W = x0.shape
    first = None
    for it in range(n_iter):
        k = torch.from_numpy(w.reshape(kh, kw).astype(np.float64)).to(dtype).requires_grad_(True)
        xs = x0[:, 0:3].detach().clone().requires_grad_(True)
        Ax = conv_reflect(xs, k)
        loss, r = loss_and_r(Ax.detach(), y, mask)
        c = tap_corr(r, x0[:, 0:3], kh, kw).reshape(B, -1)
        if first is None:
            first = loss.clone()
        if it == n_iter - 1:
            (gx,) = torch.autograd.grad(Ax, xs, r)
            g = torch.zeros_like(x0)
            g[:, 0:3] = gx
        w, _, _ = step(w, c.double().numpy(), loss.float().double().numpy(), 3 * H * W, eta, l1)
    return dict(loss=loss, g=g, w=w, c=c, first_loss=first)


def ps_chain(unet_fn, tb, x_T, y, noises, w0, kh, kw, n_iter, eta, l1, scale, mask=None, trace=None):
    """A DDPM 'ps' (rgb-guidance) chain with the blind data term: per index, p_mean_variance of the oracle on the network's output,
    sample = mean + exp(0.5 logvar) noise (none at index 0), then x = sample - scale * d/dx_prev <g, pred_xstart> with (loss, g, w) of
    `inner_loop` on pred_xstart.  unet_fn(x, t_mapped) -> [B,2C,H,W] (fp32, autograd).  Returns (img, w fp32 [T])."""
    from oracle import diffusion_ref as D
    img = x_T.clone()
    w = np.asarray(w0, dtype=np.float32).copy()
    T = tb.num_timesteps
    for k_, idx in enumerate(range(T - 1, -1, -1)):
        img = img.detach().requires_grad_(True)
        out = D.p_mean_variance(tb, unet_fn(img, torch.tensor([tb.timestep_map[idx]] * img.shape[0])), img, idx)
        sample = out["mean"].detach()
        if idx != 0:
            sample = sample + torch.exp(0.5 * out["log_variance"].detach()) * noises[k_]
        res = inner_loop(out["pred_xstart"].detach(), y, mask, w, kh, kw, n_iter, eta, l1)
        w = res["w"]
        (grad,) = torch.autograd.grad(out["pred_xstart"], img, res["g"].to(img.dtype))
        new = sample - scale * grad
        if trace is not None:
            trace.append(dict(x_in=img.detach().clone(), x_out=new.clone(), loss=res["loss"].clone(), w=w.copy()))
        img = new
    return img.detach(), w


def recovery_problem():
    """The convex problem of the recovery tests: the image is known, the kernel is not.  x float64 [1,3,36,44] = 1.5 x a 3 x 3 box
    average of U(-1, 1) under torch.manual_seed(0), k* = motion_kernel(7, 0.5, 3), y = A(k*) x, the init a gaussian of sigma 1.5.
    Returns (x, y, k* float64 [7,7], w0 fp32 [49])."""
    from osmosis_diffusion_code_amd.guided_diffusion.measurements import blind_init_kernel, motion_kernel
    torch.manual_seed(0)
    u = torch.rand(1, 3, 36, 44, dtype=torch.float64) * 2 - 1
    x = 1.5 * F.avg_pool2d(F.pad(u, (1, 1, 1, 1), mode="reflect"), 3, stride=1)
    kstar = motion_kernel(7, 0.5, 3)
    y = conv_reflect(x, torch.from_numpy(kstar))
    w0 = blind_init_kernel(7, "gaussian", 1.5).reshape(-1).astype(np.float32)
    return x, y, kstar, w0
