"""The oracle of the water / haze data term through a linear operator (the reference has no such operator): a subclass of
`oracle.diffusion_ref.OsmosisGuidance` whose loss forms I = op.forward(x0), applies A in float64 from the same fp32 band tables /
taps the kernels get, and takes the residual on A's grid:

    diff = (y - (2 A I - 1)) (A w) M          norm: ||diff||       mse: mean(diff^2) over the measurement's 3 h w

For a separable operator A is the dense pair band_to_dense(host_tables); for a PSF it is F.conv2d(F.pad(., reflect), k).
Shared by tests/test_physlin_cpu.py and tests/test_physlin_gpu.py."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import diffusion_ref as D
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M

DEGRADATIONS = {
    "gaussian_blur": dict(name="gaussian_blur", kernel_size=9, intensity=1.5),
    "motion_blur": dict(name="motion_blur", kernel_size=9),
    "psf_blur": dict(name="psf_blur", normalize=False,                          # asymmetric 3 x 7, sum 1.27
                     kernel=[[0.02, 0.0, 0.05, 0.11, 0.04, 0.0, 0.01], [0.0, 0.08, 0.21, 0.33, 0.09, 0.03, 0.0],
                             [0.01, 0.0, 0.06, 0.14, 0.0, 0.07, 0.02]]),
    "sr2_bicubic": dict(name="super_resolution", scale_factor=2, method="bicubic"),
    "sr2_box": dict(name="super_resolution", scale_factor=2, method="box"),
}


def dense_operator(deg, H, W, dtype=torch.float64):
    """A as a function on [B,P,H,W] tensors (computed in `dtype`, whatever the input's) of a `measurements.GRID_OPERATORS`
    instance, from the fp32 tables / taps the kernels read."""
    if isinstance(deg, M.SeparableOperator):
        sh, wh, sw, ww = deg.host_tables(H, W)["fwd"]
        Rh = torch.from_numpy(M.band_to_dense(sh, wh, H)).to(dtype)
        Rw = torch.from_numpy(M.band_to_dense(sw, ww, W)).to(dtype)
        return lambda x: Rh @ x.to(dtype) @ Rw.T
    dy, dx, w = deg.host_taps()
    Ry, Rx = deg.radius()
    k = torch.zeros(2 * Ry + 1, 2 * Rx + 1, dtype=dtype)
    k[torch.from_numpy(dy.astype(np.int64)) + Ry, torch.from_numpy(dx.astype(np.int64)) + Rx] = torch.from_numpy(w).to(dtype)

    def conv(x):
        P = x.shape[1]
        xp = F.pad(x.to(dtype), (Rx, Rx, Ry, Ry), mode="reflect")
        return F.conv2d(xp, k.expand(P, 1, *k.shape).contiguous(), groups=P)
    return conv


class LinGuidance(D.OsmosisGuidance):
    """The oracle's guidance with A between the image-formation model and the residual.  `A`: `dense_operator(...)`; `mask`: None
    or [B,3,h,w] / broadcastable."""
    A = None
    mask = None

    def loss(self, x0, y):
        I = self.op.forward(x0)
        It = self.A(I)
        w = self._weight(x0)
        diff = (y.to(It.dtype) - (2 * It - 1)) * (self.A(w) if torch.is_tensor(w) else 1)
        if self.mask is not None:
            diff = diff * self.mask.to(It.dtype)
        if self.loss_function == "norm":
            return torch.norm(diff.detach(), p=2, dim=[1, 2, 3]).numpy(), torch.linalg.norm(diff)
        mse = (diff ** 2).mean(dim=(1, 2, 3))
        return mse.detach().numpy(), mse.sum()


def oracle_inner_loop(opname, okw, deg, x0, y, mask, n_iter, optimizer, aux, loss_function, loss_weight, A_dtype=torch.float64):
    """One image: n_iter x (loss + auxiliary losses, backward, phi step); the last backward also into x0.
    Returns (sep loss of the last iteration, {phi name: tensor}, d total / d x0)."""
    H, W = x0.shape[-2:]
    op = D.PhysOperator(opname, batch_size=1, optimizer=optimizer, **okw)
    guide = LinGuidance(op, n_iter=n_iter, scale="7,7,7,0.9", gradient_clip="False,0", aux=aux, loss_function=loss_function,
                        loss_weight=loss_weight)
    guide.A, guide.mask = dense_operator(deg, H, W, A_dtype), mask
    xb = x0.clone().requires_grad_(True)
    op.set_requires_grad(True)
    for it in range(n_iter):
        sep, loss = guide.loss(xb, y)
        a = D.aux_loss(xb, aux)
        total = loss if a is None else loss + a
        total.backward(inputs=([xb] if it == n_iter - 1 else []) + list(op.phi.values()))
        op.sgd_step()
    return float(sep[0]), {n: p.detach().clone() for n, p in op.phi.items()}, xb.grad.detach().clone()
