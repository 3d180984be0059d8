"""`torch.library` registration of the hot path (north_star: "driven from Python through PyTorch-ROCm
custom ops"): the UNet forward / input-gradient plans and the guidance-step kernels as dispatcher-visible operators in the
`osmosis::` namespace -- schema, fake-tensor (meta) implementations and autograd registration -- with the C ABI
(include/osmosis_hip.h, called through ctypes in ops.py / engine.py) underneath.  Nothing here computes: every operator
enqueues hand-written gfx950 kernels on the current HIP stream; there is no CPU implementation (the operators are
registered for the "cuda" device type only, which is HIP on ROCm).

    osmosis::unet_fwd(x, t, engine) -> out                  UNetModel.forward (reference unet.py:713-742); differentiable
                                                           w.r.t. x (condition_methods.py:188-191 back-propagates through it)
    osmosis::unet_bwd_data(grad_out, engine) -> dx          the recorded data-gradient plan of the same engine
    osmosis::posterior(model_out, x, coef) -> (pred_xstart, mean, log_variance)     gaussian_diffusion.py:349-376 +
                                                           posterior_mean_variance.py (every registered processor pair)
    osmosis::posterior_clip(...) -> (pred_xstart clamped, mean, log_variance, raw prediction), osmosis::clamp_bwd(g, raw) -> masked g
                                                           (`clip_denoised: True` of the shipped rgb-guidance config)
    osmosis::posterior_dynthr(...) -> (pred_xstart thresholded, mean, log_variance, raw prediction, q, idx),
    osmosis::dynthr_bwd(g, raw, q, idx, s) -> d loss/d raw  (`dynamic_threshold`: clip(x * quantile(|x|, s), -1, 1) over the batch,
                                                           util/img_utils.py:8-15), osmosis::quantile_abs(x, s) -> (q, idx)
    osmosis::posterior_bwd(g, coef) -> d_model_out         d(pred_xstart)/d(model_out)^T g  (the chain rule into the UNet)
    osmosis::guide_update(mean, log_variance, g, dx_unet, noise, coef, scale4, clip) -> (x_next, grad)
                                                           condition_methods.py:186-221 update rule + the noise add of :262-271
    The step operators (posterior, posterior_clip, posterior_dynthr, posterior_bwd, guide_update, guide_update_rng, ddim_update) take a
    [B,C,H,W] state of any channel count with a network output of C or 2 C channels and a scale of C entries: (C, Cout) is read off
    the tensors and the channel-generic entry points (osm_*_c) are called, for every pair; a mismatch raises before anything
    launches.  Each has a `_c` twin (OPS_C) with the same implementation.  The [B,4,HW] C entry points remain for C callers and
    are bit-identical at (4, 8).
    osmosis::phys_loss_grad(x0, y, phi, icfg, fcfg, n_inner, freeze_phi) -> (loss, grad_x0, phi_new)
    osmosis::phys_loss_grad_lin(x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, family, tables, dims) -> (loss, grad_x0, phi_new)
    osmosis::phys_loss_grad_g(x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, group_sizes, reduce) -> (loss, grad_x0, phi_new)
                                                           measurements.py forward models + the inner phi optimisation
                                                           (cm.py:141-184), functional (phi is returned, not updated in place)
    osmosis::recon_fullres(depth, guide, image, phi_a, phi_b, phi_inf, depth_type, dval, amap, mode, radius, sigma_s, sigma_r)
                                                           -> (rgb, rgb_u8, depth_full): the physical model inverted on the ORIGINAL
                                                           pixel grid from phi and the upsampled depth (osmosis_sampling.py:253-255)
    osmosis::linop_apply(x, start_h, wt_h, start_w, wt_w, Hout, Wout, [transposed tables]) -> out
                                                           a separable banded linear operator per plane (gaussian blur, bicubic / box
                                                           downsampling) and, with the transposed tables, its adjoint = its backward
    osmosis::psf_apply(x, dy, dx, w, Ry, Rx, adjoint) -> out   a point-spread function (tap list) per plane over reflection padding
                                                           (motion blur, a measured PSF); its backward is itself with `adjoint` flipped
    osmosis::psf_apply_s(x, dy, dx, w[nb,nc,T], Ry, Rx, adjoint) -> out
                                                           the same with one weight set per image and / or per plane
    osmosis::psf_field_apply(x, dy, dx, w[gh,gw,T], iy0, fy, ix0, fx, Ry, Rx, adjoint) -> out
                                                           a field of PSFs on a node grid, interpolated bilinearly over the frame
    osmosis::field_tap_grad(x, r, dy, dx, iy0, fy, ix0, fx, gh, gw, Ry, Rx) -> part[B,NP,T]
    osmosis::field_tap_step(w[gh,gw,T], part, loss, H, W, P, eta, l1, smooth)
                                                           learning that field: the per-node tap partials, one projected step (w mutated)
    osmosis::ps_blind_loss_grad_s(x0, y, mask, dy, dx, w[nb,nc,T], Ry, Rx, n_iter, eta, l1) -> (loss, g)
                                                           blind deblurring with one learnt PSF per image / per colour plane (w mutated)

`engine` is an integer handle (`engine_handle(eng)`) because operator schemas carry tensors and scalars only; the handle
table holds weak references, so an engine dies with its model.  An engine keeps the activations of its LAST forward pass:
the autograd node of `unet_fwd` remembers which pass it belongs to (the engine's pass counter, a Python-side attribute, not an
operator output -- outputs are functions of the inputs alone, so fake-tensor tracing and `torch.library.opcheck` see pure
operators) and raises instead of differentiating through activations a later forward has overwritten."""
import itertools
import weakref
from typing import List, Optional, Tuple

import torch

from . import ops
from ._lib import OsmosisHipError, PhysDesc

_ENGINES = weakref.WeakValueDictionary()
_next_handle = itertools.count(1)


def engine_handle(eng) -> int:
    """A handle that is never reused (id(eng) can be, once the engine is collected -- and tickets restart at 0)."""
    h = getattr(eng, "_osm_handle", None)
    if h is None:
        h = eng._osm_handle = next(_next_handle)
    _ENGINES[h] = eng
    return h


def _engine(handle: int):
    eng = _ENGINES.get(int(handle))
    if eng is None:
        raise OsmosisHipError(f"osmosis:: operator called with a stale engine handle ({handle}): the engine was released")
    return eng


# ----------------------------------------------------------------------------------------------------------------- UNet
@torch.library.custom_op("osmosis::unet_fwd", mutates_args=(), device_types="cuda")
def unet_fwd(x: torch.Tensor, t: torch.Tensor, engine: int) -> torch.Tensor:
    eng = _engine(engine)
    if tuple(x.shape) != tuple(eng.x_in.shape):
        raise OsmosisHipError(f"osmosis::unet_fwd: engine is planned for x {tuple(eng.x_in.shape)}, got {tuple(x.shape)}")
    return eng.forward(x, t, need_grad=True).clone()


@unet_fwd.register_fake
def _unet_fwd_fake(x, t, engine):
    eng = _engine(engine)
    return x.new_empty((x.shape[0], eng.cout, x.shape[2], x.shape[3]))


@torch.library.custom_op("osmosis::unet_bwd_data", mutates_args=(), device_types="cuda")
def unet_bwd_data(grad_out: torch.Tensor, engine: int) -> torch.Tensor:
    """dL/dx of the engine's LAST forward pass (its activations are what the engine holds)."""
    return _engine(engine).backward(grad_out.contiguous()).clone()


@unet_bwd_data.register_fake
def _unet_bwd_fake(grad_out, engine):
    eng = _engine(engine)
    return grad_out.new_empty((grad_out.shape[0], eng.cin, grad_out.shape[2], grad_out.shape[3]))


def _unet_setup(ctx, inputs, output):
    ctx.engine = inputs[2]
    ctx.engine_obj = _engine(inputs[2])           # strong reference: the activations backward needs live in this engine
    ctx.ticket = ctx.engine_obj.ticket            # the forward pass this node belongs to (eager mode: checked below)


def _unet_backward(ctx, grad_out):
    if _engine(ctx.engine) is not ctx.engine_obj or ctx.engine_obj.ticket != ctx.ticket:
        raise RuntimeError("UNet activations were overwritten by a later forward before backward ran")
    return torch.ops.osmosis.unet_bwd_data(grad_out, ctx.engine), None, None


unet_fwd.register_autograd(_unet_backward, setup_context=_unet_setup)


# ------------------------------------------------------------------------------------------------------------ sampler step
def _chw(x):
    if x.dim() != 4 or x.dtype != torch.float32 or not x.is_contiguous():
        raise OsmosisHipError("osmosis:: guidance operators take contiguous fp32 [B,C,H,W] tensors")
    return x.shape[0], x.shape[2] * x.shape[3]


# One plain implementation per step job, serving the [B,4,HW]-era operator name and its `_c` twin alike: (C, Cout) comes from the
# tensors, and what does not fit them is refused before anything launches.  Twins with one schema are one function under two names.
def _step_ops(fn, fake, *names):
    out = []
    for name in names:
        out.append(torch.library.custom_op(f"osmosis::{name}", fn, mutates_args=(), device_types="cuda"))
        out[-1].register_fake(fake)
    return out


def _cc(model_out, x):
    if model_out.dim() != 4 or model_out.shape[1] not in (x.shape[1], 2 * x.shape[1]):
        raise OsmosisHipError("osmosis:: the network output must have C or 2 C channels")
    if model_out.shape[0] != x.shape[0] or model_out.shape[2:] != x.shape[2:]:
        raise OsmosisHipError("osmosis:: the network output must have the state's batch and grid")
    return x.shape[1], model_out.shape[1]


def _channel_scale(name, scale, x):
    if scale.numel() != x.shape[1]:
        raise OsmosisHipError(f"{name}: scale must have one entry per channel")
    return x.shape[1]


def _posterior_impl(model_out, x, coef, mean_kind, var_kind, clip):
    B, HW = _chw(x)
    Cc, Cout = _cc(model_out, x)
    x0, mean, logvar = (torch.empty_like(x) for _ in range(3))
    raw = torch.empty_like(x) if clip else None
    ops.posterior_c(model_out.contiguous(), x, coef, x0, mean, logvar, B, Cc, Cout, HW, mean_kind, var_kind, x0_raw=raw)
    return (x0, mean, logvar, raw) if clip else (x0, mean, logvar)


def _posterior_bwd_impl(g, coef, cout):
    B, HW = _chw(g)
    d_out = torch.empty(B, cout, g.shape[2], g.shape[3], device=g.device, dtype=torch.float32)
    ops.posterior_bwd_c(g, coef, d_out, B, g.shape[1], cout, HW)
    return d_out


def _guide_update_impl(name, mean, log_variance, g, dx_unet, noise, coef, scale, clip):
    B, HW = _chw(mean)
    Cc = _channel_scale(name, scale, mean)
    x_next, grad = torch.empty_like(mean), torch.empty_like(mean)
    ops.guide_update_c(mean, log_variance, g, dx_unet, noise, coef, scale, clip, x_next, grad, B, Cc, HW)
    return x_next, grad


def _guide_update_rng_impl(name, mean, log_variance, g, dx_unet, coef, scale, clip, seed, step, step_offset, img0, img_stride, sub):
    B, HW = _chw(mean)
    Cc = _channel_scale(name, scale, mean)
    x_next, grad, noise = torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)
    ops.guide_update_rng_c(mean, log_variance, g, dx_unet, coef, scale, clip, x_next, grad, noise, B, Cc, HW, seed, step,
                           step_offset=step_offset, sub=sub, img0=img0, img_stride=img_stride)
    return x_next, grad, noise


def _ddim_update_impl(name, x0, x, g, dx_unet, noise, coef, dcoef, scale, clip):
    B, HW = _chw(x0)
    Cc = _channel_scale(name, scale, x0)
    x_next, grad = torch.empty_like(x0), torch.empty_like(x0)
    ops.ddim_update_c(x0, x, g, dx_unet, noise, coef, dcoef, scale, clip, x_next, grad, B, Cc, HW)
    return x_next, grad


def _posterior(model_out: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, mean_kind: int = 0,
               var_kind: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """coef: the 8 fp32 coefficients of the step (GaussianDiffusion.coef_table row, fetched by osm_fetch_coefs); mean_kind / var_kind:
    the processors' `kernel_kind` (osm_posterior_c; 0, 0 = epsilon / learned_range).  x [B,C,H,W], model_out with 2 C channels or
    with C (no variance half: the variance processor reads model_out itself)."""
    return _posterior_impl(model_out, x, coef, mean_kind, var_kind, clip=False)


def _posterior_fake(model_out, x, coef, mean_kind=0, var_kind=0):
    return torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)


posterior, posterior_c = _step_ops(_posterior, _posterior_fake, "posterior", "posterior_c")


def _posterior_clip(model_out: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, mean_kind: int = 0,
                    var_kind: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::posterior with `clip_denoised` (process_xstart, posterior_mean_variance.py:43-50; configs/rgb_guidance_sample_config.yaml):
    (pred_xstart clamped to [-1, 1], mean formed from it, log_variance, the unclamped prediction for osmosis::clamp_bwd)."""
    return _posterior_impl(model_out, x, coef, mean_kind, var_kind, clip=True)


def _posterior_clip_fake(model_out, x, coef, mean_kind=0, var_kind=0):
    return torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.empty_like(x)


posterior_clip, posterior_clip_c = _step_ops(_posterior_clip, _posterior_clip_fake, "posterior_clip", "posterior_clip_c")


@torch.library.custom_op("osmosis::clamp_bwd", mutates_args=(), device_types="cuda")
def clamp_bwd(g: torch.Tensor, x_raw: torch.Tensor, lo: float = -1.0, hi: float = 1.0) -> torch.Tensor:
    """g where lo <= x_raw <= hi, 0 elsewhere (NaN included): the backward of x_raw.clamp(lo, hi) on a gradient (osm_clamp_bwd)."""
    out = g.detach().clone().contiguous()
    ops.clamp_bwd(out, x_raw.contiguous(), lo, hi)
    return out


@clamp_bwd.register_fake
def _clamp_bwd_fake(g, x_raw, lo=-1.0, hi=1.0):
    return torch.empty_like(g)


@torch.library.custom_op("osmosis::quantile_abs", mutates_args=(), device_types="cuda")
def quantile_abs(x: torch.Tensor, s: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(torch.quantile(x.abs(), s) as an fp32 [1] tensor, int32 [2] flat indices of its two order statistics in stable-sort order)."""
    if x.dtype != torch.float32:
        raise OsmosisHipError("osmosis::quantile_abs takes an fp32 tensor")
    xc = x.contiguous()
    q, idx = torch.empty(1, device=x.device, dtype=torch.float32), torch.empty(2, device=x.device, dtype=torch.int32)
    ops.quantile_abs(xc, s, q, idx, ops.quantile_workspace(xc.numel(), x.device))
    return q, idx


@quantile_abs.register_fake
def _quantile_abs_fake(x, s):
    return x.new_empty((1,)), x.new_empty((2,), dtype=torch.int32)


def _posterior_dynthr(model_out: torch.Tensor, x: torch.Tensor, coef: torch.Tensor, mean_kind: int = 0, var_kind: int = 0,
                      s: float = 0.98) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::posterior with `dynamic_threshold` (process_xstart, posterior_mean_variance.py:43-50): (pred_xstart = clip(raw *
    quantile(|raw|, s), -1, 1) over all B C H W elements, mean formed from it, log_variance, the raw prediction, q [1], idx [2]) -- the
    last three are what osmosis::dynthr_bwd takes."""
    B, HW = _chw(x)
    Cc, Cout = _cc(model_out, x)
    x0, mean, logvar, raw = (torch.empty_like(x) for _ in range(4))
    q, idx = torch.empty(1, device=x.device, dtype=torch.float32), torch.empty(2, device=x.device, dtype=torch.int32)
    ops.posterior_dynthr_c(model_out.contiguous(), x, coef, x0, mean, logvar, raw, q, idx,
                           ops.quantile_workspace(x.numel(), x.device), B, Cc, Cout, HW, mean_kind, var_kind, s)
    return x0, mean, logvar, raw, q, idx


def _posterior_dynthr_fake(model_out, x, coef, mean_kind=0, var_kind=0, s=0.98):
    return (torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), torch.empty_like(x), x.new_empty((1,)),
            x.new_empty((2,), dtype=torch.int32))


posterior_dynthr, posterior_dynthr_c = _step_ops(_posterior_dynthr, _posterior_dynthr_fake, "posterior_dynthr", "posterior_dynthr_c")


@torch.library.custom_op("osmosis::dynthr_bwd", mutates_args=(), device_types="cuda")
def dynthr_bwd(g: torch.Tensor, x_raw: torch.Tensor, q: torch.Tensor, idx: torch.Tensor, s: float = 0.98) -> torch.Tensor:
    """d loss/d x_raw from g = d loss/d x0 through x0 = clip(x_raw * quantile(|x_raw|, s), -1, 1) (q, idx: its forward's; osm_dynthr_bwd)."""
    out = g.detach().clone().contiguous()
    ops.dynthr_bwd(out, x_raw.contiguous(), q, idx, ops.quantile_workspace(out.numel(), g.device), s)
    return out


@dynthr_bwd.register_fake
def _dynthr_bwd_fake(g, x_raw, q, idx, s=0.98):
    return torch.empty_like(g)


@torch.library.custom_op("osmosis::posterior_bwd", mutates_args=(), device_types="cuda")
def posterior_bwd(g: torch.Tensor, coef: torch.Tensor) -> torch.Tensor:
    """d loss / d model_out for a network output of 2 C channels (the variance half is zero); C channels: osmosis::posterior_bwd_c."""
    return _posterior_bwd_impl(g, coef, 2 * g.shape[1])


@posterior_bwd.register_fake
def _posterior_bwd_fake(g, coef):
    return g.new_empty((g.shape[0], 2 * g.shape[1], g.shape[2], g.shape[3]))


@torch.library.custom_op("osmosis::guide_update", mutates_args=(), device_types="cuda")
def guide_update(mean: torch.Tensor, log_variance: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, noise: torch.Tensor,
                 coef: torch.Tensor, scale4: torch.Tensor, clip: float) -> Tuple[torch.Tensor, torch.Tensor]:
    return _guide_update_impl("osmosis::guide_update", mean, log_variance, g, dx_unet, noise, coef, scale4, clip)


@guide_update.register_fake
def _guide_update_fake(mean, log_variance, g, dx_unet, noise, coef, scale4, clip):
    return torch.empty_like(mean), torch.empty_like(mean)


@torch.library.custom_op("osmosis::guide_update_rng", mutates_args=(), device_types="cuda")
def guide_update_rng(mean: torch.Tensor, log_variance: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, coef: torch.Tensor,
                     scale4: torch.Tensor, clip: float, seed: int, step: torch.Tensor, step_offset: int, img0: int,
                     img_stride: int, sub: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::guide_update with the step noise drawn in the kernel (Philox-4x32-10: key = seed, counter = (element / 4,
    img0 + b * img_stride, (step[0] + step_offset) | sub << 16)); a pure function of its inputs.  sub: the sub-step of a step
    repeated at the same t (PCGS local_M; 0 = the plain step).  Returns (x_next, grad, the noise drawn)."""
    return _guide_update_rng_impl("osmosis::guide_update_rng", mean, log_variance, g, dx_unet, coef, scale4, clip, seed, step,
                                  step_offset, img0, img_stride, sub)


@guide_update_rng.register_fake
def _guide_update_rng_fake(mean, log_variance, g, dx_unet, coef, scale4, clip, seed, step, step_offset, img0, img_stride, sub=0):
    return torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)


@torch.library.custom_op("osmosis::ddim_update", mutates_args=(), device_types="cuda")
def ddim_update(x0: torch.Tensor, x: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor,
                dcoef: torch.Tensor, scale4: torch.Tensor, clip: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """DDIM step + guidance (osm_ddim_update): coef = the posterior row, dcoef = row of GaussianDiffusion.ddim_table()."""
    return _ddim_update_impl("osmosis::ddim_update", x0, x, g, dx_unet, noise, coef, dcoef, scale4, clip)


@ddim_update.register_fake
def _ddim_update_fake(x0, x, g, dx_unet, noise, coef, dcoef, scale4, clip):
    return torch.empty_like(x0), torch.empty_like(x0)


PHYS_ICFG = ("kind", "depth_type", "weight_type", "wdepth_type", "loss_type", "optimizer")
PHYS_FCFG = ("dval0", "dval1", "dval2", "wval0", "wval1", "wval2", "gamma_avrg", "gamma_val", "eta0", "eta1", "eta2")


def phys_config(desc: PhysDesc) -> Tuple[List[int], List[float]]:
    """The (int list, float list) form of a physics descriptor (what ConditioningMethod._prepare fills) for phys_loss_grad."""
    return ([int(getattr(desc, k)) for k in PHYS_ICFG],
            [float(v) for v in (*desc.dval, *desc.wval, desc.gamma_avrg, desc.gamma_val, *desc.eta)])


@torch.library.custom_op("osmosis::phys_loss_grad", mutates_args=(), device_types="cuda")
def phys_loss_grad(x0: torch.Tensor, y: torch.Tensor, phi: torch.Tensor, icfg: List[int], fcfg: List[float], n_inner: int,
                   freeze_phi: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """n_inner x (reduce, finalize + phi step) of the physical model's loss, then loss and dL/dx0 at the last phi and its step
    (osm_phys_optimize).  SGD / GD only here (Adam carries optimizer state across steps: use the conditioning method)."""
    return _phys_loss_grad_impl("osmosis::phys_loss_grad", x0, y, None, phi, icfg, fcfg, n_inner, freeze_phi)


def _mask_rows(name, mask, y):
    """A mask [B,3,H,W] or [B,1,H,W] as the contiguous [B,3,HW] rows the kernels read."""
    if mask.dim() != 4 or mask.shape[0] != y.shape[0] or mask.shape[1] not in (1, 3) or mask.shape[2:] != y.shape[2:]:
        raise OsmosisHipError(f"{name}: expected mask [B,3,H,W] or [B,1,H,W] on the measurement's grid")
    return mask.expand(y.shape).contiguous()


def _phys_loss_grad_impl(name, x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, grp=None):
    B, HW = _chw(x0)
    if len(icfg) != len(PHYS_ICFG) or len(fcfg) != len(PHYS_FCFG):
        raise OsmosisHipError(f"{name}: icfg / fcfg must come from torch_ops.phys_config(desc)")
    d = PhysDesc()
    for k, v in zip(PHYS_ICFG, icfg):
        setattr(d, k, int(v))
    if d.optimizer != 0:
        raise OsmosisHipError(f"{name} is functional: optimizer state (adam, ...) lives with the conditioning method")
    if d.kind == 3 and not freeze_phi:
        raise OsmosisHipError(f"{name}: the identity operator (kind 3) has no parameters: pass freeze_phi=True")
    for i in range(3):
        d.dval[i], d.wval[i], d.eta[i] = fcfg[i], fcfg[3 + i], fcfg[8 + i]
    d.gamma_avrg, d.gamma_val = fcfg[6], fcfg[7]
    d.B, d.HW = B, HW
    dev = x0.device
    phi_new = phi.detach().clone().contiguous()
    part = torch.empty(B * ops.phys_nblk(HW) * 16, device=dev, dtype=torch.float32)
    red = torch.zeros(B * 16, device=dev, dtype=torch.float32)
    loss = torch.zeros(B, device=dev, dtype=torch.float32)
    g = torch.empty_like(x0)
    if grp is not None:
        ops.phys_optimize_g(d, grp, x0, y.contiguous(), None if mask is None else _mask_rows(name, mask, y), phi_new, part, red, loss, g,
                            1 if freeze_phi else n_inner, freeze_phi)
    elif mask is None:
        ops.phys_optimize(d, x0, y.contiguous(), phi_new, part, red, loss, g, 1 if freeze_phi else n_inner, freeze_phi)
    else:
        ops.phys_optimize_m(d, x0, y.contiguous(), _mask_rows(name, mask, y), phi_new, part, red, loss, g,
                            1 if freeze_phi else n_inner, freeze_phi)
    return loss, g, phi_new


@phys_loss_grad.register_fake
def _phys_loss_grad_fake(x0, y, phi, icfg, fcfg, n_inner, freeze_phi):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0), torch.empty_like(phi)


@torch.library.custom_op("osmosis::phys_loss_grad_m", mutates_args=(), device_types="cuda")
def phys_loss_grad_m(x0: torch.Tensor, y: torch.Tensor, mask: torch.Tensor, phi: torch.Tensor, icfg: List[int], fcfg: List[float],
                     n_inner: int, freeze_phi: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::phys_loss_grad with a per-pixel validity mask [B,3,H,W] / [B,1,H,W] in [0, 1] in the data term: the residual of
    channel c is (y_c - (2 I_c - 1)) w M_c, the losses keep their normalisation (osm_phys_optimize_m)."""
    return _phys_loss_grad_impl("osmosis::phys_loss_grad_m", x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi)


@phys_loss_grad_m.register_fake
def _phys_loss_grad_m_fake(x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0), torch.empty_like(phi)


@torch.library.custom_op("osmosis::phys_loss_grad_g", mutates_args=(), device_types="cuda")
def phys_loss_grad_g(x0: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], phi: torch.Tensor, icfg: List[int],
                     fcfg: List[float], n_inner: int, freeze_phi: bool, group_sizes: List[int],
                     reduce: str) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::phys_loss_grad / _m (mask None / a mask) with shared water parameters: the batch is partitioned into contiguous
    groups of `group_sizes` images, each with ONE phi (its rows of `phi` equal on entry, equal on return), stepped once per inner
    iteration with the members' pooled gradient (`reduce`: "mean" or "sum"; osm_phys_optimize_g).  Loss and grad_x0 stay per image."""
    name = "osmosis::phys_loss_grad_g"
    if reduce not in ("mean", "sum") or not group_sizes or any(int(n) < 1 for n in group_sizes) or \
            sum(int(n) for n in group_sizes) != x0.shape[0]:
        raise OsmosisHipError(f"{name}: group_sizes must be positive ints summing to the batch {x0.shape[0]} and reduce 'mean' or 'sum', "
                              f"got {list(group_sizes)} and {reduce!r}")
    return _phys_loss_grad_impl(name, x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, grp=ops.group_desc(group_sizes, reduce))


@phys_loss_grad_g.register_fake
def _phys_loss_grad_g_fake(x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, group_sizes, reduce):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0), torch.empty_like(phi)


@torch.library.custom_op("osmosis::exposure_mask", mutates_args=(), device_types="cuda")
def exposure_mask(y: torch.Tensor, low: float, high: float, soft: float = 0.0, per_pixel: bool = False) -> torch.Tensor:
    """Validity mask [B,3,H,W] from the exposure of y [B,3,H,W] in [-1, 1] (osm_exposure_mask): 0 where v = (y + 1) / 2 leaves
    (low, high), a ramp of width `soft` inside each bound; per_pixel: the channel minimum on every channel."""
    if y.dim() != 4 or y.shape[1] != 3:
        raise OsmosisHipError("osmosis::exposure_mask: expected y [B,3,H,W]")
    out = torch.empty(y.shape, device=y.device, dtype=torch.float32)
    ops.exposure_mask(y.contiguous(), out, y.shape[0], y.shape[2] * y.shape[3], low, high, soft, per_pixel)
    return out


@exposure_mask.register_fake
def _exposure_mask_fake(y, low, high, soft=0.0, per_pixel=False):
    return y.new_empty(y.shape)


# ---- the `_c` names of the step operators whose schema differs from their twin's (`cout`; `scale` for `scale4`): same implementations
@torch.library.custom_op("osmosis::posterior_bwd_c", mutates_args=(), device_types="cuda")
def posterior_bwd_c(g: torch.Tensor, coef: torch.Tensor, cout: int) -> torch.Tensor:
    """d loss / d model_out [B,cout,H,W] from g = d loss / d x0 [B,C,H,W] (osm_posterior_bwd_c); cout = C or 2 C."""
    return _posterior_bwd_impl(g, coef, cout)


@posterior_bwd_c.register_fake
def _posterior_bwd_c_fake(g, coef, cout):
    return g.new_empty((g.shape[0], cout, g.shape[2], g.shape[3]))


@torch.library.custom_op("osmosis::guide_update_c", mutates_args=(), device_types="cuda")
def guide_update_c(mean: torch.Tensor, log_variance: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, noise: torch.Tensor,
                   coef: torch.Tensor, scale: torch.Tensor, clip: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """osmosis::guide_update under its `_c` name; scale: [C]."""
    return _guide_update_impl("osmosis::guide_update_c", mean, log_variance, g, dx_unet, noise, coef, scale, clip)


@guide_update_c.register_fake
def _guide_update_c_fake(mean, log_variance, g, dx_unet, noise, coef, scale, clip):
    return torch.empty_like(mean), torch.empty_like(mean)


@torch.library.custom_op("osmosis::guide_update_rng_c", mutates_args=(), device_types="cuda")
def guide_update_rng_c(mean: torch.Tensor, log_variance: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, coef: torch.Tensor,
                       scale: torch.Tensor, clip: float, seed: int, step: torch.Tensor, step_offset: int, img0: int,
                       img_stride: int, sub: int = 0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::guide_update_rng under its `_c` name (counter word 0 = element / 4 within the image's C H W elements)."""
    return _guide_update_rng_impl("osmosis::guide_update_rng_c", mean, log_variance, g, dx_unet, coef, scale, clip, seed, step,
                                  step_offset, img0, img_stride, sub)


@guide_update_rng_c.register_fake
def _guide_update_rng_c_fake(mean, log_variance, g, dx_unet, coef, scale, clip, seed, step, step_offset, img0, img_stride, sub=0):
    return torch.empty_like(mean), torch.empty_like(mean), torch.empty_like(mean)


@torch.library.custom_op("osmosis::ddim_update_c", mutates_args=(), device_types="cuda")
def ddim_update_c(x0: torch.Tensor, x: torch.Tensor, g: torch.Tensor, dx_unet: torch.Tensor, noise: torch.Tensor, coef: torch.Tensor,
                  dcoef: torch.Tensor, scale: torch.Tensor, clip: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """osmosis::ddim_update under its `_c` name; scale: [C]."""
    return _ddim_update_impl("osmosis::ddim_update_c", x0, x, g, dx_unet, noise, coef, dcoef, scale, clip)


@ddim_update_c.register_fake
def _ddim_update_c_fake(x0, x, g, dx_unet, noise, coef, dcoef, scale, clip):
    return torch.empty_like(x0), torch.empty_like(x0)


@torch.library.custom_op("osmosis::ps_loss_grad_c", mutates_args=(), device_types="cuda")
def ps_loss_grad_c(x0: torch.Tensor, y: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """The 'ps' data term (identity operator, gaussian noiser) on x0 [B,C,H,W], y [B,3,H,W]: (loss [B] = ||y - x0[:, 0:3]|| per
    image, g = d loss / d x0) (osm_ps_loss_grad_c)."""
    B, HW = _chw(x0)
    if y.shape[0] != B or y.shape[1] != 3 or x0.shape[1] < 3:
        raise OsmosisHipError("osmosis::ps_loss_grad_c: expected x0 [B,C>=3,H,W] and y [B,3,H,W]")
    loss = torch.empty(B, device=x0.device, dtype=torch.float32)
    g = torch.empty_like(x0)
    part = torch.empty(B * ops.phys_nblk(HW), device=x0.device, dtype=torch.float32)
    ops.ps_loss_grad_c(x0, y.contiguous(), part, loss, g, B, x0.shape[1], HW)
    return loss, g


@ps_loss_grad_c.register_fake
def _ps_loss_grad_c_fake(x0, y):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0)


@torch.library.custom_op("osmosis::ps_loss_grad_mc", mutates_args=(), device_types="cuda")
def ps_loss_grad_mc(x0: torch.Tensor, y: torch.Tensor, mask: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
    """osmosis::ps_loss_grad_c with a validity mask [B,3,H,W] / [B,1,H,W] in [0, 1]: loss [B] = ||M (y - x0[:, 0:3])|| per image,
    g = -M^2 (y - x0) / loss (0 for an image that is masked out entirely) (osm_ps_loss_grad_mc)."""
    B, HW = _chw(x0)
    if y.shape[0] != B or y.shape[1] != 3 or x0.shape[1] < 3:
        raise OsmosisHipError("osmosis::ps_loss_grad_mc: expected x0 [B,C>=3,H,W] and y [B,3,H,W]")
    loss = torch.empty(B, device=x0.device, dtype=torch.float32)
    g = torch.empty_like(x0)
    part = torch.empty(B * ops.phys_nblk(HW), device=x0.device, dtype=torch.float32)
    ops.ps_loss_grad_mc(x0, y.contiguous(), _mask_rows("osmosis::ps_loss_grad_mc", mask, y), part, loss, g, B, x0.shape[1], HW)
    return loss, g


@ps_loss_grad_mc.register_fake
def _ps_loss_grad_mc_fake(x0, y, mask):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0)


@torch.library.custom_op("osmosis::recon_fullres", mutates_args=(), device_types="cuda")
def recon_fullres(depth: torch.Tensor, guide: torch.Tensor, image: torch.Tensor, phi_a: torch.Tensor, phi_b: torch.Tensor,
                  phi_inf: torch.Tensor, depth_type: int, dval: List[float], amap: List[float], mode: int = 0, radius: int = 2,
                  sigma_s: float = 1.0, sigma_r: float = 0.1) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """The physical model inverted on the original pixel grid (osm_recon_fullres): raw network depth [h,w], guide [3,h,w] (the image
    the sampler saw, [0,1]), image [3,Hc,Wc] (the photo's covered rectangle, [0,1]), phi_a / phi_b / phi_inf [3], depth_type / dval
    from utils.depth_code_and_values, amap = [ay, by, ax, bx] (image pixel -> network-grid coordinate), mode 0 bilinear / 1 joint
    bilateral upsampling -> (rgb [3,Hc,Wc] fp32 unclipped, rgb_u8 [Hc,Wc,3] uint8 truncated, depth_full [Hc,Wc] raw depth)."""
    if len(dval) != 3 or len(amap) != 4:
        raise OsmosisHipError("osmosis::recon_fullres: dval has 3 entries, amap 4")
    if image.dim() != 3 or image.shape[0] != 3:
        raise OsmosisHipError("osmosis::recon_fullres: image must be [3,Hc,Wc]")
    Hc, Wc = image.shape[1], image.shape[2]
    rgb = torch.empty((3, Hc, Wc), device=image.device, dtype=torch.float32)
    u8 = torch.empty((Hc, Wc, 3), device=image.device, dtype=torch.uint8)
    full = torch.empty((Hc, Wc), device=image.device, dtype=torch.float32)
    ops.recon_fullres(depth.contiguous(), guide.contiguous(), image.contiguous(), phi_a.contiguous(), phi_b.contiguous(),
                      phi_inf.contiguous(), depth_type, dval, amap, rgb, u8, full, mode, radius, sigma_s, sigma_r)
    return rgb, u8, full


@recon_fullres.register_fake
def _recon_fullres_fake(depth, guide, image, phi_a, phi_b, phi_inf, depth_type, dval, amap, mode=0, radius=2, sigma_s=1.0,
                        sigma_r=0.1):
    Hc, Wc = image.shape[1], image.shape[2]
    return (image.new_empty((3, Hc, Wc)), image.new_empty((Hc, Wc, 3), dtype=torch.uint8), image.new_empty((Hc, Wc)))


# ---- tiled sampling: canvas [C,Hc,Wc] <-> overlapping tiles [n,C,th,tw]; each operator is the other's backward (same weights)
def _tile_weights(name, wy, wx, inv_norm):
    ws = (wy, wx, inv_norm)
    if any(w is None for w in ws) != all(w is None for w in ws):
        raise OsmosisHipError(f"{name}: wy, wx and inv_norm are given together or not at all")
    return tuple(None if w is None else w.detach().contiguous() for w in ws)


@torch.library.custom_op("osmosis::tile_gather", mutates_args=(), device_types="cuda")
def tile_gather(canvas: torch.Tensor, origins: torch.Tensor, th: int, tw: int, wy: Optional[torch.Tensor] = None,
                wx: Optional[torch.Tensor] = None, inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """tiles [n,C,th,tw] of canvas [C,Hc,Wc] at origins int32 [n,2] (y, x) (osm_tile_gather): a bit-exact crop without weights,
    else scaled by wy[y] wx[x] inv_norm[oy+y,ox+x].  Backward: osmosis::tile_blend with the same weights."""
    if canvas.dim() != 3:
        raise OsmosisHipError("osmosis::tile_gather: canvas must be [C,Hc,Wc]")
    tiles = torch.empty((origins.shape[0], canvas.shape[0], th, tw), device=canvas.device, dtype=torch.float32)
    ops.tile_gather(canvas.contiguous(), tiles, origins.contiguous(), *_tile_weights("osmosis::tile_gather", wy, wx, inv_norm))
    return tiles


@tile_gather.register_fake
def _tile_gather_fake(canvas, origins, th, tw, wy=None, wx=None, inv_norm=None):
    return canvas.new_empty((origins.shape[0], canvas.shape[0], th, tw))


@torch.library.custom_op("osmosis::tile_blend", mutates_args=(), device_types="cuda")
def tile_blend(tiles: torch.Tensor, origins: torch.Tensor, Hc: int, Wc: int, wy: Optional[torch.Tensor] = None,
               wx: Optional[torch.Tensor] = None, inv_norm: Optional[torch.Tensor] = None) -> torch.Tensor:
    """canvas [C,Hc,Wc] = inv_norm * sum over the covering tiles (ascending index, fp32) of wy wx tiles (osm_tile_blend; without
    weights the plain sum; an uncovered pixel is 0).  Backward: osmosis::tile_gather with the same weights."""
    if tiles.dim() != 4:
        raise OsmosisHipError("osmosis::tile_blend: tiles must be [n,C,th,tw]")
    canvas = torch.empty((tiles.shape[1], Hc, Wc), device=tiles.device, dtype=torch.float32)
    ops.tile_blend(tiles.contiguous(), canvas, origins.contiguous(), *_tile_weights("osmosis::tile_blend", wy, wx, inv_norm))
    return canvas


@tile_blend.register_fake
def _tile_blend_fake(tiles, origins, Hc, Wc, wy=None, wx=None, inv_norm=None):
    return tiles.new_empty((tiles.shape[1], Hc, Wc))


def _tile_gather_setup(ctx, inputs, output):
    canvas, origins, _th, _tw, wy, wx, inv_norm = inputs
    ctx.hw = (canvas.shape[1], canvas.shape[2])
    ctx.save_for_backward(origins, *(w for w in (wy, wx, inv_norm) if w is not None))


def _tile_gather_backward(ctx, grad):
    origins, *ws = ctx.saved_tensors
    ws = ws if ws else [None, None, None]
    return (torch.ops.osmosis.tile_blend(grad.contiguous(), origins, ctx.hw[0], ctx.hw[1], *ws), None, None, None, None, None, None)


def _tile_blend_setup(ctx, inputs, output):
    tiles, origins, _Hc, _Wc, wy, wx, inv_norm = inputs
    ctx.hw = (tiles.shape[2], tiles.shape[3])
    ctx.save_for_backward(origins, *(w for w in (wy, wx, inv_norm) if w is not None))


def _tile_blend_backward(ctx, grad):
    origins, *ws = ctx.saved_tensors
    ws = ws if ws else [None, None, None]
    return (torch.ops.osmosis.tile_gather(grad.contiguous(), origins, ctx.hw[0], ctx.hw[1], *ws), None, None, None, None, None, None)


tile_gather.register_autograd(_tile_gather_backward, setup_context=_tile_gather_setup)
tile_blend.register_autograd(_tile_blend_backward, setup_context=_tile_blend_setup)


# ---- separable banded linear operators (blur, downsampling): out = R_h x R_w^T per plane; the backward is the operator itself with the
# transposed tables, which the caller hands over beside the forward ones (measurements.SeparableOperator builds both)
def _linop_tables(name, start_h, wt_h, start_w, wt_w, Hout, Wout):
    if wt_h.dim() != 2 or wt_w.dim() != 2 or tuple(start_h.shape) != (Hout,) or tuple(start_w.shape) != (Wout,) \
            or wt_h.shape[0] != Hout or wt_w.shape[0] != Wout:
        raise OsmosisHipError(f"{name}: expected start_h [{Hout}], wt_h [{Hout},Kh], start_w [{Wout}], wt_w [{Wout},Kw], got "
                              f"{tuple(start_h.shape)}, {tuple(wt_h.shape)}, {tuple(start_w.shape)}, {tuple(wt_w.shape)}")
    return start_h.contiguous(), wt_h.detach().contiguous(), start_w.contiguous(), wt_w.detach().contiguous()


@torch.library.custom_op("osmosis::linop_apply", mutates_args=(), device_types="cuda")
def linop_apply(x: torch.Tensor, start_h: torch.Tensor, wt_h: torch.Tensor, start_w: torch.Tensor, wt_w: torch.Tensor, Hout: int,
                Wout: int, tstart_h: Optional[torch.Tensor] = None, twt_h: Optional[torch.Tensor] = None,
                tstart_w: Optional[torch.Tensor] = None, twt_w: Optional[torch.Tensor] = None) -> torch.Tensor:
    """out [B,P,Hout,Wout], out[b,p,i,j] = sum_a wt_h[i][a] sum_c wt_w[j][c] x[b,p,start_h[i]+a,start_w[j]+c] of x [B,P,Hin,Win]
    (osm_linop_apply): band tables on the device, start int32 [n_out], wt fp32 [n_out,K].  tstart_* / twt_*: the tables of the
    transposed factors ([Hin] / [Hin,K'] and [Win] / [Win,K'']); with them the operator is differentiable w.r.t. x -- its backward is
    the operator itself with the two pairs of tables exchanged -- and without them it is forward only."""
    if x.dim() != 4:
        raise OsmosisHipError("osmosis::linop_apply: x must be [B,P,Hin,Win]")
    B, P, Hin, Win = x.shape
    tabs = _linop_tables("osmosis::linop_apply", start_h, wt_h, start_w, wt_w, Hout, Wout)
    out = torch.empty((B, P, Hout, Wout), device=x.device, dtype=torch.float32)
    ops.linop_apply(x.contiguous(), out, *tabs, B, P, P * Hin * Win, P * Hout * Wout, Hin, Win)
    return out


@linop_apply.register_fake
def _linop_apply_fake(x, start_h, wt_h, start_w, wt_w, Hout, Wout, tstart_h=None, twt_h=None, tstart_w=None, twt_w=None):
    return x.new_empty((x.shape[0], x.shape[1], Hout, Wout))


def _linop_setup(ctx, inputs, output):
    x, start_h, wt_h, start_w, wt_w, _Hout, _Wout, tstart_h, twt_h, tstart_w, twt_w = inputs
    ctx.hw = (x.shape[2], x.shape[3])
    ctx.has_t = tstart_h is not None and twt_h is not None and tstart_w is not None and twt_w is not None
    if ctx.has_t:
        ctx.save_for_backward(start_h, wt_h, start_w, wt_w, tstart_h, twt_h, tstart_w, twt_w)


def _linop_backward(ctx, grad):
    if not ctx.has_t:
        raise OsmosisHipError("osmosis::linop_apply: the backward needs the transposed tables (tstart_h, twt_h, tstart_w, twt_w)")
    start_h, wt_h, start_w, wt_w, tstart_h, twt_h, tstart_w, twt_w = ctx.saved_tensors
    gx = torch.ops.osmosis.linop_apply(grad.contiguous(), tstart_h, twt_h, tstart_w, twt_w, ctx.hw[0], ctx.hw[1], start_h, wt_h,
                                       start_w, wt_w)
    return (gx,) + (None,) * 10


linop_apply.register_autograd(_linop_backward, setup_context=_linop_setup)


# ---- point-spread-function operators (a 2-D kernel as a tap list): reflection padding + cross-correlation per plane, or (adjoint) the
# exact transpose of that map; the backward is the operator itself with `adjoint` flipped
@torch.library.custom_op("osmosis::psf_apply", mutates_args=(), device_types="cuda")
def psf_apply(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, w: torch.Tensor, Ry: int, Rx: int, adjoint: bool) -> torch.Tensor:
    """out [B,P,H,W] of x [B,P,H,W] (osm_psf_apply): out[b,p,i,j] = sum_t w[t] x[b,p,refl_H(i+dy[t]),refl_W(j+dx[t])] (torch 'reflect'
    padding, cross-correlation), or with `adjoint` the transpose of that map.  The tap list lives on the device: dy, dx int32 [T],
    w fp32 [T]; Ry >= max |dy|, Rx >= max |dx| (Ry < H, Rx < W).  Differentiable w.r.t. x."""
    if x.dim() != 4:
        raise OsmosisHipError("osmosis::psf_apply: x must be [B,P,H,W]")
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape) or tuple(w.shape) != tuple(dy.shape):
        raise OsmosisHipError(f"osmosis::psf_apply: expected dy [T], dx [T], w [T], got {tuple(dy.shape)}, {tuple(dx.shape)}, {tuple(w.shape)}")
    B, P, H, W = x.shape
    out = torch.empty((B, P, H, W), device=x.device, dtype=torch.float32)
    ops.psf_apply(x.contiguous(), out, dy.contiguous(), dx.contiguous(), w.detach().contiguous(), Ry, Rx, B, P, P * H * W, P * H * W, H, W,
                  adjoint=adjoint)
    return out


@psf_apply.register_fake
def _psf_apply_fake(x, dy, dx, w, Ry, Rx, adjoint):
    return x.new_empty(x.shape)


def _psf_setup(ctx, inputs, output):
    _x, dy, dx, w, ctx.Ry, ctx.Rx, ctx.adjoint = inputs
    ctx.save_for_backward(dy, dx, w)


def _psf_backward(ctx, grad):
    dy, dx, w = ctx.saved_tensors
    return (torch.ops.osmosis.psf_apply(grad.contiguous(), dy, dx, w, ctx.Ry, ctx.Rx, not ctx.adjoint),) + (None,) * 6


psf_apply.register_autograd(_psf_backward, setup_context=_psf_setup)


# ---- the same operator with weight SETS w [nb,nc,T]: one PSF per image (nb = B) and / or per plane (nc = P), include/osmosis_psfset.h
@torch.library.custom_op("osmosis::psf_apply_s", mutates_args=(), device_types="cuda")
def psf_apply_s(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, w: torch.Tensor, Ry: int, Rx: int, adjoint: bool) -> torch.Tensor:
    """out [B,P,H,W] of x [B,P,H,W] (osm_psf_apply_s): `osmosis::psf_apply` where plane p of image b takes the weights
    w[nb > 1 ? b : 0, nc > 1 ? p : 0] of w fp32 [nb,nc,T], nb in {1, B}, nc in {1, P}; the tap list dy, dx int32 [T] is shared.
    Differentiable w.r.t. x."""
    if x.dim() != 4:
        raise OsmosisHipError("osmosis::psf_apply_s: x must be [B,P,H,W]")
    B, P, H, W = x.shape
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape) or w.dim() != 3 or w.shape[2] != dy.shape[0] or w.shape[0] not in (1, B) \
            or w.shape[1] not in (1, P):
        raise OsmosisHipError(f"osmosis::psf_apply_s: expected dy [T], dx [T], w [nb,nc,T] with nb in (1, {B}), nc in (1, {P}), got "
                              f"{tuple(dy.shape)}, {tuple(dx.shape)}, {tuple(w.shape)}")
    out = torch.empty((B, P, H, W), device=x.device, dtype=torch.float32)
    ops.psf_apply_s(x.contiguous(), out, dy.contiguous(), dx.contiguous(), w.detach().contiguous(), Ry, Rx, B, P, P * H * W, P * H * W, H, W,
                    adjoint=adjoint)
    return out


@psf_apply_s.register_fake
def _psf_apply_s_fake(x, dy, dx, w, Ry, Rx, adjoint):
    return x.new_empty(x.shape)


def _psf_s_backward(ctx, grad):
    dy, dx, w = ctx.saved_tensors
    return (torch.ops.osmosis.psf_apply_s(grad.contiguous(), dy, dx, w, ctx.Ry, ctx.Rx, not ctx.adjoint),) + (None,) * 6


psf_apply_s.register_autograd(_psf_s_backward, setup_context=_psf_setup)


# ---- a FIELD of point-spread functions w [gh,gw,T] on a node grid, interpolated bilinearly (include/osmosis_psffield.h)
@torch.library.custom_op("osmosis::psf_field_apply", mutates_args=(), device_types="cuda")
def psf_field_apply(x: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, w: torch.Tensor, iy0: torch.Tensor, fy: torch.Tensor,
                    ix0: torch.Tensor, fx: torch.Tensor, Ry: int, Rx: int, adjoint: bool) -> torch.Tensor:
    """out [B,P,H,W] of x [B,P,H,W] (osm_psf_field_apply): every pixel blurred with the bilinear interpolation of the four corner PSFs
    of its cell of the gh x gw node grid -- w fp32 [gh,gw,T] over the shared tap list dy, dx int32 [T]; (iy0, fy, ix0, fx) =
    `ops.field_tables(H, W, gh, gw, device)` -- or with `adjoint` the transpose of that map.  Differentiable w.r.t. x."""
    if x.dim() != 4:
        raise OsmosisHipError("osmosis::psf_field_apply: x must be [B,P,H,W]")
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape) or w.dim() != 3 or w.shape[2] != dy.shape[0]:
        raise OsmosisHipError(f"osmosis::psf_field_apply: expected dy [T], dx [T], w [gh,gw,T], got {tuple(dy.shape)}, {tuple(dx.shape)}, "
                              f"{tuple(w.shape)}")
    B, P, H, W = x.shape
    out = torch.empty((B, P, H, W), device=x.device, dtype=torch.float32)
    ops.psf_field_apply(x.contiguous(), out, dy.contiguous(), dx.contiguous(), w.detach().contiguous(),
                        (iy0.contiguous(), fy.contiguous(), ix0.contiguous(), fx.contiguous()), Ry, Rx, B, P, P * H * W, P * H * W, H, W,
                        adjoint=adjoint)
    return out


@psf_field_apply.register_fake
def _psf_field_apply_fake(x, dy, dx, w, iy0, fy, ix0, fx, Ry, Rx, adjoint):
    return x.new_empty(x.shape)


def _psf_field_setup(ctx, inputs, output):
    _x, dy, dx, w, iy0, fy, ix0, fx, ctx.Ry, ctx.Rx, ctx.adjoint = inputs
    ctx.save_for_backward(dy, dx, w, iy0, fy, ix0, fx)


def _psf_field_backward(ctx, grad):
    return (torch.ops.osmosis.psf_field_apply(grad.contiguous(), *ctx.saved_tensors, ctx.Ry, ctx.Rx, not ctx.adjoint),) + (None,) * 10


psf_field_apply.register_autograd(_psf_field_backward, setup_context=_psf_field_setup)


# ---- learning that field (include/osmosis_blindfield.h): the per-node tap partials and the projected step of every node
@torch.library.custom_op("osmosis::field_tap_grad", mutates_args=(), device_types="cuda")
def field_tap_grad(x: torch.Tensor, r: torch.Tensor, dy: torch.Tensor, dx: torch.Tensor, iy0: torch.Tensor, fy: torch.Tensor,
                   ix0: torch.Tensor, fx: torch.Tensor, gh: int, gw: int, Ry: int, Rx: int) -> torch.Tensor:
    """part [B, NP, T] of x, r [B,P,H,W] (osm_field_tap_grad): the 32 x 32 tile partials of the tap gradient c_n of every node n of the
    gh x gw field, in the compact layout of `ops.field_tap_layout(H, W, gh, gw, P)` (per image; per node; plane-major; the node's
    tiles row-major); (iy0, fy, ix0, fx) = `ops.field_tables(H, W, gh, gw, device)`.  No autograd formula."""
    name = "osmosis::field_tap_grad"
    if x.dim() != 4 or tuple(r.shape) != tuple(x.shape):
        raise OsmosisHipError(f"{name}: x and r must be [B,P,H,W] alike, got {tuple(x.shape)} and {tuple(r.shape)}")
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape):
        raise OsmosisHipError(f"{name}: expected dy [T], dx [T], got {tuple(dy.shape)}, {tuple(dx.shape)}")
    B, P, H, W = x.shape
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, P, x.device)
    part = torch.empty((B, NP, dy.shape[0]), device=x.device, dtype=torch.float32)
    ops.field_tap_grad(x.contiguous(), r.contiguous(), dy.contiguous(), dx.contiguous(),
                       (iy0.contiguous(), fy.contiguous(), ix0.contiguous(), fx.contiguous()), lay, NP, gh, gw, Ry, Rx, B, P, P * H * W,
                       P * H * W, H, W, part)
    return part


@field_tap_grad.register_fake
def _field_tap_grad_fake(x, r, dy, dx, iy0, fy, ix0, fx, gh, gw, Ry, Rx):
    B, P, H, W = x.shape
    return x.new_empty((B, ops.field_tap_layout(int(H), int(W), gh, gw, int(P))[1], dy.shape[0]))


@torch.library.custom_op("osmosis::field_tap_step", mutates_args=("w",), device_types="cuda")
def field_tap_step(w: torch.Tensor, part: torch.Tensor, loss: torch.Tensor, H: int, W: int, P: int, eta: float, l1: float,
                   smooth: float) -> None:
    """One projected step of every node of the field w fp32 [gh,gw,T], IN PLACE (osm_field_tap_step): part [B, NP, T] as
    `osmosis::field_tap_grad` returns it for P planes of H x W, loss [B]; the normaliser is 3 H W."""
    name = "osmosis::field_tap_step"
    if w.dim() != 3 or not w.is_contiguous() or part.dim() != 3 or part.shape[2] != w.shape[2] or loss.dim() != 1 \
            or loss.shape[0] != part.shape[0]:
        raise OsmosisHipError(f"{name}: expected a contiguous w [gh,gw,T], part [B,NP,T] and loss [B], got {tuple(w.shape)}, "
                              f"{tuple(part.shape)}, {tuple(loss.shape)}")
    gh, gw = int(w.shape[0]), int(w.shape[1])
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, P, w.device)
    if part.shape[1] != NP:
        raise OsmosisHipError(f"{name}: part has {part.shape[1]} partials per image, the layout of {P} x {H} x {W} under {gh} x {gw} has {NP}")
    ops.field_tap_step(w, torch.empty_like(w), part.contiguous(), loss.contiguous(), lay, NP, part.shape[0], 3 * H * W, eta, l1, smooth)


@field_tap_step.register_fake
def _field_tap_step_fake(w, part, loss, H, W, P, eta, l1, smooth):
    return None


# ---- the water / haze data term through a linear operator (blur, super-resolution, a PSF) between the model and the photo
def lin_config(operator, H, W, device) -> Tuple[int, List[torch.Tensor], List[int]]:
    """(family, tables, dims) of a `measurements.GRID_OPERATORS` instance for phys_loss_grad_lin at the image grid H x W:
    family 0 (separable): the four forward band tables then the four transposed ones, dims = [h, w];
    family 1 (psf): dy, dx, w, dims = [Ry, Rx]."""
    from .guided_diffusion.measurements import BlindFieldOperator, PSFFieldOperator, PSFOperator, SeparableOperator
    if isinstance(operator, BlindFieldOperator):
        raise OsmosisHipError("lin_config: 'blind_field_blur' carries a learnt field of point-spread functions; the composed water / haze "
                              "data term takes one fixed point-spread function (osm_lin_desc has no such family)")
    if isinstance(operator, PSFFieldOperator):
        raise OsmosisHipError("lin_config: 'field_blur' carries a field of point-spread functions; the composed water / haze data term "
                              "takes one (osm_lin_desc has no such family)")
    if isinstance(operator, PSFOperator):
        if operator.weight_sets != (1, 1):
            raise OsmosisHipError(f"lin_config: the operator carries weight sets {operator.weight_sets} (per_image / per_channel); the "
                                  "composed water / haze data term takes one point-spread function")
        operator.out_shape(H, W)
        return 1, list(operator.taps(device)), list(operator.radius())
    if not isinstance(operator, SeparableOperator):
        raise OsmosisHipError(f"lin_config: {type(operator).__name__} is neither a SeparableOperator nor a PSFOperator")
    t = operator.tables(H, W, device)
    return 0, list(t["fwd"]) + list(t["adj"]), list(operator.out_shape(H, W))


@torch.library.custom_op("osmosis::phys_loss_grad_lin", mutates_args=(), device_types="cuda")
def phys_loss_grad_lin(x0: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], phi: torch.Tensor, icfg: List[int],
                       fcfg: List[float], n_inner: int, freeze_phi: bool, family: int, tables: List[torch.Tensor],
                       dims: List[int]) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """osmosis::phys_loss_grad_m with a linear operator A between the image-formation model and the photo (osm_phys_optimize_lin):
    x0 [B,4,H,W]; y [B,3,h,w] and the optional mask ([B,3,h,w] / [B,1,h,w]) on A's grid; the residual of channel c is
    (y_c - (2 (A I)_c - 1)) (A w) M_c, mse divides by 3 h w.  A travels as `lin_config(operator, H, W, device)`.  SGD / GD only."""
    name = "osmosis::phys_loss_grad_lin"
    from ._lib import LinDesc
    B, HW = _chw(x0)
    H, W = x0.shape[2], x0.shape[3]
    if len(icfg) != len(PHYS_ICFG) or len(fcfg) != len(PHYS_FCFG):
        raise OsmosisHipError(f"{name}: icfg / fcfg must come from torch_ops.phys_config(desc)")
    d = PhysDesc()
    for k, v in zip(PHYS_ICFG, icfg):
        setattr(d, k, int(v))
    if d.optimizer != 0:
        raise OsmosisHipError(f"{name} is functional: optimizer state (adam, ...) lives with the conditioning method")
    if d.kind == 3:
        raise OsmosisHipError(f"{name}: the identity operator (kind 3) has no image-formation model to compose with")
    for i in range(3):
        d.dval[i], d.wval[i], d.eta[i] = fcfg[i], fcfg[3 + i], fcfg[8 + i]
    d.gamma_avrg, d.gamma_val = fcfg[6], fcfg[7]
    d.B, d.HW = B, HW
    lin = LinDesc()
    lin.family, lin.H, lin.W = int(family), H, W
    if family == 0:
        if len(tables) != 8 or len(dims) != 2:
            raise OsmosisHipError(f"{name}: a separable operator is 8 band tables (forward, transposed) and dims = [h, w]")
        h, w = int(dims[0]), int(dims[1])
        fwd = _linop_tables(name, *tables[:4], h, w)
        adj = _linop_tables(name, *tables[4:], H, W)
        for t in fwd + adj:
            if t.dtype not in (torch.int32, torch.float32):
                raise OsmosisHipError(f"{name}: band tables are start int32 / wt fp32")
        # (four tables, a min and a max each: eight device-to-host reads per call -- this functional operator is off the fused loop,
        #  which hands the operator's own checked tables to osm_phys_optimize_lin; an out-of-range start would be an out-of-bounds read)
        for (start, wt), n_in in zip(((fwd[0], fwd[1]), (fwd[2], fwd[3]), (adj[0], adj[1]), (adj[2], adj[3])), (H, W, h, w)):
            if start.numel() and (int(start.min()) < 0 or int(start.max()) + wt.shape[1] > n_in):
                raise OsmosisHipError(f"{name}: a band table reads outside [0, {n_in})")
        lin.h, lin.w = h, w
        lin.start_h, lin.wt_h, lin.start_w, lin.wt_w = (ops.ptr(t) for t in fwd)
        lin.tstart_h, lin.twt_h, lin.tstart_w, lin.twt_w = (ops.ptr(t) for t in adj)
        lin.Kh, lin.Kw, lin.tKh, lin.tKw = fwd[1].shape[1], fwd[3].shape[1], adj[1].shape[1], adj[3].shape[1]
        lin._keep = fwd + adj
    elif family == 1:
        if len(tables) != 3 or len(dims) != 2:
            raise OsmosisHipError(f"{name}: a psf operator is the tap list dy, dx, w and dims = [Ry, Rx]")
        dy, dx, tw = (t.contiguous() for t in tables)
        if dy.dim() != 1 or dy.dtype != torch.int32 or dx.dtype != torch.int32 or tw.dtype != torch.float32 \
                or tuple(dx.shape) != tuple(dy.shape) or tuple(tw.shape) != tuple(dy.shape) or dy.numel() < 1:
            raise OsmosisHipError(f"{name}: expected dy int32 [T], dx int32 [T], w fp32 [T]")
        h, w = H, W
        lin.h, lin.w, lin.Ry, lin.Rx, lin.T = H, W, int(dims[0]), int(dims[1]), int(tw.shape[0])
        if not (0 <= lin.Ry < H and 0 <= lin.Rx < W):
            raise OsmosisHipError(f"{name}: reflection padding needs 0 <= Ry < H and 0 <= Rx < W")
        lin.dy, lin.dx, lin.tap_w = ops.ptr(dy), ops.ptr(dx), ops.ptr(tw)
        lin._keep = (dy, dx, tw)
    else:
        raise OsmosisHipError(f"{name}: family must be 0 (separable) or 1 (psf)")
    if tuple(y.shape) != (B, 3, h, w):
        raise OsmosisHipError(f"{name}: expected y [{B},3,{h},{w}] on the operator's grid, got {tuple(y.shape)}")
    hw, P, dev = h * w, ops.phys_lin_planes(d), x0.device
    f32 = dict(device=dev, dtype=torch.float32)
    phi_new = phi.detach().clone().contiguous()
    red, loss, g = torch.zeros(B * 16, **f32), torch.zeros(B, **f32), torch.empty_like(x0)
    ops.phys_optimize_lin(d, lin, x0, y.contiguous(), None if mask is None else _mask_rows(name, mask, y), phi_new,
                          torch.empty(B, P, HW, **f32), torch.empty(B, P, hw, **f32), torch.empty(B, 3, hw, **f32),
                          torch.empty(B, 3, HW, **f32), torch.empty(B * ops.phys_nblk(hw), **f32),
                          torch.empty(B * ops.phys_nblk(HW) * 16, **f32), red, loss, g, 1 if freeze_phi else n_inner, freeze_phi)
    return loss, g, phi_new


@phys_loss_grad_lin.register_fake
def _phys_loss_grad_lin_fake(x0, y, mask, phi, icfg, fcfg, n_inner, freeze_phi, family, tables, dims):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0), torch.empty_like(phi)


# ---- blind deblurring: the 'ps' data term through a PSF whose weights are learnt; the only operator here that mutates an argument
@torch.library.custom_op("osmosis::ps_blind_loss_grad", mutates_args=("w",), device_types="cuda")
def ps_blind_loss_grad(x0: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], dy: torch.Tensor, dx: torch.Tensor, w: torch.Tensor,
                       Ry: int, Rx: int, n_iter: int, eta: float, l1: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """One guided sub-step of a `blind_blur` data term (osm_ps_blind_optimize, include/osmosis_blind.h): x0 [B,C,H,W] (C >= 3),
    y [B,3,H,W], the optional mask ([B,3,H,W] / [B,1,H,W]), the tap list dy, dx int32 [T] and the weights w fp32 [T], which are
    STEPPED IN PLACE n_iter times (one PSF for the batch).  Returns (loss [B], g = A(w)^T d loss / d (A x0) on the colour planes, 0
    beyond), both for the weights before the last step."""
    name = "osmosis::ps_blind_loss_grad"
    B, HW = _chw(x0)
    C, H, W = x0.shape[1], x0.shape[2], x0.shape[3]
    if C < 3 or tuple(y.shape) != (B, 3, H, W):
        raise OsmosisHipError(f"{name}: expected x0 [B,C>=3,H,W] and y [B,3,H,W], got {tuple(x0.shape)} and {tuple(y.shape)}")
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape) or tuple(w.shape) != tuple(dy.shape) or not w.is_contiguous():
        raise OsmosisHipError(f"{name}: expected dy [T], dx [T] and a contiguous w [T], got {tuple(dy.shape)}, {tuple(dx.shape)}, {tuple(w.shape)}")
    f32 = dict(device=x0.device, dtype=torch.float32)
    loss, g = torch.zeros(B, **f32), torch.empty_like(x0)
    ops.ps_blind_optimize(x0.contiguous(), y.contiguous(), None if mask is None else _mask_rows(name, mask, y), dy.contiguous(),
                          dx.contiguous(), w, Ry, Rx, B, C, H, W, torch.empty(B, 3, HW, **f32), torch.empty(B, 3, HW, **f32),
                          torch.empty(B * ops.phys_nblk(HW), **f32), torch.empty(B * ops.tap_grad_nparts(3, H, W) * w.numel(), **f32),
                          loss, g, n_iter, eta, l1)
    return loss, g


@ps_blind_loss_grad.register_fake
def _ps_blind_loss_grad_fake(x0, y, mask, dy, dx, w, Ry, Rx, n_iter, eta, l1):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0)


@torch.library.custom_op("osmosis::ps_blind_loss_grad_s", mutates_args=("w",), device_types="cuda")
def ps_blind_loss_grad_s(x0: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], dy: torch.Tensor, dx: torch.Tensor, w: torch.Tensor,
                         Ry: int, Rx: int, n_iter: int, eta: float, l1: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """`osmosis::ps_blind_loss_grad` with weight sets (osm_ps_blind_optimize_s, include/osmosis_psfset.h): w fp32 [nb,nc,T], nb in
    {1, B} (one PSF per image), nc in {1, 3} (one per colour plane), every set STEPPED IN PLACE n_iter times from its own images /
    planes.  Returns (loss [B], g) for the weights before the last step."""
    name = "osmosis::ps_blind_loss_grad_s"
    B, HW = _chw(x0)
    C, H, W = x0.shape[1], x0.shape[2], x0.shape[3]
    if C < 3 or tuple(y.shape) != (B, 3, H, W):
        raise OsmosisHipError(f"{name}: expected x0 [B,C>=3,H,W] and y [B,3,H,W], got {tuple(x0.shape)} and {tuple(y.shape)}")
    if dy.dim() != 1 or tuple(dx.shape) != tuple(dy.shape) or w.dim() != 3 or w.shape[2] != dy.shape[0] or w.shape[0] not in (1, B) \
            or w.shape[1] not in (1, 3) or not w.is_contiguous():
        raise OsmosisHipError(f"{name}: expected dy [T], dx [T] and a contiguous w [nb,nc,T] with nb in (1, {B}), nc in (1, 3), got "
                              f"{tuple(dy.shape)}, {tuple(dx.shape)}, {tuple(w.shape)}")
    f32 = dict(device=x0.device, dtype=torch.float32)
    loss, g = torch.zeros(B, **f32), torch.empty_like(x0)
    ops.ps_blind_optimize_s(x0.contiguous(), y.contiguous(), None if mask is None else _mask_rows(name, mask, y), dy.contiguous(),
                            dx.contiguous(), w, Ry, Rx, B, C, H, W, torch.empty(B, 3, HW, **f32), torch.empty(B, 3, HW, **f32),
                            torch.empty(B * ops.phys_nblk(HW), **f32), torch.empty(B * ops.tap_grad_nparts(3, H, W) * w.shape[2], **f32),
                            loss, g, n_iter, eta, l1)
    return loss, g


@ps_blind_loss_grad_s.register_fake
def _ps_blind_loss_grad_s_fake(x0, y, mask, dy, dx, w, Ry, Rx, n_iter, eta, l1):
    return x0.new_empty((x0.shape[0],)), torch.empty_like(x0)


# ---- range-map depth prior of the Osmosis data term (include/osmosis_depthprior.h): adds its envelope gradient INTO g
@torch.library.custom_op("osmosis::depth_prior_loss_grad", mutates_args=("g",), device_types="cuda")
def depth_prior_loss_grad(x0: torch.Tensor, z: torch.Tensor, m: torch.Tensor, g: torch.Tensor, align: str, loss: str, weight: float,
                          scale: float, scale_min: float, depth_type: int, dval: List[float]) -> Tuple[torch.Tensor, torch.Tensor]:
    """The range-map depth prior on x0 [B,4,H,W] (osm_depth_loss_grad): z, m [B,1,H,W] fp32 (range, confidence in [0, 1]; m = 0 where
    there is no range), g [B,4,H,W] = dL/dx0 of the data term, whose depth plane receives `weight` times the gradient of the
    prior's loss IN PLACE where m > 0 (nothing else of g is written).  align 'none' | 'scale' | 'affine', loss 'norm' | 'mse';
    depth_type / dval: the operator's depth conversion.  Returns (depth_loss fp32 [B], without the weight; fit float64 [B,4] =
    a, c, gs, L)."""
    name = "osmosis::depth_prior_loss_grad"
    B, HW = _chw(x0)
    if x0.shape[1] != 4 or tuple(g.shape) != tuple(x0.shape) or g.dtype != torch.float32 or not g.is_contiguous():
        raise OsmosisHipError(f"{name}: expected x0 [B,4,H,W] and a contiguous fp32 g of its shape, got {tuple(x0.shape)} and {tuple(g.shape)}")
    want = (B, 1, x0.shape[2], x0.shape[3])
    if tuple(z.shape) != want or tuple(m.shape) != want or len(dval) != 3:
        raise OsmosisHipError(f"{name}: expected z and m {list(want)} and three dval entries, got {tuple(z.shape)} and {tuple(m.shape)}")
    try:
        d = ops.depth_desc(align, loss, weight, scale, scale_min, depth_type, dval, B, HW)
    except ValueError as e:
        raise OsmosisHipError(f"{name}: {e}") from None
    dev = x0.device
    part = torch.empty(B * ops.depth_nblk(HW) * 8, device=dev, dtype=torch.float64)
    fit = torch.empty(B, 4, device=dev, dtype=torch.float64)
    depth_loss = torch.empty(B, device=dev, dtype=torch.float32)
    ops.depth_loss_grad(d, x0, z.contiguous().view(B, 1, HW), m.contiguous().view(B, 1, HW), part, fit, depth_loss, g)
    return depth_loss, fit


@depth_prior_loss_grad.register_fake
def _depth_prior_loss_grad_fake(x0, z, m, g, align, loss, weight, scale, scale_min, depth_type, dval):
    return x0.new_empty((x0.shape[0],)), x0.new_empty((x0.shape[0], 4), dtype=torch.float64)


# ---- few-step solvers (include/osmosis_solver.h): the state update of a DDIM / DPM-Solver++ 2M step, in place
@torch.library.custom_op("osmosis::solver_update", mutates_args=("x_next", "hist"), device_types="cuda")
def solver_update(x0: torch.Tensor, x: torch.Tensor, hist: torch.Tensor, g: Optional[torch.Tensor], dx_unet: Optional[torch.Tensor],
                  noise: Optional[torch.Tensor], coef: torch.Tensor, srow: torch.Tensor, scale: torch.Tensor, clip: float,
                  x_next: torch.Tensor) -> torch.Tensor:
    """osm_solver_update_c: x_next = A x + B0 x0 + B1 hist + S noise - scale[c] clamp(c0 g + dx_unet), written IN PLACE, then
    hist <- x0 IN PLACE (read only when B1 != 0).  coef: the posterior row; srow = [A, B0, B1, S, noise_on, 0, 0, t_model], a row of
    `gaussian_diffusion.solver_table` as `_Chain.open` lays it out; scale [C]; clip < 0: no clamp.  Returns grad = c0 g + dx_unet
    (zeros without g).  x_next may be x itself only through the C ABI (an operator argument that is mutated cannot alias another)."""
    name = "osmosis::solver_update"
    B, HW = _chw(x0)
    Cc = _channel_scale(name, scale, x0)
    for t, what in ((x, "x"), (hist, "hist"), (x_next, "x_next"), (g, "g"), (dx_unet, "dx_unet"), (noise, "noise")):
        if t is not None and (tuple(t.shape) != tuple(x0.shape) or t.dtype != torch.float32 or not t.is_contiguous()):
            raise OsmosisHipError(f"{name}: {what} must be a contiguous fp32 tensor of x0's shape {tuple(x0.shape)}")
    if coef.numel() < 8 or srow.numel() < 8:
        raise OsmosisHipError(f"{name}: coef and srow are rows of 8 floats")
    grad = torch.zeros_like(x0) if g is None else torch.empty_like(x0)
    ops.solver_update_c(x0, x, hist, g, dx_unet, noise, coef, srow, scale, clip, x_next, None if g is None else grad, None, B, Cc, HW)
    return grad


@solver_update.register_fake
def _solver_update_fake(x0, x, hist, g, dx_unet, noise, coef, srow, scale, clip, x_next):
    return torch.empty_like(x0)


# ---- robust data term (include/osmosis_robust.h): the IRLS weights of a sub-step folded into the mask, written IN PLACE
@torch.library.custom_op("osmosis::robust_mask", mutates_args=("m_eff", "omega", "sigma", "n_valid"), device_types="cuda")
def robust_mask(pred: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], m_eff: torch.Tensor, omega: torch.Tensor,
                sigma: torch.Tensor, n_valid: torch.Tensor, pa: float, pb: float, loss: str, c: float, scale: float, sigma_min: float,
                per_pixel: bool) -> None:
    """osm_robust_mask: e = y - (pa pred[:, 0:3] + pb) (pred [B,P>=3,H,W], y [B,3,H,W]); sigma [B] = max(1.4826 median |e|, sigma_min)
    over the entries with mask > 0 (mask [B,3,H,W] or [B,1,H,W], None: ones) and e finite, n_valid [B] int32 their number -- or, with
    `scale` > 0, sigma is that value and neither is written (`scale` = 0 selects the mad scale); m_eff = mask sqrt(omega) and omega
    [B,3,H,W] of loss 'huber' | 'tukey' | 'cauchy' at u = |e| / (c sigma), all written IN PLACE."""
    name = "osmosis::robust_mask"
    B, hw = _chw(y)
    if pred.dim() != 4 or pred.shape[0] != B or pred.shape[1] < 3 or pred.shape[2:] != y.shape[2:] or y.shape[1] != 3 \
            or pred.dtype != torch.float32 or not pred.is_contiguous():
        raise OsmosisHipError(f"{name}: expected a contiguous fp32 pred [B,P>=3,H,W] and y [B,3,H,W], got {tuple(pred.shape)} and "
                              f"{tuple(y.shape)}")
    for t, what in ((m_eff, "m_eff"), (omega, "omega")):
        if tuple(t.shape) != tuple(y.shape) or t.dtype != torch.float32 or not t.is_contiguous():
            raise OsmosisHipError(f"{name}: {what} must be a contiguous fp32 tensor of y's shape {tuple(y.shape)}")
    if tuple(sigma.shape) != (B,) or sigma.dtype != torch.float32 or tuple(n_valid.shape) != (B,) or n_valid.dtype != torch.int32:
        raise OsmosisHipError(f"{name}: sigma must be fp32 [{B}] and n_valid int32 [{B}]")
    if not scale >= 0.0:
        raise OsmosisHipError(f"{name}: scale must be > 0 (a fixed sigma) or 0 (the mad scale), got {scale}")
    try:
        d = ops.robust_desc(loss, c, "mad" if scale == 0.0 else scale, sigma_min, per_pixel, B, hw)
    except ValueError as err:
        raise OsmosisHipError(f"{name}: {err}") from None
    e = torch.empty_like(y)
    ops.robust_mask(d, pred, pa, pb, y, None if mask is None else _mask_rows(name, mask, y), e, sigma, n_valid, m_eff, omega)


@robust_mask.register_fake
def _robust_mask_fake(pred, y, mask, m_eff, omega, sigma, n_valid, pa, pb, loss, c, scale, sigma_min, per_pixel):
    return None


# ---- learnt vignetting gain field (include/osmosis_gain.h): the sub-step's node steps and (y', M G), written IN PLACE
@torch.library.custom_op("osmosis::gain_prepare", mutates_args=("nodes", "y_eff", "m_eff", "field", "t", "s", "cs"), device_types="cuda")
def gain_prepare(F: torch.Tensor, y: torch.Tensor, mask: Optional[torch.Tensor], nodes: torch.Tensor, y_eff: torch.Tensor,
                 m_eff: torch.Tensor, field: torch.Tensor, t: torch.Tensor, s: torch.Tensor, cs: torch.Tensor, loss: str, eta: float,
                 n_iter: int, smooth: float, g_min: float, learn: bool, freeze_phi: bool) -> None:
    """osm_gain_prepare: with G the bilinear interpolation of nodes [B,gh,gw] over y's grid, `n_iter` x (the gradient of the `loss`
    'norm' | 'mse' of the model G F with respect to the nodes on F [B,P,H,W] (P = 4: plane 3 the depth weight), y [B,3,H,W] and mask
    ([B,3,H,W] or [B,1,H,W], None: ones); the projected step of include/osmosis_gain.h) unless `freeze_phi` or not `learn`, then
    y_eff = (y + 1) / G - 1, m_eff = mask G [B,3,H,W] and field = G [B,1,H,W]; t [B,H,gw], s [B,H] and cs [B, gh gw + 1] float64 are
    the workspaces.  Everything is written IN PLACE."""
    name = "osmosis::gain_prepare"
    B, hw = _chw(y)
    if y.dim() != 4 or y.shape[1] != 3 or F.dim() != 4 or F.shape[0] != B or F.shape[1] not in (3, 4) or F.shape[2:] != y.shape[2:] \
            or F.dtype != torch.float32 or not F.is_contiguous():
        raise OsmosisHipError(f"{name}: expected a contiguous fp32 F [B,3 or 4,H,W] and y [B,3,H,W], got {tuple(F.shape)} and "
                              f"{tuple(y.shape)}")
    if nodes.dim() != 3 or nodes.shape[0] != B:
        raise OsmosisHipError(f"{name}: nodes must be [B,gh,gw], got {tuple(nodes.shape)}")
    if loss not in ("norm", "mse"):
        raise OsmosisHipError(f"{name}: loss must be 'norm' or 'mse', got {loss!r}")
    H, W = y.shape[2], y.shape[3]
    try:
        d = ops.gain_desc(tuple(nodes.shape[1:]), eta, n_iter, smooth, g_min, learn, 0 if loss == "norm" else 1, F.shape[1], B, H, W)
        ops.gain_prepare(d, ops.gain_tables(H, W, d.gh, d.gw, y.device), F, y.contiguous(),
                         None if mask is None else _mask_rows(name, mask, y), nodes, t, s, cs, y_eff, m_eff, field, freeze_phi=freeze_phi)
    except ValueError as err:
        raise OsmosisHipError(f"{name}: {err}") from None


@gain_prepare.register_fake
def _gain_prepare_fake(F, y, mask, nodes, y_eff, m_eff, field, t, s, cs, loss, eta, n_iter, smooth, g_min, learn, freeze_phi):
    return None


OPS_C = ("posterior_c", "posterior_clip_c", "posterior_dynthr_c", "posterior_bwd_c", "guide_update_c", "guide_update_rng_c",
         "ddim_update_c", "ps_loss_grad_c")
OPS = ("unet_fwd", "unet_bwd_data", "posterior", "posterior_clip", "clamp_bwd", "quantile_abs", "posterior_dynthr", "dynthr_bwd", "posterior_bwd", "guide_update", "guide_update_rng", "ddim_update", "phys_loss_grad", "phys_loss_grad_m",
       "ps_loss_grad_mc", "exposure_mask", "recon_fullres", "tile_gather", "tile_blend", "linop_apply", "psf_apply", "phys_loss_grad_lin",
       "phys_loss_grad_g", "ps_blind_loss_grad", "depth_prior_loss_grad", "solver_update", "robust_mask", "gain_prepare", "psf_apply_s",
       "ps_blind_loss_grad_s", "psf_field_apply", "field_tap_grad", "field_tap_step") + OPS_C
