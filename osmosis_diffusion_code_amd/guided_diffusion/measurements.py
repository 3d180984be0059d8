"""Measurement operators and noisers -- registry surface of the reference's
guided_diffusion/measurements.py (register_operator/get_operator :19-38, register_noise/get_noise
:444-459) with the learnable physical operators re-designed for the fused HIP guidance kernels.

Reference semantics kept:
  * `get_operator(name, device=, batch_size=, **cfg)` builds a fresh operator (phi re-initialised
    per image) and sets `operator.__name__ = name`; unknown / duplicate names raise NameError.
  * phi values arrive as strings ("1.1,0.95,0.95"), etas as strings or floats ("1e-5"),
    `phi_*_learn_flag=False` freezes a variable (eta 0)            (measurements.py:213-249)
  * plain SGD `phi <- phi - eta * dL/dphi` (`optimizer: sgd`, or the 'GD' branch: same math), or any elementwise torch.optim
    class the reference's factory knows (adam, adamw, adamax, rmsprop, adagrad, adadelta, asgd, rprop: torch defaults, lr = eta
    per parameter group, state per operator instance = per image), all stepped on device inside osm_phys_finalize
    (measurements.py:266-303).  'sparseadam' / 'lbfgs' raise (they cannot step these parameters in the reference either).

Device state: `phi` is ONE fp32 device tensor [B][9] = phi_a[3] | phi_b[3] | phi_inf[3]
(`underwater_physical` and `haze_physical` keep phi_ab in the phi_a slots; haze's scalar is
replicated).  It is read and updated in place by osm_phys_* kernels (csrc/guidance.hip); the
Python object never syncs with the device unless the caller asks for values.
"""
import os
from abc import ABC, abstractmethod

import numpy as np
import torch

from .._lib import PhysDesc
from ..osmosis_utils import utils as utilso

__OPERATOR__ = {}


def register_operator(name: str):
    def wrapper(cls):
        if __OPERATOR__.get(name, None):
            raise NameError(f"Name {name} is already registered!")
        __OPERATOR__[name] = cls
        return cls
    return wrapper


def get_operator(name: str, **kwargs):
    if __OPERATOR__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined.")
    operator = __OPERATOR__[name](**kwargs)
    operator.__name__ = name
    return operator


class LinearOperator(ABC):
    @abstractmethod
    def forward(self, data, **kwargs):
        pass

    @abstractmethod
    def transpose(self, data, **kwargs):
        pass

    def ortho_project(self, data, **kwargs):
        return data - self.transpose(self.forward(data, **kwargs), **kwargs)

    def project(self, data, measurement, **kwargs):
        return self.ortho_project(measurement, **kwargs) - self.forward(data, **kwargs)


class _IdentityOperator(LinearOperator):
    def __init__(self, device, batch_size=1, **kwargs):
        self.device = device
        self.batch_size = batch_size

    def forward(self, data, **kwargs):
        return data

    def transpose(self, data, **kwargs):
        return data

    def ortho_project(self, data, **kwargs):
        return data

    def project(self, data, **kwargs):
        return data


@register_operator(name="noise")
class DenoiseOperator(_IdentityOperator):
    pass


@register_operator(name="rgb_guidance")
class RGBGuidanceOperator(_IdentityOperator):
    pass


# ----------------------------------------------------------------------------- separable banded linear operators
# A = R_h (x) R_w on each colour plane; a factor R [n_out, n_in] travels as a band table: row i has its K non-zeros at the columns
# start[i] .. start[i] + K - 1 with the values wt[i] (osm_linop_apply, include/osmosis_linop.h).  The transpose of a band is a
# band, so the adjoint is the same kernel with the transposed table.
def check_band(start, wt, n_in):
    """Raise ValueError unless every row of the band table reads inside [0, n_in): 0 <= start and start + K <= n_in."""
    start, wt = np.asarray(start), np.asarray(wt)
    if wt.ndim != 2 or start.shape != (wt.shape[0],) or wt.shape[1] < 1:
        raise ValueError(f"a band table is start [n_out] with wt [n_out, K >= 1], got {start.shape} and {wt.shape}")
    if start.size and (int(start.min()) < 0 or int(start.max()) + wt.shape[1] > n_in):
        raise ValueError(f"band table reads outside [0, {n_in}): start in [{int(start.min())}, {int(start.max())}], K = {wt.shape[1]}")


def dense_to_band(R):
    """(start int32 [n_out], wt float64 [n_out, K]) of a dense float64 matrix: K = the widest row span of non-zeros, a row's
    window shifted left where it would leave the matrix (the extra entries are the matrix's own zeros)."""
    R = np.asarray(R, dtype=np.float64)
    n_out, n_in = R.shape
    nz = R != 0
    first = np.where(nz.any(1), nz.argmax(1), 0)
    last = np.where(nz.any(1), n_in - 1 - nz[:, ::-1].argmax(1), 0)
    K = int((last - first).max()) + 1
    start = np.minimum(first, n_in - K).astype(np.int32)
    wt = R[np.arange(n_out)[:, None], start[:, None] + np.arange(K)[None, :]]
    check_band(start, wt, n_in)
    return start, np.ascontiguousarray(wt)


def band_to_dense(start, wt, n_in):
    """The dense matrix [n_out, n_in] of a band table, in the table's dtype."""
    check_band(start, wt, n_in)
    wt = np.asarray(wt)
    R = np.zeros((wt.shape[0], n_in), dtype=wt.dtype)
    R[np.arange(wt.shape[0])[:, None], np.asarray(start)[:, None] + np.arange(wt.shape[1])[None, :]] = wt
    return R


def _linop_op():
    from .. import torch_ops  # noqa: F401  (registers osmosis::linop_apply)
    return torch.ops.osmosis.linop_apply


class SeparableOperator(LinearOperator):
    """A linear map of the three colour planes that factors per axis, measurement [B,3,h,w] = R_h image R_w^T with (h, w) =
    `out_shape(H, W)`: no learnable parameters.  A subclass gives `axis_matrix(n_in)` (dense float64, built once per size on the
    host); the band tables of it and of its transpose (taken in float64 from the forward table, then cast to fp32) are cached per
    (H, W, device).  `forward` / `transpose` run osm_linop_apply on device tensors through `osmosis::linop_apply`, which is
    differentiable (its backward is the same operator with the other pair of tables), so autograd conditioning works too."""

    def __init__(self, device, batch_size=1, **kwargs):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.batch_size = batch_size
        self._host, self._dev = {}, {}

    def axis_matrix(self, n_in):
        raise NotImplementedError

    def axis_out(self, n_in):
        return n_in

    def axis_in(self, n_out):
        """The image size along an axis whose measurement has n_out samples (`transpose` takes its shape from this)."""
        return n_out

    def out_shape(self, H, W):
        return self.axis_out(H), self.axis_out(W)

    def host_tables(self, H, W):
        """{'fwd': (start_h, wt_h, start_w, wt_w), 'adj': the same of the transposes}: numpy, start int32, wt fp32."""
        tabs = self._host.get((H, W))
        if tabs is None:
            fwd, adj = [], []
            for n in (H, W):
                start, wt = dense_to_band(self.axis_matrix(n))
                tstart, twt = dense_to_band(band_to_dense(start, wt, n).T)      # float64 throughout; cast below
                fwd += [start, wt.astype(np.float32)]
                adj += [tstart, twt.astype(np.float32)]
            tabs = self._host[(H, W)] = {"fwd": tuple(fwd), "adj": tuple(adj)}
        return tabs

    def tables(self, H, W, device=None):
        """`host_tables` as device tensors."""
        device = torch.device(device if device is not None else self.device)
        key = (H, W, str(device))
        tabs = self._dev.get(key)
        if tabs is None:
            host = self.host_tables(H, W)
            tabs = self._dev[key] = {k: tuple(torch.from_numpy(a).to(device).contiguous() for a in v) for k, v in host.items()}
        return tabs

    def forward(self, data, **kwargs):
        H, W = data.shape[-2:]
        t = self.tables(H, W, data.device)
        h, w = self.out_shape(H, W)
        return _linop_op()(data, *t["fwd"], h, w, *t["adj"])

    def transpose(self, data, **kwargs):
        H, W = self.axis_in(data.shape[-2]), self.axis_in(data.shape[-1])
        t = self.tables(H, W, data.device)
        return _linop_op()(data, *t["adj"], H, W, *t["fwd"])


@register_operator(name="gaussian_blur")
class GaussianBlurOperator(SeparableOperator):
    """Blur with the k x k kernel g (x) g, g[t] ~ exp(-(t - r)^2 / 2 sigma^2), r = k // 2, normalised to sum 1 in float64, over the
    image padded by reflection (torch 'reflect': no edge repeat) -- the padding is folded into the band, a reflected tap adds onto
    the in-range column.  DPS config keys: kernel_size (odd), intensity (sigma).  The measurement has the image's size."""

    def __init__(self, device, kernel_size=61, intensity=3.0, batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        self.kernel_size, self.intensity = int(kernel_size), float(intensity)
        if self.kernel_size != kernel_size or self.kernel_size < 1 or self.kernel_size % 2 == 0:
            raise ValueError(f"gaussian_blur: kernel_size must be a positive odd integer, got {kernel_size!r}")
        if not self.intensity > 0:
            raise ValueError(f"gaussian_blur: intensity (sigma) must be positive, got {intensity!r}")

    def taps(self):
        r = self.kernel_size // 2
        g = np.exp(-((np.arange(self.kernel_size, dtype=np.float64) - r) ** 2) / (2.0 * self.intensity ** 2))
        return g / g.sum()

    def axis_matrix(self, n_in):
        r = self.kernel_size // 2
        if r >= n_in:
            raise ValueError(f"gaussian_blur: reflection padding needs kernel_size // 2 = {r} < the image side {n_in}")
        g = self.taps()
        R = np.zeros((n_in, n_in), dtype=np.float64)
        for i in range(n_in):
            for t in range(self.kernel_size):
                c = i + t - r
                c = -c if c < 0 else (2 * (n_in - 1) - c if c >= n_in else c)
                R[i, c] += g[t]
        return R


def _cubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x < 1, ((a + 2) * x - (a + 3)) * x * x + 1, np.where(x < 2, (((x - 5) * x + 8) * x - 4) * a, 0.0))


@register_operator(name="super_resolution")
class SuperResolutionOperator(SeparableOperator):
    """Downsampling by the integer `scale_factor` s >= 2: the measurement is H // s x W // s (H and W multiples of s).
    method 'bicubic' IS F.interpolate(mode='bicubic', align_corners=False, antialias=True), its weights computed analytically
    (scale = n_in / n_out, support = 2 scale, center = scale (i + 1/2), xmin = max(0, int(center - support + 1/2)), xsize =
    min(int(center + support + 1/2), n_in) - xmin, w_j = cubic((j + xmin - center + 1/2) / scale) with a = -0.5, normalised by
    their sum: a band 4 s wide); 'box' is the s x s mean (avg_pool2d)."""

    def __init__(self, device, scale_factor=4, method="bicubic", batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        self.scale_factor, self.method = int(scale_factor), str(method)
        if self.scale_factor != scale_factor or self.scale_factor < 2:
            raise ValueError(f"super_resolution: scale_factor must be an integer >= 2, got {scale_factor!r}")
        if self.method not in ("bicubic", "box"):
            raise ValueError(f"super_resolution: method must be 'bicubic' or 'box', got {method!r}")

    def axis_out(self, n_in):
        if n_in % self.scale_factor != 0 or n_in < self.scale_factor:
            raise ValueError(f"super_resolution: the image side {n_in} is no multiple of scale_factor {self.scale_factor}")
        return n_in // self.scale_factor

    def axis_in(self, n_out):
        return n_out * self.scale_factor

    def axis_matrix(self, n_in):
        n_out, s = self.axis_out(n_in), self.scale_factor
        R = np.zeros((n_out, n_in), dtype=np.float64)
        if self.method == "box":
            for i in range(n_out):
                R[i, i * s:(i + 1) * s] = 1.0 / s
            return R
        scale = n_in / n_out
        support = 2.0 * scale
        for i in range(n_out):
            center = scale * (i + 0.5)
            xmin = max(0, int(center - support + 0.5))
            xsize = min(int(center + support + 0.5), n_in) - xmin
            w = _cubic((np.arange(xsize, dtype=np.float64) + xmin - center + 0.5) / scale)
            R[i, xmin:xmin + xsize] = w / w.sum()
        return R


# ----------------------------------------------------------------------------- point-spread-function operators
# A 2-D kernel that does not factor per axis (motion blur, a measured PSF) travels as a tap list: the offsets (dy, dx) of its non-zeros
# from the anchor (the centre) and their weights (osm_psf_apply, include/osmosis_psf.h).  The adjoint is the same kernel launch with
# `adjoint` set: the transpose of reflection padding folds the mirrored taps back.
def _psf_op(sets=False):
    from .. import torch_ops  # noqa: F401  (registers osmosis::psf_apply and osmosis::psf_apply_s)
    return torch.ops.osmosis.psf_apply_s if sets else torch.ops.osmosis.psf_apply


def check_kernel_sets(kernel, per_image, per_channel, batch_size, what="psf"):
    """The float64 [nb,nc,kh,kw] array of the PSFs of an operator: `kernel` is [kh,kw], [3,kh,kw] with `per_channel`, [B,kh,kw] with
    `per_image` and [B,3,kh,kw] with both (B = batch_size); ValueError for a shape that does not match the flags, and for any
    kernel `check_kernel2d` refuses."""
    try:
        k = np.asarray(kernel, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: the kernel must be an array of numbers ({e})")
    want = 2 + bool(per_image) + bool(per_channel)
    if k.ndim != want:
        raise ValueError(f"{what}: with per_image={bool(per_image)}, per_channel={bool(per_channel)} the kernel is "
                         f"{'[B,' if per_image else '['}{'3,' if per_channel else ''}kh,kw], got shape {k.shape}")
    k = k.reshape((k.shape[0] if per_image else 1, k.shape[-3] if per_channel else 1) + k.shape[-2:])
    if per_channel and k.shape[1] != 3:
        raise ValueError(f"{what}: per_channel takes one kernel per colour plane (3), got {k.shape[1]}")
    if per_image and k.shape[0] != int(batch_size):
        raise ValueError(f"{what}: per_image takes one kernel per image of the batch: {k.shape[0]} kernels for batch_size {batch_size}")
    for b in range(k.shape[0]):
        for c in range(k.shape[1]):
            check_kernel2d(k[b, c], what)
    return k


def check_kernel2d(kernel, what="psf"):
    """The float64 [kh, kw] array of a PSF given as an array or a nested list; ValueError unless it is 2-D with odd sides (the anchor
    is the centre), finite, and not all zero."""
    try:
        k = np.asarray(kernel, dtype=np.float64)
    except (TypeError, ValueError) as e:
        raise ValueError(f"{what}: the kernel must be a 2-D array of numbers ({e})")
    if k.ndim != 2 or k.size == 0:
        raise ValueError(f"{what}: the kernel must be 2-D [kh, kw], got shape {k.shape}")
    if k.shape[0] % 2 == 0 or k.shape[1] % 2 == 0:
        raise ValueError(f"{what}: both sides of the kernel must be odd (the anchor is the centre), got {k.shape[0]} x {k.shape[1]}")
    if not np.isfinite(k).all():
        raise ValueError(f"{what}: the kernel holds non-finite values")
    if not (k != 0).any():
        raise ValueError(f"{what}: the kernel is all zero")
    return k


class PSFOperator(LinearOperator):
    """Blur of the three colour planes with one 2-D point-spread function over the image padded by reflection (torch 'reflect'), as
    cross-correlation -- F.conv2d(F.pad(x, reflect), k), what nn.Conv2d and the DPS `Blurkernel` compute: no learnable parameters, the
    measurement has the image's size.  A subclass gives `kernel2d()` (float64 [kh, kw], both sides odd, anchor at the centre); the
    non-zero taps are taken in row-major order, their weights cast to fp32, and cached as device tensors per device.  `forward` /
    `transpose` run osm_psf_apply through `osmosis::psf_apply`, which is differentiable (its backward is the same operator with
    `adjoint` flipped), so autograd conditioning works too.
    WEIGHT SETS (include/osmosis_psfset.h): `weight_sets` = (nb, nc), default (1, 1).  An operator with one PSF per image (nb =
    batch_size) and / or per colour plane (nc = 3) keeps its kernels in `_kernels` float64 [nb,nc,kh,kw] (`kernels()`); the tap list
    is then the row-major UNION of the kernels' non-zeros, a kernel without a tap there carries 0.0, and the weights are
    w [nb,nc,T]: plane p of image b is blurred with set (nb > 1 ? b : 0, nc > 1 ? p : 0) through `osmosis::psf_apply_s`.  Such an
    operator takes batches of exactly nb images (and nc planes); `kernel2d()` is what it was for one set and raises for more."""

    _sets = (1, 1)
    _kernels = None         # float64 [nb,nc,kh,kw] of an operator with more than one weight set

    def __init__(self, device, batch_size=1, **kwargs):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.batch_size = batch_size
        self._host, self._dev = None, {}

    @property
    def weight_sets(self):
        """(nb, nc): how many PSFs the operator carries per batch and per image -- (1, 1): one for every plane of every image."""
        return self._sets

    def _name(self):
        return getattr(self, "__name__", type(self).__name__)

    def kernel2d(self):
        raise NotImplementedError

    def _single(self, k):
        """`kernel2d()` of a subclass that may carry several kernels: the one kernel, or ValueError naming `kernels()`."""
        if self.weight_sets != (1, 1):
            raise ValueError(f"{self._name()}: the operator carries {self.weight_sets[0]} x {self.weight_sets[1]} point-spread functions "
                             f"(per image x per channel); kernel2d() is one kernel -- use kernels()")
        return k

    def kernels(self):
        """Every PSF of the operator, float64 [nb,nc,kh,kw]."""
        if self.weight_sets == (1, 1):
            return np.asarray(self.kernel2d(), dtype=np.float64)[None, None].copy()
        return self._kernels.copy()

    def host_taps(self):
        """(dy int32 [T], dx int32 [T], w fp32): the kernel's non-zeros in row-major order, offsets from the centre, w [T]; with more
        than one weight set the union of the kernels' non-zeros and w [nb,nc,T]."""
        if self._host is None and self.weight_sets != (1, 1):
            ks = self._kernels
            iy, ix = np.nonzero((ks != 0).any(axis=(0, 1)))                         # row-major union
            self._host = ((iy - ks.shape[2] // 2).astype(np.int32), (ix - ks.shape[3] // 2).astype(np.int32),
                          np.ascontiguousarray(ks[:, :, iy, ix].astype(np.float32)))
        if self._host is None:
            k = check_kernel2d(self.kernel2d(), self._name())
            iy, ix = np.nonzero(k)                                                  # row-major
            self._host = ((iy - k.shape[0] // 2).astype(np.int32), (ix - k.shape[1] // 2).astype(np.int32), k[iy, ix].astype(np.float32))
        return self._host

    def check_batch(self, B, P=3):
        """ValueError unless a batch of B images with P planes is one the operator's weight sets serve (nb in (1, B), nc in (1, P))."""
        nb, nc = self.weight_sets
        if nb > 1 and int(B) != nb:
            raise ValueError(f"{self._name()}: the operator carries one point-spread function per image of a batch of {nb} (per_image); "
                             f"got a batch of {int(B)}")
        if nc > 1 and int(P) != nc:
            raise ValueError(f"{self._name()}: the operator carries one point-spread function per colour plane ({nc}, per_channel); "
                             f"got {int(P)} planes")

    def radius(self):
        """(Ry, Rx): the largest |dy| and |dx| of the taps."""
        dy, dx, _ = self.host_taps()
        return int(np.abs(dy).max()), int(np.abs(dx).max())

    def taps(self, device=None):
        """`host_taps` as device tensors."""
        device = torch.device(device if device is not None else self.device)
        t = self._dev.get(str(device))
        if t is None:
            t = self._dev[str(device)] = tuple(self._to_device(a, device) for a in self.host_taps())
        return t

    def _to_device(self, a, device):
        return torch.from_numpy(a).to(device).contiguous()

    def out_shape(self, H, W):
        Ry, Rx = self.radius()
        if Ry >= H or Rx >= W:
            raise ValueError(f"{getattr(self, '__name__', type(self).__name__)}: reflection padding needs the kernel's reach {Ry} x {Rx} "
                             f"< the image sides {H} x {W}")
        return H, W

    def _apply(self, data, adjoint):
        self.out_shape(*data.shape[-2:])
        if self.weight_sets != (1, 1):
            self.check_batch(data.shape[0], data.shape[1])
            return _psf_op(True)(data, *self.taps(data.device), *self.radius(), adjoint)
        return _psf_op()(data, *self.taps(data.device), *self.radius(), adjoint)

    def forward(self, data, **kwargs):
        return self._apply(data, False)

    def transpose(self, data, **kwargs):
        return self._apply(data, True)


# the linear operators whose measurement lives on a grid of its own, `out_shape(H, W)`, and whose data term the fused `ps` loop
# evaluates with their own kernels (condition_methods.PosteriorSampling, sampling.restore_image)
GRID_OPERATORS = (SeparableOperator, PSFOperator)

MOTION_STEP = 0.5          # pixels between two samples of the trajectory
MOTION_TURN = 0.3          # standard deviation of the heading's change per sample at intensity 1, radians


def motion_trajectory(kernel_size=61, intensity=0.5, seed=0):
    """The camera path of `motion_kernel`, float64 [2 m + 1, 2] of (y, x) offsets from the centre, r = kernel_size // 2, m = 2 r:
    with rng = np.random.default_rng(seed), theta = rng.uniform(0, pi) and turn = rng.normal(size=(2, m)) (drawn in this order), arm
    a in (0, 1) leaves the centre with the heading theta + a pi and takes m steps of MOTION_STEP pixels, the heading changing by
    intensity * MOTION_TURN * turn[a, i] BEFORE step i; every point is clamped to [-r, r] per axis.  Order: arm 1 reversed, the
    centre, arm 0 -- one connected path through (0, 0); intensity 0: a straight segment of length 2 r."""
    k, s = int(kernel_size), float(intensity)
    if k != kernel_size or k < 1 or k % 2 == 0:
        raise ValueError(f"motion_blur: kernel_size must be a positive odd integer, got {kernel_size!r}")
    if not 0.0 <= s <= 1.0:
        raise ValueError(f"motion_blur: intensity must lie in [0, 1], got {intensity!r}")
    r = k // 2
    m = 2 * r
    rng = np.random.default_rng(seed)
    theta = rng.uniform(0.0, np.pi)
    turn = rng.normal(size=(2, m))
    arms = []
    for a in range(2):
        heading = theta + a * np.pi + np.cumsum(s * MOTION_TURN * turn[a])
        steps = MOTION_STEP * np.stack([np.sin(heading), np.cos(heading)], axis=1)
        arms.append(np.clip(np.cumsum(steps, axis=0), -r, r))
    return np.concatenate([arms[1][::-1], np.zeros((1, 2)), arms[0]], axis=0).reshape(2 * m + 1, 2)


def motion_kernel(kernel_size=61, intensity=0.5, seed=0):
    """The motion-blur PSF, float64 [kernel_size, kernel_size]: the points of `motion_trajectory(kernel_size, intensity, seed)`, each
    splatted with weight 1 onto its four neighbouring pixels bilinearly (pixel (r + floor y + a, r + floor x + b) gets
    (a ? fy : 1 - fy) (b ? fx : 1 - fx), fy = y - floor y; a pixel beyond the kernel can only get weight 0 and is dropped), the sum
    normalised to 1.  Deterministic in its three arguments, non-negative, the centre pixel always hit.  (DPS draws its kernels from
    the `motionblur` package; this definition stands in for it and does not reproduce that package's random stream.)"""
    return _splat_points(motion_trajectory(kernel_size, intensity, seed), int(kernel_size))


def _splat_points(pts, k):
    """float64 [k, k], sum 1: the points pts [n, 2] of (y, x) offsets from the centre (each within [-k // 2, k // 2] per axis), every
    one splatted bilinearly with weight 1 as `motion_kernel` states."""
    r = k // 2
    ker = np.zeros((k, k), dtype=np.float64)
    fl = np.floor(pts)
    frac = pts - fl
    for a in range(2):
        for b in range(2):
            wgt = (frac[:, 0] if a else 1.0 - frac[:, 0]) * (frac[:, 1] if b else 1.0 - frac[:, 1])
            iy, ix = fl[:, 0].astype(np.int64) + r + a, fl[:, 1].astype(np.int64) + r + b
            ok = (iy < k) & (ix < k) & (wgt > 0)
            np.add.at(ker, (iy[ok], ix[ok]), wgt[ok])
    return ker / ker.sum()


@register_operator(name="motion_blur")
class MotionBlurOperator(PSFOperator):
    """Blur with a random camera-shake trajectory, `motion_kernel(kernel_size, intensity, seed)`.  DPS config keys: kernel_size (odd,
    default 61), intensity (in [0, 1], default 0.5: 0 a straight streak, 1 the most erratic path); `seed` (default 0) picks the path.
    A LIST of seeds gives every image of the batch its own trajectory (`per_image`: weight sets (batch_size, 1)); its length must
    equal batch_size."""

    def __init__(self, device, kernel_size=61, intensity=0.5, seed=0, batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        self.per_image = isinstance(seed, (list, tuple))
        if self.per_image:
            if len(seed) != int(batch_size) or len(seed) < 1:
                raise ValueError(f"motion_blur: a list under `seed` is one trajectory per image: {len(seed)} seeds for batch_size {batch_size}")
            self._kernels = np.stack([motion_kernel(kernel_size, intensity, s) for s in seed])[:, None]
            self._sets = (len(seed), 1)
            self._kernel = self._kernels[0, 0]
            seed = list(seed)
        else:
            self._kernel = motion_kernel(kernel_size, intensity, seed)              # validates its arguments
        self.kernel_size, self.intensity, self.seed = int(kernel_size), float(intensity), seed

    def kernel2d(self):
        return self._single(self._kernel)


@register_operator(name="psf_blur")
class PSFBlurOperator(PSFOperator):
    """Blur with a point-spread function of the user's: `kernel` is a 2-D array, a nested list, or the path of a .npy file holding one
    (both sides odd, finite; the anchor is the centre, applied as cross-correlation); `normalize` (default True) divides it by its
    float64 sum, which must not be zero.
    `per_channel`: `kernel` is [3,kh,kw], one PSF per colour plane (lateral chromatic aberration, wavelength-dependent scattering);
    `per_image`: [B,kh,kw] with B = batch_size, one per image; both: [B,3,kh,kw].  A shape that does not match the flags raises;
    `normalize` acts per kernel."""

    def __init__(self, device, kernel=None, normalize=True, batch_size=1, per_image=False, per_channel=False, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        self.per_image, self.per_channel = bool(per_image), bool(per_channel)
        if kernel is None:
            raise ValueError("psf_blur: a `kernel` is required (a 2-D array, a nested list or the path of a .npy file)")
        if isinstance(kernel, (str, bytes)) or hasattr(kernel, "__fspath__"):
            kernel = np.load(kernel, allow_pickle=False)
        if isinstance(kernel, torch.Tensor):
            kernel = kernel.detach().cpu().numpy()
        if self.per_image or self.per_channel:
            ks = check_kernel_sets(kernel, self.per_image, self.per_channel, batch_size, "psf_blur")
            if normalize:
                totals = ks.sum(axis=(2, 3), keepdims=True)
                if (totals == 0.0).any() or not np.isfinite(totals).all():
                    raise ValueError(f"psf_blur: normalize divides every kernel by its sum; the sums are {totals.reshape(ks.shape[:2]).tolist()}")
                ks = ks / totals
            self._kernels, self._sets = ks, tuple(ks.shape[:2])
            self._kernel, self.normalize = ks[0, 0], bool(normalize)
            return
        k = check_kernel2d(kernel, "psf_blur")
        if normalize:
            total = float(k.sum())
            if total == 0.0 or not np.isfinite(total):
                raise ValueError(f"psf_blur: normalize divides by the kernel's sum, which is {total}")
            k = k / total
        self._kernel, self.normalize = k, bool(normalize)

    def kernel2d(self):
        return self._single(self._kernel)


# ----------------------------------------------------------------------------- a field of PSFs: spatially varying blur
FIELD_MAX_GRID = 32        # nodes per axis (include/osmosis_psffield.h; the gain field's limit)
FIELD_MAX_KERNEL = 61      # the largest side of a node kernel (the window a workgroup stages: halo <= 32 per side, then slower)


def _field_grid(grid, what):
    try:
        gh, gw = (int(v) for v in grid)
        ok = (gh, gw) == tuple(grid)
    except (TypeError, ValueError):
        ok = False
    if not ok or not (2 <= gh <= FIELD_MAX_GRID and 2 <= gw <= FIELD_MAX_GRID):
        raise ValueError(f"{what}: grid must be a pair of ints (gh, gw) within 2 .. {FIELD_MAX_GRID} per side, got {grid!r}")
    return gh, gw


def _field_kernel_size(kernel_size, what):
    k = kernel_size
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k % 2 == 0 or k > FIELD_MAX_KERNEL:
        raise ValueError(f"{what}: kernel_size must be a positive odd integer <= {FIELD_MAX_KERNEL}, got {kernel_size!r}")
    return int(k)


def radial_defocus_field(kernel_size=31, sigma_center=0.5, sigma_corner=3.0, grid=(5, 5)):
    """A dome port's field curvature, float64 [gh,gw,k,k]: node (jy, jx) carries the Gaussian of standard deviation
    sigma = sigma_center + (sigma_corner - sigma_center) rho^2, sampled at the pixel centres and normalised to sum 1 in float64;
    rho = sqrt((uy^2 + ux^2) / 2) with uy = 2 jy / (gh - 1) - 1, ux alike: the node's distance from the centre over the corner's,
    each axis normalised by its own half side (0 at the centre, 1 at the four corners)."""
    what = "field_blur: radial_defocus"
    k = _field_kernel_size(kernel_size, what)
    gh, gw = _field_grid(grid, what)
    sc, se = float(sigma_center), float(sigma_corner)
    if not (np.isfinite(sc) and np.isfinite(se) and sc > 0 and se > 0):
        raise ValueError(f"{what}: sigma_center and sigma_corner must be positive numbers, got {sigma_center!r}, {sigma_corner!r}")
    a = np.arange(k, dtype=np.float64) - k // 2
    d2 = a[:, None] ** 2 + a[None, :] ** 2
    out = np.empty((gh, gw, k, k), dtype=np.float64)
    for jy in range(gh):
        for jx in range(gw):
            uy, ux = 2.0 * jy / (gh - 1) - 1.0, 2.0 * jx / (gw - 1) - 1.0
            sigma = sc + (se - sc) * ((uy * uy + ux * ux) / 2.0)
            ker = np.exp(-d2 / (2.0 * sigma * sigma))
            out[jy, jx] = ker / ker.sum()
    return out


def roll_shake_field(kernel_size=31, angle_deg=1.0, grid=(5, 5), image_size=(256, 256)):
    """A hand-held roll about the optical axis during the exposure, float64 [gh,gw,k,k]: node (jy, jx) sits at
    (y, x) = (jy (H - 1) / (gh - 1), jx (W - 1) / (gw - 1)) of an image_size = (H, W) frame, at the offset (ry, rx) and the distance
    r from the image centre ((H - 1) / 2, (W - 1) / 2); its PSF is a straight streak through the kernel's centre along the tangent
    (rx, -ry) / r of the circle about the image centre through the node, of length angle r pixels (angle in radians): the points
    i MOTION_STEP along the tangent for |i| <= floor(angle r / (2 MOTION_STEP)), each clamped to [-k // 2, k // 2] per axis and
    splatted bilinearly as `motion_kernel` does, the sum normalised to 1.  A node at the image centre carries the delta."""
    what = "field_blur: roll_shake"
    k = _field_kernel_size(kernel_size, what)
    gh, gw = _field_grid(grid, what)
    ang = float(angle_deg)
    if not (np.isfinite(ang) and ang >= 0.0):
        raise ValueError(f"{what}: angle_deg must be a finite number >= 0, got {angle_deg!r}")
    try:
        H, W = (int(v) for v in image_size)
        ok = (H, W) == tuple(image_size) and H >= 2 and W >= 2
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"{what}: image_size must be a pair of ints (H, W) >= 2, got {image_size!r}")
    half = k // 2
    out = np.empty((gh, gw, k, k), dtype=np.float64)
    for jy in range(gh):
        for jx in range(gw):
            ry, rx = jy * (H - 1) / (gh - 1) - (H - 1) / 2.0, jx * (W - 1) / (gw - 1) - (W - 1) / 2.0
            r = float(np.hypot(ry, rx))
            n = int(np.floor(np.deg2rad(ang) * r / (2.0 * MOTION_STEP))) if r > 0 else 0
            s = np.arange(-n, n + 1, dtype=np.float64) * MOTION_STEP
            t = np.array([rx / r, -ry / r]) if r > 0 else np.zeros(2)
            out[jy, jx] = _splat_points(np.clip(s[:, None] * t[None, :], -half, half), k)
    return out


def _field_op():
    from .. import torch_ops  # noqa: F401  (registers osmosis::psf_field_apply)
    return torch.ops.osmosis.psf_field_apply


@register_operator(name="field_blur")
class PSFFieldOperator(PSFOperator):
    """Spatially varying blur: a FIELD of point-spread functions K_n on a gh x gw node grid that spans the frame (the nodes sit where
    the gain field's do: on the image corners inclusive), every pixel p blurred with the bilinear interpolation sum_n hat_n(p) K_n of
    the four corner kernels of its cell, over reflection padding, as cross-correlation (osm_psf_field_apply,
    include/osmosis_psffield.h; `forward` / `transpose` run it through `osmosis::psf_field_apply`, which is differentiable).
    No learnable parameters; the measurement has the image's size.  The field is shared by the images of a batch and by the colour
    planes: `weight_sets` stays (1, 1).
    Config keys (an unknown one raises ValueError): EITHER `kernels`, a [gh,gw,kh,kw] array, nested list or the path of a .npy file
    (odd sides, finite, no all-zero node: `check_kernel2d` per node) with `normalize` (default True: every node over its own float64
    sum), OR `model`: 'radial_defocus' with {kernel_size=31, sigma_center=0.5, sigma_corner=3.0, grid=[5,5]}
    (`radial_defocus_field`) or 'roll_shake' with {kernel_size=31, angle_deg=1.0, grid=[5,5], image_size=[256,256]}
    (`roll_shake_field`); `simulate` is the driver's.  `per_image` / `per_channel` are refused: a field per image or per channel is
    out of scope.
    `kernels()` float64 [gh,gw,kh,kw]; `grid` (gh, gw); `host_taps()` the row-major union of the nodes' non-zeros with w fp32
    [gh,gw,T]; `kernel2d()` raises: a field is never one PSF."""

    DRIVER_KEYS = ("simulate",)
    MODELS = {"radial_defocus": (radial_defocus_field, ("kernel_size", "sigma_center", "sigma_corner", "grid")),
              "roll_shake": (roll_shake_field, ("kernel_size", "angle_deg", "grid", "image_size"))}

    def __init__(self, device, kernels=None, normalize=True, model=None, batch_size=1, **kwargs):
        many = [k for k in ("per_image", "per_channel") if k in kwargs]
        if many:
            raise ValueError(f"field_blur: {', '.join(many)} is not supported -- the field is shared by the images of a batch and by the "
                             f"colour planes (a field per image or per channel is out of scope)")
        if (kernels is None) == (model is None):
            raise ValueError("field_blur: give either `kernels` ([gh,gw,kh,kw]) or `model` ('radial_defocus' | 'roll_shake'), not both")
        if model is not None and model not in self.MODELS:
            raise ValueError(f"field_blur: model must be one of {sorted(self.MODELS)}, got {model!r}")
        known = self.MODELS[model][1] if model is not None else ()
        unknown = sorted(set(kwargs) - set(self.DRIVER_KEYS) - set(known))
        if unknown:
            raise ValueError(f"field_blur: unknown config key(s) {unknown} (known: kernels, normalize, model"
                             f"{''.join(', ' + k for k in known)}, simulate)")
        super().__init__(device, batch_size)
        if model is not None:
            ks = self.MODELS[model][0](**{k: kwargs[k] for k in known if k in kwargs})
        else:
            if isinstance(kernels, (str, bytes)) or hasattr(kernels, "__fspath__"):
                if not str(os.fspath(kernels) if hasattr(kernels, "__fspath__") else kernels).endswith(".npy"):
                    raise ValueError(f"field_blur: kernels must be a [gh,gw,kh,kw] array of numbers, a nested list or the path of a .npy "
                                     f"file, got {kernels!r}")
                kernels = np.load(kernels, allow_pickle=False)
            if isinstance(kernels, torch.Tensor):
                kernels = kernels.detach().cpu().numpy()
            try:
                ks = np.asarray(kernels, dtype=np.float64)
            except (TypeError, ValueError) as e:
                raise ValueError(f"field_blur: kernels must be a [gh,gw,kh,kw] array of numbers ({e})")
            if ks.ndim != 4:
                raise ValueError(f"field_blur: kernels must be [gh,gw,kh,kw], got shape {ks.shape}")
            _field_grid(ks.shape[:2], "field_blur")
            for jy in range(ks.shape[0]):
                for jx in range(ks.shape[1]):
                    check_kernel2d(ks[jy, jx], f"field_blur: node ({jy}, {jx})")
            if max(ks.shape[2:]) > FIELD_MAX_KERNEL:
                raise ValueError(f"field_blur: a node kernel of {ks.shape[2]} x {ks.shape[3]} is larger than {FIELD_MAX_KERNEL} per side")
            if normalize:
                totals = ks.sum(axis=(2, 3), keepdims=True)
                if (totals == 0.0).any() or not np.isfinite(totals).all():
                    raise ValueError(f"field_blur: normalize divides every node by its sum; the sums are {totals.reshape(ks.shape[:2]).tolist()}")
                ks = ks / totals
        self._field = np.ascontiguousarray(ks)
        self.model, self.normalize = model, bool(normalize)

    @property
    def grid(self):
        """(gh, gw): the nodes per axis."""
        return tuple(int(v) for v in self._field.shape[:2])

    def kernel2d(self):
        raise ValueError(f"{self._name()}: the operator carries a field of {self.grid[0]} x {self.grid[1]} point-spread functions; "
                         f"kernel2d() is one kernel -- use kernels()")

    def kernels(self):
        """Every node's PSF, float64 [gh,gw,kh,kw]."""
        return self._field.copy()

    def host_taps(self):
        """(dy int32 [T], dx int32 [T], w fp32 [gh,gw,T]): the row-major union of the nodes' non-zeros, offsets from the centre; a node
        without a tap there carries 0.0."""
        if self._host is None:
            ks = self._field
            iy, ix = np.nonzero((ks != 0).any(axis=(0, 1)))                         # row-major union
            self._host = ((iy - ks.shape[2] // 2).astype(np.int32), (ix - ks.shape[3] // 2).astype(np.int32),
                          np.ascontiguousarray(ks[:, :, iy, ix].astype(np.float32)))
        return self._host

    def out_shape(self, H, W):
        gh, gw = self.grid
        if gh > H or gw > W:
            raise ValueError(f"{self._name()}: the node grid {gh} x {gw} has more nodes than the image has pixels ({H} x {W})")
        return super().out_shape(H, W)

    def field_tables(self, H, W, device=None):
        """The interpolation tables (iy0, fy, ix0, fx) of the node grid on an H x W image, on the device (`ops.field_tables`)."""
        from .. import ops
        return ops.field_tables(H, W, *self.grid, torch.device(device if device is not None else self.device))

    def _apply(self, data, adjoint):
        H, W = data.shape[-2:]
        self.out_shape(H, W)
        return _field_op()(data, *self.taps(data.device), *self.field_tables(H, W, data.device), *self.radius(), adjoint)


BLIND_MAX_KERNEL = 61      # the largest side of a learnt PSF (the window a workgroup of osm_psf_tap_grad stages: halo <= 32 per side)


def blind_init_kernel(kernel_size=31, init="gaussian", init_sigma=None):
    """The starting point of a learnt PSF, float64 [k, k], non-negative, summing to 1: `init` is 'gaussian' (standard deviation
    `init_sigma`, default k / 6, sampled at the pixel centres), 'delta' (the identity), 'uniform', or a kernel of the user's -- a
    2-D array, a nested list or the path of a .npy file (`check_kernel2d`; no side larger than k; centred in the k x k support)."""
    k = kernel_size
    if isinstance(k, bool) or not isinstance(k, (int, np.integer)) or k < 1 or k % 2 == 0:
        raise ValueError(f"blind_blur: kernel_size must be a positive odd integer, got {kernel_size!r}")
    k = int(k)
    if k > BLIND_MAX_KERNEL:
        raise ValueError(f"blind_blur: kernel_size {k} is larger than {BLIND_MAX_KERNEL}, the largest support the tap-gradient kernel stages")
    if isinstance(init, str) and init in ("gaussian", "delta", "uniform"):
        if init == "gaussian":
            sigma = k / 6.0 if init_sigma is None else float(init_sigma)
            if not (np.isfinite(sigma) and sigma > 0):
                raise ValueError(f"blind_blur: init_sigma must be a positive number, got {init_sigma!r}")
            a = np.arange(k, dtype=np.float64) - k // 2
            ker = np.exp(-(a[:, None] ** 2 + a[None, :] ** 2) / (2.0 * sigma * sigma))
        elif init == "delta":
            ker = np.zeros((k, k), dtype=np.float64)
            ker[k // 2, k // 2] = 1.0
        else:
            ker = np.ones((k, k), dtype=np.float64)
    else:
        if isinstance(init, (str, bytes)) or hasattr(init, "__fspath__"):
            if not str(os.fspath(init) if hasattr(init, "__fspath__") else init).endswith(".npy"):
                raise ValueError(f"blind_blur: init must be 'gaussian', 'delta', 'uniform', a 2-D array or the path of a .npy file, got {init!r}")
            init = np.load(init, allow_pickle=False)
        if isinstance(init, torch.Tensor):
            init = init.detach().cpu().numpy()
        given = check_kernel2d(init, "blind_blur")
        if (given < 0).any():
            raise ValueError("blind_blur: the init kernel must be non-negative (the estimate lives on the simplex)")
        kh, kw = given.shape
        if kh > k or kw > k:
            raise ValueError(f"blind_blur: the init kernel {kh} x {kw} is larger than kernel_size {k}")
        ker = np.zeros((k, k), dtype=np.float64)
        ker[(k - kh) // 2:(k - kh) // 2 + kh, (k - kw) // 2:(k - kw) // 2 + kw] = given
    return ker / ker.sum()


@register_operator(name="blind_blur")
class BlindBlurOperator(PSFOperator):
    """Blind deblurring: blur with ONE unknown 2-D point-spread function on the dense support kernel_size x kernel_size (T = k^2 taps
    in row-major order, Ry = Rx = k // 2) whose weights are LEARNT during sampling: they live in a device tensor `w` fp32 [T] that
    the step kernel overwrites between the network's forward and backward, with no host sync (osm_ps_blind_optimize,
    include/osmosis_blind.h: a projected gradient step on Q(w) = sum_b ||M (y_b - A(w) x0_b)||^2 / (2 * 3 h w) per inner iteration).
    By default the PSF is shared by the batch (`couples_batch`): photos through one optical system.  `per_image: True` learns one
    PSF per image of the batch (photos with unrelated shakes; the images stay independent, `couples_batch` is False and a chunked
    batch needs no grouped walk), `per_channel: True` one per colour plane (lateral chromatic aberration, wavelength-dependent
    scattering); the live weights are then `w` fp32 [nb,nc,T] with nb = batch_size or 1, nc = 3 or 1, every set starting from the
    init and stepped on its own simplex from its own images / planes (osm_ps_blind_optimize_s, include/osmosis_psfset.h).
    Config keys: kernel_size (odd, <= 61, default 31); init ('gaussian' with init_sigma default kernel_size / 6, 'delta', 'uniform',
    or a kernel: array / nested list / .npy path, non-negative, normalised to sum 1 in float64); eta (step size, 0.1), n_iter (inner
    iterations per guided sub-step, 1), l1 (sparsity shrinkage, 0.0); learn (True); per_image (False), per_channel (False).  The defaults are parameters, not tuned values.
    `learn: False` IS `psf_blur` with the init kernel (its non-zero taps, the three-launch data term, nothing stepped); the driver
    still treats it by its name: `simulate: True` needs `simulate_with`, so that switching `learn` does not change the measurement.
    An unknown config key raises ValueError.
    `taps(device)` returns (dy, dx, w_live); `forward` / `transpose` apply the current estimate; `kernel2d()` copies it from the
    device on demand only (one set; `kernels()` [nb,nc,k,k] for any number); `reset()` puts the initial weights of every set back
    (same tensors: recorded launches stay valid).  Not learning, the flags change nothing: every set would be the init."""

    couples_batch = True

    DRIVER_KEYS = ("simulate", "simulate_with")       # read by `sampling.restore_image`, not by the operator

    def __init__(self, device, kernel_size=31, init="gaussian", init_sigma=None, eta=0.1, n_iter=1, l1=0.0, learn=True, batch_size=1,
                 per_image=False, per_channel=False, **kwargs):
        unknown = sorted(set(kwargs) - set(self.DRIVER_KEYS))
        if unknown:                                   # (a mistyped `n_iters` would otherwise run with the default, silently)
            raise ValueError(f"blind_blur: unknown config key(s) {unknown} (known: kernel_size, init, init_sigma, eta, n_iter, l1, learn, "
                             f"per_image, per_channel, simulate, simulate_with)")
        super().__init__(device, batch_size, **kwargs)
        self._init = blind_init_kernel(kernel_size, init, init_sigma)
        self.kernel_size = int(kernel_size)
        self.eta, self.l1 = float(eta), float(l1)
        if not (np.isfinite(self.eta) and self.eta >= 0.0):
            raise ValueError(f"blind_blur: eta must be a finite number >= 0, got {eta!r}")
        if not (np.isfinite(self.l1) and self.l1 >= 0.0):
            raise ValueError(f"blind_blur: l1 must be a finite number >= 0, got {l1!r}")
        if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 1:
            raise ValueError(f"blind_blur: n_iter must be an integer >= 1, got {n_iter!r}")
        self.n_iter = int(n_iter)
        self.learn = bool(learn)
        for key, v in (("per_image", per_image), ("per_channel", per_channel)):
            if not isinstance(v, (bool, np.bool_)):
                raise ValueError(f"blind_blur: {key} must be True or False, got {v!r}")
        self.per_image, self.per_channel = bool(per_image), bool(per_channel)
        if self.learn:
            self._sets = (max(1, int(batch_size)) if self.per_image else 1, 3 if self.per_channel else 1)
        # a fixed kernel leaves the images of a batch independent, and so does one learnt kernel per image
        self.couples_batch = self.learn and not self.per_image

    def host_taps(self):
        if not self.learn:
            return super().host_taps()           # the init kernel's non-zeros: psf_blur
        if self._host is None:
            k = self.kernel_size
            iy, ix = np.divmod(np.arange(k * k), k)
            w = self._init.reshape(-1).astype(np.float32)
            if self.weight_sets != (1, 1):
                w = np.ascontiguousarray(np.broadcast_to(w, self.weight_sets + w.shape))
            self._host = ((iy - k // 2).astype(np.int32), (ix - k // 2).astype(np.int32), w)
        return self._host

    def radius(self):
        if not self.learn:
            return super().radius()
        return self.kernel_size // 2, self.kernel_size // 2

    def _to_device(self, a, device):
        # the live weights are a copy of their own: on the CPU `from_numpy` would alias the host's init, which `reset()` reads
        return super()._to_device(a.copy() if self.learn else a, device)

    def kernel2d(self):
        """The current estimate, float64 [k, k] (one device-to-host copy, made here and nowhere else); not learning: the init.
        The weights are read from where the data term stepped them: the tensors `taps(device)` made for the operator's own device
        ('cuda' and 'cuda:0' are different keys there: an index-less device finds them all the same), else the ones made last."""
        if not self.learn:
            return self._init.copy()
        return self._single(self.kernels()[0, 0])

    def kernels(self):
        """The current estimate of every set, float64 [nb,nc,k,k] (one device-to-host copy); not learning: the init [1,1,k,k]."""
        if not self.learn:
            return self._init[None, None].copy()
        t = self._dev.get(str(self.device))
        if t is None and self._dev:
            same = [v for v in self._dev.values() if v[2].device.type == self.device.type]
            t = (same or list(self._dev.values()))[-1]
        w = self.host_taps()[2] if t is None else t[2].detach().cpu().numpy()
        return w.astype(np.float64).reshape(self.weight_sets + self._init.shape)

    def reset(self):
        """Put the initial weights back on every device the operator lives on, in place."""
        if self.learn:
            for dev, (_, _, w) in self._dev.items():
                w.copy_(torch.from_numpy(self.host_taps()[2]))
        return self


def blind_field_init(kernel_size, grid, init="gaussian", init_sigma=None):
    """The starting point of a learnt field, float64 [gh,gw,k,k], every node non-negative and summing to 1: `init` is one of
    `blind_init_kernel`'s forms (the same kernel at every node), or a field of the user's -- a [gh,gw,kh,kw] array, nested list or
    the path of a .npy file holding one (every node as `blind_init_kernel` takes a kernel: centred in the k x k support)."""
    what = "blind_field_blur"
    k = _field_kernel_size(kernel_size, what)
    gh, gw = _field_grid(grid, what)
    if (isinstance(init, (str, bytes)) or hasattr(init, "__fspath__")) and str(os.fspath(init) if hasattr(init, "__fspath__") else init).endswith(".npy"):
        init = np.load(init, allow_pickle=False)
    if isinstance(init, torch.Tensor):
        init = init.detach().cpu().numpy()
    try:
        if not isinstance(init, (str, bytes)) and np.ndim(init) == 4:
            nodes = np.asarray(init, dtype=np.float64)
            if nodes.shape[:2] != (gh, gw):
                raise ValueError(f"{what}: the init field has {nodes.shape[0]} x {nodes.shape[1]} nodes, the grid is {gh} x {gw}")
            return np.stack([np.stack([blind_init_kernel(k, nodes[jy, jx]) for jx in range(gw)]) for jy in range(gh)])
        one = blind_init_kernel(k, init, init_sigma)
    except ValueError as e:
        raise ValueError(str(e).replace("blind_blur", what, 1)) from None
    return np.ascontiguousarray(np.broadcast_to(one, (gh, gw, k, k)))


@register_operator(name="blind_field_blur")
class BlindFieldOperator(PSFFieldOperator):
    """Blind spatially varying deblurring: `field_blur`'s operator -- a FIELD of point-spread functions on a gh x gw node grid,
    interpolated bilinearly over the frame -- whose node kernels are unknown and LEARNT during sampling.  Every node carries the dense
    support kernel_size x kernel_size (T = k^2 taps in row-major order, Ry = Rx = k // 2); the weights live in ONE device tensor `w`
    fp32 [gh,gw,T] that the step kernel overwrites between the network's forward and backward, with no host sync
    (osm_field_tap_grad / osm_field_tap_step, include/osmosis_blindfield.h: per inner
    iteration a projected gradient step of every node on Q(w) = sum_b ||M (y_b - A(w) x0_b)||^2 / (2 * 3 h w), each node on its own
    simplex, optionally tied to its 4-neighbours by `smooth`).  The field is shared by the batch (`couples_batch`) and by the planes.
    Config keys (an unknown one raises ValueError): kernel_size (odd, <= 61, default 31); grid ([gh, gw], default [3, 3], the
    field's limits); init (`blind_init_kernel`'s forms -- the same kernel at every node -- or a [gh,gw,kh,kw] array / .npy path)
    with init_sigma; eta (0.1), n_iter (1), l1 (0.0), smooth (0.0: >= 0, finite), learn (True).  The defaults are parameters, not
    tuned values.  `per_image` / `per_channel` are refused.  `learn: False` IS `field_blur` with the init field (its non-zero taps,
    the three-launch data term, nothing stepped); the driver still treats it by its name: `simulate: True` needs `simulate_with`.
    `taps(device)` returns (dy, dx, w_live); `forward` / `transpose` apply the current estimate; `kernels()` copies it from the device
    on demand, float64 [gh,gw,k,k]; `reset()` puts the initial field back in place (same tensor: recorded launches stay valid)."""

    couples_batch = True

    DRIVER_KEYS = ("simulate", "simulate_with")

    def __init__(self, device, kernel_size=31, grid=(3, 3), init="gaussian", init_sigma=None, eta=0.1, n_iter=1, l1=0.0, smooth=0.0,
                 learn=True, batch_size=1, **kwargs):
        what = "blind_field_blur"
        many = [k for k in ("per_image", "per_channel") if k in kwargs]
        if many:
            raise ValueError(f"{what}: {', '.join(many)} is not supported -- the learnt field is shared by the images of a batch and by "
                             f"the colour planes (a field per image or per channel is out of scope)")
        unknown = sorted(set(kwargs) - set(self.DRIVER_KEYS))
        if unknown:
            raise ValueError(f"{what}: unknown config key(s) {unknown} (known: kernel_size, grid, init, init_sigma, eta, n_iter, l1, "
                             f"smooth, learn, simulate, simulate_with)")
        PSFOperator.__init__(self, device, batch_size)
        self._field = self._init = np.ascontiguousarray(blind_field_init(kernel_size, grid, init, init_sigma))
        self.model, self.normalize = None, True
        self.kernel_size = int(kernel_size)
        self.eta, self.l1, self.smooth = float(eta), float(l1), float(smooth)
        for key, v, given in (("eta", self.eta, eta), ("l1", self.l1, l1), ("smooth", self.smooth, smooth)):
            if not (np.isfinite(v) and v >= 0.0):
                raise ValueError(f"{what}: {key} must be a finite number >= 0, got {given!r}")
        if isinstance(n_iter, bool) or int(n_iter) != n_iter or int(n_iter) < 1:
            raise ValueError(f"{what}: n_iter must be an integer >= 1, got {n_iter!r}")
        self.n_iter = int(n_iter)
        self.learn = bool(learn)
        self.couples_batch = self.learn       # a fixed field leaves the images of a batch independent

    def host_taps(self):
        if not self.learn:
            return super().host_taps()           # the init field's non-zeros: field_blur
        if self._host is None:
            k = self.kernel_size
            iy, ix = np.divmod(np.arange(k * k), k)
            w = np.ascontiguousarray(self._init.reshape(*self._init.shape[:2], k * k).astype(np.float32))
            self._host = ((iy - k // 2).astype(np.int32), (ix - k // 2).astype(np.int32), w)
        return self._host

    def radius(self):
        if not self.learn:
            return super().radius()
        return self.kernel_size // 2, self.kernel_size // 2

    def _to_device(self, a, device):
        # the live weights are a copy of their own: on the CPU `from_numpy` would alias the host's init, which `reset()` reads
        return super()._to_device(a.copy() if self.learn else a, device)

    def kernels(self):
        """The current estimate of every node, float64 [gh,gw,k,k] (one device-to-host copy); not learning: the init field."""
        if not self.learn:
            return self._init.copy()
        t = self._dev.get(str(self.device))
        if t is None and self._dev:
            same = [v for v in self._dev.values() if v[2].device.type == self.device.type]
            t = (same or list(self._dev.values()))[-1]
        w = self.host_taps()[2] if t is None else t[2].detach().cpu().numpy()
        return w.astype(np.float64).reshape(self._init.shape)

    def reset(self):
        """Put the initial field back on every device the operator lives on, in place."""
        if self.learn:
            for dev, (_, _, w) in self._dev.items():
                w.copy_(torch.from_numpy(self.host_taps()[2]))
        return self


class LearnableOperator(ABC):
    @abstractmethod
    def forward(self, data, **kwargs):
        pass


def _vec(s, n=3):
    a = np.array([float(p) for p in str(s).split(",")], dtype=np.float32)
    if a.size == 1 and n == 3:
        a = np.repeat(a, 3)
    if a.size != n:
        raise ValueError(f"expected {n} comma separated values, got {s!r}")
    return a


# optimizer name (utils.py:494-524) -> osm_phys_desc.optimizer
OPTIMIZER_CODES = {"": 0, "gd": 0, "sgd": 0, "adam": 1, "adamw": 2, "adamax": 3, "rmsprop": 4, "adagrad": 5, "adadelta": 6,
                   "asgd": 7, "rprop": 8}


# phi solvers that are not a torch.optim class of the reference's factory (its names stay in OPTIMIZER_CODES): the damped
# Gauss-Newton / Levenberg-Marquardt solver of include/osmosis_hip.h (osm_phys_desc.optimizer = 9), which steps phi from the normal
# equations the reduce kernel sums; `lm_lambda` is its initial damping.
PHI_SOLVER_CODES = {"lm": 9, "levenberg_marquardt": 9}
LM_LAMBDA_DEFAULT = 1.0


def optimizer_code(name):
    """osm_phys_desc.optimizer of an optimizer / solver name (`_check_optimizer` has vetted it)."""
    n = (name or "").lower()
    return PHI_SOLVER_CODES[n] if n in PHI_SOLVER_CODES else OPTIMIZER_CODES.get(n, 0)


def parse_lm_lambda(value):
    """`lm_lambda` of a physical operator: the initial damping of the `lm` solver, positive and finite (None: LM_LAMBDA_DEFAULT)."""
    if value is None:
        return LM_LAMBDA_DEFAULT
    try:
        lam = float(value)
    except (TypeError, ValueError):
        raise ValueError(f"lm_lambda must be a positive finite number, got {value!r}") from None
    if isinstance(value, bool) or not (lam > 0.0 and np.isfinite(lam)):
        raise ValueError(f"lm_lambda must be a positive finite number, got {value!r}")
    return lam


def _check_optimizer(name):
    n = (name or "").lower()
    if n in OPTIMIZER_CODES or n in PHI_SOLVER_CODES:
        return n
    if n in ("sparseadam", "lbfgs"):
        # the reference builds these, and its optimize() then raises: SparseAdam refuses dense gradients, LBFGS.step() needs a
        # closure (measurements.py:296-297 calls step() without one)
        raise NotImplementedError(f"optimizer '{name}' cannot step the phi parameters (in the reference either: SparseAdam needs "
                                  f"sparse gradients, LBFGS a closure)")
    raise ValueError(f"Optimizer '{name}' is not supported.")


def build_degradation(degradation, device, batch_size=1):
    """The linear operator between a physical image-formation model and the photo (`_PhysicalOperator(degradation=)`): None, an
    operator instance (handed through as it is), or a dict {name: <a registered blur / super-resolution / PSF operator>, ...its
    keys} built here.  NameError for a name nobody registered, ValueError for one that is no `GRID_OPERATORS` class and for
    'blind_blur' and 'field_blur' (by name: they are `PSFOperator`s, but a learnt PSF or a field of PSFs inside the water / haze model
    is out of scope)."""
    if degradation is None or not isinstance(degradation, dict):
        if isinstance(degradation, BlindFieldOperator):
            raise ValueError("degradation: 'blind_field_blur' (a learnt field of point-spread functions) inside a physical image-formation "
                             "model is not supported -- the composed data term takes one fixed point-spread function; give a 'psf_blur' kernel")
        if isinstance(degradation, PSFFieldOperator):
            raise ValueError("degradation: 'field_blur' (a field of point-spread functions) inside a physical image-formation model is not "
                             "supported -- the composed data term takes one point-spread function; give a fixed 'psf_blur' kernel")
        if getattr(degradation, "weight_sets", (1, 1)) != (1, 1):
            raise ValueError(f"degradation: the operator carries more than one point-spread function (per_image / per_channel: weight sets "
                             f"{degradation.weight_sets}), which a physical image-formation model does not take -- the composed route "
                             f"applies the operator to the depth-weight plane too, which has no channel; give one kernel")
        return degradation
    cfg = dict(degradation)
    name = cfg.pop("name", None)
    if name == "blind_blur":
        raise ValueError("degradation: 'blind_blur' (a learnt PSF) inside a physical image-formation model is not supported -- its "
                         "weights and the water / haze parameters would have to be stepped together; give a fixed 'psf_blur' kernel")
    if name == "blind_field_blur":
        raise ValueError("degradation: 'blind_field_blur' (a learnt field of point-spread functions) inside a physical image-formation "
                         "model is not supported -- the composed data term takes one fixed point-spread function; give a 'psf_blur' kernel")
    if name == "field_blur":
        raise ValueError("degradation: 'field_blur' (a field of point-spread functions) inside a physical image-formation model is not "
                         "supported -- the composed data term takes one point-spread function; give a fixed 'psf_blur' kernel")
    many = [k for k in ("per_image", "per_channel") if cfg.get(k)] + (["seed (a list)"] if isinstance(cfg.get("seed"), (list, tuple)) else [])
    if many:
        raise ValueError(f"degradation: {name!r} with {', '.join(many)} carries more than one point-spread function, which a physical "
                         f"image-formation model does not take -- the composed route applies the operator to the depth-weight plane "
                         f"too, which has no channel; give one kernel")
    cls = __OPERATOR__.get(name)
    grid = sorted(n for n, c in __OPERATOR__.items() if issubclass(c, GRID_OPERATORS))
    if cls is None:
        raise NameError(f"degradation: name {name!r} is not defined (the grid operators: {grid})")
    if not issubclass(cls, GRID_OPERATORS):
        raise ValueError(f"degradation: {name!r} is not a linear operator with a grid of its own (one of {grid})")
    cfg.pop("batch_size", None)
    return get_operator(name, device=device, batch_size=batch_size, **cfg)


def parse_phi_groups(phi_groups, batch_size):
    """`phi_groups` of a physical operator -> the tuple of group sizes, or None (every image its own phi): None; "all" / True, one
    group of `batch_size`; a list of positive ints summing to `batch_size`.  Anything else raises ValueError."""
    if phi_groups is None or phi_groups is False:
        return None
    if phi_groups is True or (isinstance(phi_groups, str) and phi_groups == "all"):
        return (int(batch_size),)
    if isinstance(phi_groups, (list, tuple)) and len(phi_groups) > 0 and \
            all(isinstance(n, (int, np.integer)) and not isinstance(n, bool) and n >= 1 for n in phi_groups):
        sizes = tuple(int(n) for n in phi_groups)
        if sum(sizes) != int(batch_size):
            raise ValueError(f"phi_groups {list(sizes)} sums to {sum(sizes)}, the operator has batch_size = {batch_size}")
        return sizes
    raise ValueError(f"phi_groups must be None, 'all' / True or a list of positive ints summing to batch_size, got {phi_groups!r}")


class _PhysicalOperator(LearnableOperator):
    """Shared machinery of the three image-formation models
    I = 0.5(rgb+1) exp(-phi_a d) + phi_inf (1 - exp(-phi_b d)),  d = convert_depth(x[:,3]).
    `degradation=` (a `GRID_OPERATORS` instance or its config dict, `build_degradation`; default None) puts a linear operator A
    between the model and the photo: the photo in [0, 1] is A I on A's grid `out_shape(H, W)`.  `forward` stays the water / haze
    image on the image grid; `observe` is A of it.
    `phi_groups=` (`parse_phi_groups`; default None) partitions the batch into contiguous groups of photos of ONE water body: a
    group's rows of `phi` (and of the optimizer state) are equal and stay equal, stepped once with the members' pooled gradient,
    `phi_reduce=` "mean" (default: the eta of the configs were chosen for one image's gradient) or "sum".  Attributes
    `group_sizes` (None: ungrouped), `group_offsets`, `phi_reduce`.
    `optimizer=` one of the reference's names (`OPTIMIZER_CODES`) or a solver of `PHI_SOLVER_CODES`: "lm" steps phi by damped
    Gauss-Newton from normal equations the kernels sum, `lm_lambda=` its initial damping (`parse_lm_lambda`); its etas only say which
    parameters are learnt, and it takes neither `phi_groups` nor a `degradation`."""
    KIND = -1
    VARS = ()

    def __init__(self, device, batch_size=1, **kwargs):
        self.device = torch.device(device) if not isinstance(device, torch.device) else device
        self.batch_size = batch_size
        self.depth_type = kwargs.get("depth_type", None)
        self.value = utilso.get_depth_value(kwargs.get("value", None)) if kwargs.get("value", None) is not None else None
        self.depth_code, self.depth_vals = utilso.depth_code_and_values(self.depth_type, kwargs.get("value", None))
        self.optimizer = _check_optimizer(kwargs.get("optimizer", None))
        self._requires_grad = {v: False for v in self.VARS}
        self.degradation = build_degradation(kwargs.get("degradation", None), self.device, batch_size)
        self.group_sizes = parse_phi_groups(kwargs.get("phi_groups", None), batch_size)
        self.phi_reduce = kwargs.get("phi_reduce", None) or "mean"
        if self.phi_reduce not in ("mean", "sum"):
            raise ValueError(f"phi_reduce must be 'mean' or 'sum', got {self.phi_reduce!r}")
        self.group_offsets = None if self.group_sizes is None else tuple(int(v) for v in np.cumsum((0,) + self.group_sizes))
        self.lm_lambda = parse_lm_lambda(kwargs.get("lm_lambda", None))
        if self.optimizer in PHI_SOLVER_CODES:
            # the solver's normal equations are those of ONE image's plain residual (include/osmosis_hip.h, optimizer 9)
            if self.group_sizes is not None:
                raise NotImplementedError(f"optimizer '{self.optimizer}' (lm, the Levenberg-Marquardt phi solver) with phi_groups is not "
                                          f"built: a group's normal equations would pool its members' Gram sums")
            if self.degradation is not None:
                raise NotImplementedError(f"optimizer '{self.optimizer}' (lm, the Levenberg-Marquardt phi solver) with a degradation is not "
                                          f"built: the operator would have to be applied to the Jacobian planes")

    # -- state ------------------------------------------------------------------------------
    def _init_phi(self, a, b, inf):
        row = np.concatenate([a, b, inf]).astype(np.float32)
        self.phi = torch.from_numpy(np.tile(row, (self.batch_size, 1))).to(self.device).contiguous()
        # The reference's parameter tensors (`self.phi_a`, ... [B,3,1,1]; haze `phi_ab` [B,1,1,1]) as VIEWS of the [B][9] block the
        # kernels step: leaves of autograd for code written against the reference API (a third-party conditioning method that calls
        # `operator.forward` under autograd, `loss.backward(inputs=[x_prev] + operator.get_variable_list())`, `operator.optimize()`),
        # and always the current values whichever side moved them.
        self._leaves = {}
        for name, (lo, n) in self._slots().items():
            leaf = self.phi[:, lo:lo + n].unflatten(1, (n, 1, 1))
            self._leaves[name] = leaf
            setattr(self, name, leaf)
        self._torch_optimizer = None

    def _slots(self):
        """{variable name: (first column of self.phi, width)}."""
        raise NotImplementedError

    def eta3(self):
        raise NotImplementedError

    def fill_desc(self, d: PhysDesc):
        d.kind = self.KIND
        d.depth_type = self.depth_code
        for i in range(3):
            d.dval[i] = self.depth_vals[i]
            d.eta[i] = self.eta3()[i]

    def _slot(self, lo, n=3):
        return self.phi[:, lo:lo + n].detach().clone().reshape(self.batch_size, n, 1, 1)

    # -- reference API ----------------------------------------------------------------------
    def forward(self, data, **kwargs):
        """Image formation on torch tensors (measurements.py:138-151, :251-264, :363-376), differentiable w.r.t. `data` AND the
        parameter tensors (`get_variable_list()`), as in the reference.  The sampler's own hot path evaluates the model inside the
        osm_phys_* kernels; this is the API for visualisation and for conditioning methods written against the reference."""
        rgb01 = 0.5 * (data[:, 0:-1] + 1)
        d = utilso.convert_depth(depth=data[:, -1:], depth_type=self.depth_type, value=self.value)
        lv = {k: (v if v.device == data.device else v.to(data.device)) for k, v in self._leaves.items()}
        pa = lv["phi_a"] if "phi_a" in lv else lv["phi_ab"]
        pb = lv["phi_b"] if "phi_b" in lv else pa
        return rgb01 * torch.exp(-pa * d) + lv["phi_inf"] * (1 - torch.exp(-pb * d))

    def observe(self, data, **kwargs):
        """What the camera records, in [0, 1]: `degradation.forward(forward(data))` on the degradation's grid (differentiable
        through `osmosis::linop_apply` / `osmosis::psf_apply`); without a degradation, `forward(data)`."""
        image = self.forward(data, **kwargs)
        return image if self.degradation is None else self.degradation.forward(image.contiguous())

    def out_shape(self, H, W):
        """(h, w) of the measurement of an H x W image."""
        return (int(H), int(W)) if self.degradation is None else tuple(self.degradation.out_shape(int(H), int(W)))

    def optimize(self, **kwargs):
        """measurements.py:266-303.  The package's conditioning method steps phi on the device (osm_phys_finalize) and calls this
        for the variables dictionary only.  A caller that back-propagated into the parameter tensors itself (their `.grad` is set)
        gets the reference's step here: plain gradient descent phi -= eta * grad for 'GD' / 'sgd' / '', else the torch optimizer of
        `optimizer:` over one parameter group per variable (lr = eta), then the gradients are zeroed."""
        if not kwargs.get("freeze_phi", False) and any(v.grad is not None for v in self._leaves.values()):
            if self.optimizer in PHI_SOLVER_CODES:
                raise NotImplementedError(f"optimizer '{self.optimizer}' (lm, the Levenberg-Marquardt phi solver) cannot step from the "
                                          f"parameters' .grad (operator.optimize() on the autograd route of a foreign degradation or "
                                          f"loss): a gradient is not a Jacobian; the solver runs inside the osm_phys_* kernels only")
            if self.group_sizes is not None:
                # shared water parameters: the rows of a group are one parameter, so its gradient is the members' pooled one (sum or
                # mean), handed to every row -- the same optimizer code below then keeps the rows equal
                with torch.no_grad():
                    for v in self._leaves.values():
                        if v.grad is not None:
                            for lo, hi in zip(self.group_offsets[:-1], self.group_offsets[1:]):
                                pooled = v.grad[lo:hi].sum(dim=0, keepdim=True)
                                v.grad[lo:hi] = pooled / (hi - lo) if self.phi_reduce == "mean" else pooled
            etas = dict(zip(("phi_a", "phi_b", "phi_inf"), self.eta3()))
            etas["phi_ab"] = etas["phi_a"]
            if OPTIMIZER_CODES[self.optimizer] == 0:
                with torch.no_grad():
                    for name, v in self._leaves.items():
                        if v.requires_grad and v.grad is not None:
                            v.add_(v.grad, alpha=-etas[name])
            else:
                if self._torch_optimizer is None:
                    self._torch_optimizer = utilso.get_optimizer(self.optimizer, [{"params": v, "lr": etas[n]} for n, v in self._leaves.items()])
                self._torch_optimizer.step()
            for v in self._leaves.values():
                if v.grad is not None:
                    v.grad.zero_()
        return self.variables()

    def set_variable_gradients(self, value=None, **kwargs):
        if value is None:
            raise ValueError("A value should be specified (True or False for general or dictionary)")
        for v in self.VARS:
            self._requires_grad[v] = bool(value[v] if isinstance(value, dict) else value)
            self._leaves[v].requires_grad_(self._requires_grad[v])

    def get_variable_gradients(self, **kwargs):
        return {v: self._leaves[v].requires_grad for v in self.VARS}

    def get_variable_list(self, **kwargs):
        return [self._leaves[v] for v in self.VARS]


@register_operator(name="underwater_physical_revised")
class UnderWaterPhysicalRevisedOperator(_PhysicalOperator):
    KIND = 0
    VARS = ("phi_a", "phi_b", "phi_inf")

    def __init__(self, device, phi_a, phi_b, phi_inf, phi_a_eta=1e-5, phi_b_eta=1e-5, phi_inf_eta=1e-5,
                 phi_a_learn_flag=True, phi_b_learn_flag=True, phi_inf_learn_flag=True, batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        self._init_phi(_vec(phi_a), _vec(phi_b), _vec(phi_inf))
        self.phi_a_eta = float(phi_a_eta) if phi_a_learn_flag else 0.0
        self.phi_b_eta = float(phi_b_eta) if phi_b_learn_flag else 0.0
        self.phi_inf_eta = float(phi_inf_eta) if phi_inf_learn_flag else 0.0

    def eta3(self):
        return (self.phi_a_eta, self.phi_b_eta, self.phi_inf_eta)

    def _slots(self):
        return {"phi_a": (0, 3), "phi_b": (3, 3), "phi_inf": (6, 3)}

    def variables(self):
        return {"phi_a": self._slot(0), "phi_b": self._slot(3), "phi_inf": self._slot(6)}


class _ABOperator(_PhysicalOperator):
    VARS = ("phi_ab", "phi_inf")

    def eta3(self):
        return (self.phi_ab_eta, 0.0, self.phi_inf_eta)


@register_operator(name="underwater_physical")
class UnderWaterPhysicalOperator(_ABOperator):
    KIND = 1

    def __init__(self, device, phi_ab, phi_inf, phi_ab_eta=1e-5, phi_inf_eta=1e-5, phi_ab_learn_flag=True,
                 phi_inf_learn_flag=True, batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        ab = _vec(phi_ab)
        self._init_phi(ab, ab, _vec(phi_inf))
        self.phi_ab_eta = float(phi_ab_eta) if phi_ab_learn_flag else 0.0
        self.phi_inf_eta = float(phi_inf_eta) if phi_inf_learn_flag else 0.0

    def _slots(self):
        return {"phi_ab": (0, 3), "phi_inf": (6, 3)}

    def variables(self):
        return {"phi_ab": self._slot(0), "phi_inf": self._slot(6)}


@register_operator(name="haze_physical")
class HazePhysicalOperator(_ABOperator):
    KIND = 2

    def __init__(self, device, phi_ab, phi_inf, phi_ab_eta=1e-5, phi_inf_eta=1e-5, phi_ab_learn_flag=True,
                 phi_inf_learn_flag=True, batch_size=1, **kwargs):
        super().__init__(device, batch_size, **kwargs)
        ab = np.repeat(np.float32(float(phi_ab)), 3)
        self._init_phi(ab, ab, _vec(phi_inf))
        self.phi_ab_eta = float(phi_ab_eta) if phi_ab_learn_flag else 0.0
        self.phi_inf_eta = float(phi_inf_eta) if phi_inf_learn_flag else 0.0

    def _slots(self):
        return {"phi_ab": (0, 1), "phi_inf": (6, 3)}

    def variables(self):
        return {"phi_ab": self._slot(0, 1), "phi_inf": self._slot(6)}


# ----------------------------------------------------------------------------- noisers
__NOISE__ = {}


def register_noise(name: str):
    def wrapper(cls):
        if __NOISE__.get(name, None):
            raise NameError(f"Name {name} is already defined!")
        __NOISE__[name] = cls
        return cls
    return wrapper


def get_noise(name: str, **kwargs):
    if __NOISE__.get(name, None) is None:
        raise NameError(f"Name {name} is not defined.")
    noiser = __NOISE__[name](**kwargs)
    noiser.__name__ = name
    return noiser


class Noise(ABC):
    def __call__(self, data):
        return self.forward(data)

    @abstractmethod
    def forward(self, data):
        pass


@register_noise(name="clean")
class Clean(Noise):
    def forward(self, data):
        return data


@register_noise(name="gaussian")
class GaussianNoise(Noise):
    def __init__(self, sigma):
        self.sigma = sigma

    def forward(self, data):
        return data + torch.randn_like(data) * self.sigma


@register_noise(name="poisson")
class PoissonNoise(Noise):
    def __init__(self, rate):
        self.rate = rate

    def forward(self, data):
        dev = data.device
        d01 = ((data + 1.0) / 2.0).clamp(0, 1).detach().cpu()
        noisy = torch.from_numpy(np.random.poisson(d01 * 255.0 * self.rate) / 255.0 / self.rate)
        return (noisy * 2.0 - 1.0).clamp(-1, 1).to(dev)
