"""Input pipeline of the reference driver: `osmosis_utils/data.py:15-109`
(`ImagesFolder`, `ImagesFolder_GT`) and the transform chain of `osmosis_sampling.py:46-49`
    ToTensor -> Resize(256) -> CenterCrop([256, 256]) -> Normalize(0.5, 0.5)
without torchvision / cv2 / natsort (none of them is in this image): PIL + torch only.

Resize follows the pinned torchvision 0.14.1 behaviour for TENSOR inputs (the chain resizes after ToTensor):
bilinear, align_corners=False, NO antialiasing, smaller edge -> `size`, longer edge -> int(size * long / short).
torchvision is absent here, so the pin is one level down: tests/golden/resize_chain.npz holds the output of the
ATen call torchvision 0.14.x makes (`interpolate(..., "bilinear", align_corners=False, antialias=False)`,
oracle/tools/gen_resize_golden.py); this module and the numpy restatement oracle/data_ref.py are both tested against it.
Host-side code; the sampler takes the resulting [B,3,256,256] tensor in [-1, 1].
"""
import glob
import os
import re
from dataclasses import dataclass
from os.path import join as pjoin

import numpy as np
import torch
import torch.nn.functional as F
from PIL import Image
from torch.utils.data import Dataset


# ----------------------------------------------------------------------------- natural ordering (natsort.natsorted)
def _natural_key(s):
    return [(0, int(p), "") if p.isdigit() else (1, 0, p) for p in re.split(r"(\d+)", str(s)) if p != ""]


def natsorted(items):
    """Default natsort order: digit runs compare as unsigned integers, the rest as text ('img2' < 'img10')."""
    return sorted(items, key=_natural_key)


# ----------------------------------------------------------------------------- transforms
def to_tensor(pic):
    """transforms.ToTensor: PIL image / HxWxC uint8 array -> float32 CxHxW in [0, 1] (other dtypes: no scaling)."""
    arr = np.array(pic)          # a writable copy (PIL buffers are read-only)
    if arr.ndim == 2:
        arr = arr[:, :, None]
    t = torch.from_numpy(np.ascontiguousarray(arr)).permute(2, 0, 1)
    if t.dtype == torch.uint8:
        return t.to(torch.float32).div(255)
    return t.to(torch.float32) if t.dtype != torch.float32 else t


def resize(img, size):
    """transforms.Resize(size=int) on a tensor [..., H, W]: smaller edge -> size, bilinear, no antialias."""
    h, w = img.shape[-2:]
    if isinstance(size, int):
        short, long_ = (w, h) if w <= h else (h, w)
        new_short, new_long = size, int(size * long_ / short)
        nw, nh = (new_short, new_long) if w <= h else (new_long, new_short)
    else:
        nh, nw = size
    if (nh, nw) == (h, w):
        return img
    x = img if img.dim() == 4 else img.unsqueeze(0)
    y = F.interpolate(x.to(torch.float32), size=(nh, nw), mode="bilinear", align_corners=False, antialias=False)
    return y if img.dim() == 4 else y.squeeze(0)


def center_crop(img, output_size):
    """transforms.CenterCrop: zero-pads when the image is smaller, then crops at round((H - h) / 2)."""
    th, tw = (output_size, output_size) if isinstance(output_size, int) else output_size
    h, w = img.shape[-2:]
    if tw > w or th > h:
        pl = (tw - w) // 2 if tw > w else 0
        pt = (th - h) // 2 if th > h else 0
        pr = (tw - w + 1) // 2 if tw > w else 0
        pb = (th - h + 1) // 2 if th > h else 0
        img = F.pad(img, (pl, pr, pt, pb))
        h, w = img.shape[-2:]
        if (th, tw) == (h, w):
            return img
    top = int(round((h - th) / 2.0))
    left = int(round((w - tw) / 2.0))
    return img[..., top:top + th, left:left + tw]


def normalize(img, mean=(0.5, 0.5, 0.5), std=(0.5, 0.5, 0.5)):
    m = torch.as_tensor(mean, dtype=img.dtype).view(-1, 1, 1)
    s = torch.as_tensor(std, dtype=img.dtype).view(-1, 1, 1)
    return (img - m) / s


def default_transform(size=256):
    """osmosis_sampling.py:46-49."""
    def apply(pic):
        return normalize(center_crop(resize(to_tensor(pic), size), [size, size]))
    return apply


# ----------------------------------------------------------------------------- geometry of the transform chain
@dataclass(frozen=True)
class Geometry:
    """Where the network grid sits in the original photo (`transform_geometry`).

    An original pixel centre (i, j) has the network-grid coordinate v = (ay * i + by, ax * j + bx); the covered rectangle
    [y0, y0 + Hc) x [x0, x0 + Wc) holds exactly the original pixels whose v lies in [-0.5, h - 0.5) x [-0.5, w - 0.5)."""
    H0: int
    W0: int
    nh: int          # size after Resize
    nw: int
    top: int         # crop window in resized pixels
    left: int
    h: int           # network grid
    w: int
    ay: float
    by: float
    ax: float
    bx: float
    y0: int          # covered rectangle in original pixels
    x0: int
    Hc: int
    Wc: int

    def rect_map(self):
        """(ay, by, ax, bx) for indices counted from the covered rectangle's corner instead of the photo's."""
        return self.ay, self.ay * self.y0 + self.by, self.ax, self.ax * self.x0 + self.bx


def _covered(n0, n, lo, length):
    """Original indices i in [0, n0) with lo <= (i + 0.5) * n / n0 < lo + length, in integers: (first, count)."""
    first = max(0, -((n - 2 * lo * n0) // (2 * n)))                  # ceil((2 lo n0 - n) / (2 n))
    end = min(n0, -((n - 2 * (lo + length) * n0) // (2 * n)))
    return first, max(0, end - first)


def transform_geometry(H0, W0, size=256, crop="center", multiple=32):
    """The geometry of Resize(size) -> CenterCrop on an H0 x W0 photo, in the arithmetic of `resize` / `center_crop` (int()
    truncation of the long edge, round() of the crop offset).  crop="center": the [size, size] crop of `default_transform`;
    crop="fit": the whole resized image, each side center-cropped down to the largest multiple of `multiple` (what the engine
    accepts).  Raises ValueError when the network grid would be finer than the photo: the full-resolution path only upsamples."""
    H0, W0, size = int(H0), int(W0), int(size)
    short, long_ = (W0, H0) if W0 <= H0 else (H0, W0)
    new_long = int(size * long_ / short)
    nw, nh = (size, new_long) if W0 <= H0 else (new_long, size)
    if nh > H0 or nw > W0:
        raise ValueError(f"a {H0} x {W0} image is coarser than its {nh} x {nw} network grid: nothing to upsample")
    if crop == "center":
        h = w = size
    elif crop == "fit":
        h, w = nh // multiple * multiple, nw // multiple * multiple
    else:
        raise ValueError(f"crop must be 'center' or 'fit', got {crop!r}")
    if h < 1 or w < 1 or h > nh or w > nw:
        raise ValueError(f"a {h} x {w} crop does not fit the {nh} x {nw} resized image")
    top, left = int(round((nh - h) / 2.0)), int(round((nw - w) / 2.0))
    ay, ax = nh / H0, nw / W0
    y0, Hc = _covered(H0, nh, top, h)
    x0, Wc = _covered(W0, nw, left, w)
    return Geometry(H0, W0, nh, nw, top, left, h, w, ay, 0.5 * ay - 0.5 - top, ax, 0.5 * ax - 0.5 - left, y0, x0, Hc, Wc)


def fit_transform(size=256, multiple=32):
    """ToTensor -> Resize(size) -> center crop to multiples of `multiple` -> Normalize: the whole photo instead of its central
    square.  Returns a function pic -> (tensor [3,h,w] in [-1,1], Geometry)."""
    def apply(pic):
        t = to_tensor(pic)
        geo = transform_geometry(t.shape[-2], t.shape[-1], size, "fit", multiple)
        return normalize(center_crop(resize(t, size), [geo.h, geo.w])), geo
    return apply


def transform_mask(mask, size=256, crop="center", multiple=32, geometry=None):
    """A validity mask given at the photo's own resolution, taken through the geometry of the photo's transform: `resize`
    (bilinear, as the photo) and `center_crop`, clamped to [0, 1]; no Normalize.  crop="center": the [size, size] crop of
    `default_transform`; crop="fit" or a
    `geometry` (the `Geometry` that `fit_transform` returned for the photo): the grid of `fit_transform`.
    mask: [H0,W0], [1,H0,W0] or [3,H0,W0] (anything `torch.as_tensor` takes; bool / uint8 0-1 maps included).
    Returns fp32 [1,C,h,w] with C = 1 or 3: what `restore_image(mask=)` and `p_sample_loop(measurement_mask=)` accept."""
    m = torch.as_tensor(np.asarray(mask) if not torch.is_tensor(mask) else mask).to(torch.float32)
    if m.dim() == 2:
        m = m.unsqueeze(0)
    if m.dim() != 3 or m.shape[0] not in (1, 3):
        raise ValueError(f"mask must be [H0,W0], [1,H0,W0] or [3,H0,W0], got {tuple(m.shape)}")
    if geometry is not None:
        if (m.shape[-2], m.shape[-1]) != (geometry.H0, geometry.W0):
            raise ValueError(f"the mask is {m.shape[-2]} x {m.shape[-1]} but the geometry describes a {geometry.H0} x {geometry.W0} photo")
        out_hw = [geometry.h, geometry.w]
    elif crop == "center":
        out_hw = [size, size]
    else:
        geo = transform_geometry(m.shape[-2], m.shape[-1], size, crop, multiple)
        out_hw = [geo.h, geo.w]
    return center_crop(resize(m, size), out_hw).clamp(0.0, 1.0).unsqueeze(0).contiguous()


def transform_range(z, confidence=None, size=256, crop="center", multiple=32, geometry=None, min_cover=0.5):
    """A range map given at the photo's own resolution (structure from motion, stereo, an altimeter; any unit), taken through the
    geometry of the photo's transform, hole-aware: with v = [z finite and > 0],
        z_out = resize(z v) / resize(v) where resize(v) >= min_cover, else 0         (a hole does not bleed towards 0)
        m_out = resize(confidence v) [resize(v) >= min_cover]                        (confidence None: 1)
    `resize` (bilinear, as the photo) and `center_crop` as in `transform_mask`; crop / geometry select the grid the same way.
    z, confidence: [H0,W0] or [1,H0,W0].  Returns (z [1,1,h,w], m [1,1,h,w]) fp32: what `restore_image(depth=, depth_confidence=)`
    and `p_sample_loop(depth_prior=dict(z=, confidence=))` accept."""
    def plane(t, what):
        t = torch.as_tensor(np.asarray(t) if not torch.is_tensor(t) else t).to(torch.float32)
        if t.dim() == 2:
            t = t.unsqueeze(0)
        if t.dim() != 3 or t.shape[0] != 1:
            raise ValueError(f"{what} must be [H0,W0] or [1,H0,W0], got {tuple(t.shape)}")
        return t
    z = plane(z, "the range map")
    if not 0.0 < float(min_cover) <= 1.0:
        raise ValueError(f"min_cover must lie in (0, 1], got {min_cover}")
    v = (torch.isfinite(z) & (z > 0)).to(torch.float32)
    c = v if confidence is None else plane(confidence, "the confidence") * v
    if tuple(c.shape) != tuple(z.shape):
        raise ValueError(f"the confidence {tuple(c.shape)} must have the range map's shape {tuple(z.shape)}")
    if confidence is not None and (not bool(torch.isfinite(c).all()) or float(c.min()) < 0.0 or float(c.max()) > 1.0):
        raise ValueError("the confidence must be finite and lie within [0, 1]")
    if geometry is not None:
        if (z.shape[-2], z.shape[-1]) != (geometry.H0, geometry.W0):
            raise ValueError(f"the range map is {z.shape[-2]} x {z.shape[-1]} but the geometry describes a {geometry.H0} x {geometry.W0} photo")
        out_hw, size = [geometry.h, geometry.w], (geometry.nh, geometry.nw)      # the geometry's own resize, whatever `size` says
    elif crop == "center":
        out_hw = [size, size]
    else:
        geo = transform_geometry(z.shape[-2], z.shape[-1], size, crop, multiple)
        out_hw = [geo.h, geo.w]
    zv = torch.where(v > 0, z, torch.zeros_like(z))
    rz, rv, rc = (center_crop(resize(t, size), out_hw) for t in (zv, v, c))
    keep = rv >= float(min_cover)
    z_out = torch.where(keep, rz / rv.clamp_min(1e-12), torch.zeros_like(rz))
    m_out = torch.where(keep, rc, torch.zeros_like(rc)).clamp(0.0, 1.0)
    return z_out.unsqueeze(0).contiguous(), m_out.unsqueeze(0).contiguous()


# ----------------------------------------------------------------------------- datasets
class ImagesFolder(Dataset):
    """data.py:15-38: every file of `root_dir` in natural order -> (transformed image, file name)."""

    def __init__(self, root_dir, transform=None):
        self.root_dir = root_dir
        self.images_list = natsorted(os.listdir(root_dir))
        self.transform = transform

    def __len__(self):
        return len(self.images_list)

    def __getitem__(self, idx):
        image = Image.open(os.path.join(self.root_dir, self.images_list[idx]))
        if self.transform is not None:
            image = self.transform(image)
        return image, self.images_list[idx]


class ImagesFolder_GT(Dataset):
    """data.py:73-109 (simulation config): ([image, gt_rgb, gt_depth as 3 equal channels], image file name).
    16-bit depth maps are reduced to 8 bits by an integer division by 256, like the reference."""

    def __init__(self, root_dir, gt_rgb_dir, gt_depth_dir, transform=None):
        self.gt_rgb_dir, self.gt_depth_dir, self.root_dir = gt_rgb_dir, gt_depth_dir, root_dir
        self.gt_rgb_list = natsorted(glob.glob(pjoin(gt_rgb_dir, "*.*")))
        self.gt_depth_list = natsorted(glob.glob(pjoin(gt_depth_dir, "*.*")))
        self.images_list = natsorted(glob.glob(pjoin(root_dir, "*.*")))
        self.transform = transform

    def __len__(self):
        return len(self.gt_rgb_list)

    def __getitem__(self, idx):
        image_name = os.path.basename(self.images_list[idx])
        image = Image.open(self.images_list[idx])
        gt_rgb = Image.open(self.gt_rgb_list[idx])
        depth = np.asarray(Image.open(self.gt_depth_list[idx]))
        if depth.dtype == np.uint16 or depth.dtype == np.int32:      # PIL opens 16-bit PNGs as I;16 / I
            depth = (depth // 256).astype(np.uint8)
        gt_depth = Image.fromarray(depth)
        if self.transform is not None:
            image = self.transform(image)
            gt_rgb = self.transform(gt_rgb)
            gt_depth = self.transform(gt_depth.convert(mode="RGB"))
        return [image, gt_rgb, gt_depth], image_name
