"""Per-pixel validity masks in the guidance data term, the parts that need no GPU: validation and broadcast of
`set_measurement_mask`, the geometry helper `data.transform_mask`, the autograd paths (`_loss_autograd`, `ps`'s `grad_and_value`)
against float64 restatements, the config key, and the kernel path's refusal of CPU tensors."""
import numpy as np
import pytest
import torch

from osmosis_diffusion_code_amd import sampling
from osmosis_diffusion_code_amd._lib import OsmosisHipError
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
from osmosis_diffusion_code_amd.osmosis_utils import data

OKW = dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8", phi_inf="0.14, 0.29, 0.49")


def osmosis_cond(B=1, **kw):
    op = M.get_operator("underwater_physical_revised", device="cpu", batch_size=B, **OKW)
    args = dict(loss_function="norm", loss_weight="depth", weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9",
                gradient_x_prev=True, gradient_clip="False,0", n_iter=1, pattern="pcgs")
    args.update(kw)
    return CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), **args)


def ps_cond(B=1):
    return CM.get_conditioning_method("ps", M.get_operator("noise", device="cpu", batch_size=B), M.get_noise("gaussian", sigma=0.0),
                                      scale="0.3")


# ------------------------------------------------------------------------------------------------------------ validation, broadcast
@pytest.mark.parametrize("make", [osmosis_cond, ps_cond])
def test_mask_validation(make):
    cond = make(2)
    ok = torch.rand(2, 3, 6, 8)
    with pytest.raises(ValueError, match="rank 4"):
        cond.set_measurement_mask(ok[0])
    with pytest.raises(ValueError, match="rank 4"):
        cond.set_measurement_mask(ok[None])
    with pytest.raises(ValueError, match="1 or 3 channels"):
        cond.set_measurement_mask(torch.rand(2, 2, 6, 8))
    with pytest.raises(ValueError, match="1 or 3 channels"):
        cond.set_measurement_mask(torch.rand(2, 4, 6, 8))
    with pytest.raises(ValueError, match=r"within \[0, 1\]"):
        cond.set_measurement_mask(ok + 0.5)
    with pytest.raises(ValueError, match=r"within \[0, 1\]"):
        cond.set_measurement_mask(ok - 0.5)
    bad = ok.clone()
    bad[1, 2, 3, 4] = float("nan")
    with pytest.raises(ValueError, match="finite"):
        cond.set_measurement_mask(bad)
    bad[1, 2, 3, 4] = float("inf")
    with pytest.raises(ValueError, match="finite"):
        cond.set_measurement_mask(bad)
    with pytest.raises(ValueError, match="batch 3"):
        cond.set_measurement_mask(torch.rand(3, 3, 6, 8), batch=2)
    assert cond._mask is None                                  # nothing was stored by a refused call
    cond.set_measurement_mask(ok)
    assert cond._mask is not None
    cond.set_measurement_mask(None)
    assert cond._mask is None and cond.measurement_mask(2, 48, "cpu") is None


@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 1, 5, 7), (1, 3, 5, 7), (1, 1, 5, 7)])
@pytest.mark.parametrize("make", [osmosis_cond, ps_cond])
def test_every_accepted_shape_reaches_b3hw(make, shape):
    cond = make(2)
    m = torch.rand(*shape, generator=torch.Generator().manual_seed(3))
    rows = cond.set_measurement_mask(m, batch=2)
    assert rows.shape == (2, 3, 35) and rows.is_contiguous() and rows.dtype == torch.float32
    assert torch.equal(rows.view(2, 3, 5, 7), m.expand(2, 3, 5, 7))
    # without the batch, a batch-1 mask is expanded when the measurement's batch is known
    cond.set_measurement_mask(m)
    got = cond.measurement_mask(2, 35, "cpu")
    assert got.shape == (2, 3, 35) and got.is_contiguous() and torch.equal(got.view(2, 3, 5, 7), m.expand(2, 3, 5, 7))
    with pytest.raises(ValueError, match="does not fit"):
        cond.measurement_mask(2, 36, "cpu")


def test_p_sample_loop_checks_the_mask_against_x_start():
    sampler = gd.get_sampler("ddpm")(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                     model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False,
                                     clip_denoised=False, rescale_timesteps=False)
    cond = osmosis_cond(2)
    kw = dict(model=None, x_start=torch.zeros(2, 4, 8, 8), measurement=torch.zeros(2, 3, 8, 8), measurement_cond_fn=cond.conditioning,
              record=False, save_root=None, pretrain_model="osmosis")
    with pytest.raises(ValueError, match="batch 3"):
        sampler.p_sample_loop(measurement_mask=torch.ones(3, 1, 8, 8), **kw)
    with pytest.raises(ValueError, match="image grid"):
        sampler.p_sample_loop(measurement_mask=torch.ones(2, 1, 8, 6), **kw)
    with pytest.raises(ValueError, match=r"within \[0, 1\]"):
        sampler.p_sample_loop(measurement_mask=2 * torch.ones(2, 1, 8, 8), **kw)
    with pytest.raises(TypeError, match="set_measurement_mask"):
        sampler.p_sample_loop(measurement_mask=torch.ones(2, 1, 8, 8), **dict(kw, measurement_cond_fn=lambda **k: None))


# ------------------------------------------------------------------------------------------------------------ geometry helper
def _rect_lands(mask_t, photo_t, tol):
    """The transformed indicator against the transformed photo: the photo is 1 inside the rectangle in channel 0, so the two
    transforms of the same geometry must give the same map (the photo goes through Normalize: undo it)."""
    assert mask_t.shape[0] == 1 and mask_t.shape[2:] == photo_t.shape[1:]
    assert float(mask_t.min()) >= 0.0 and float(mask_t.max()) <= 1.0
    assert float((mask_t[0, 0] - 0.5 * (photo_t[0] + 1)).abs().max()) <= tol
    assert float(mask_t.max()) == 1.0 and float(mask_t.min()) == 0.0      # the rectangle is inside the crop, and so is its outside


def test_mask_geometry_follows_the_photo():
    H0, W0 = 653, 900
    ind = np.zeros((H0, W0), dtype=np.float32)
    ind[200:420, 310:600] = 1.0
    photo = (np.repeat(ind[:, :, None], 3, axis=2) * 255).astype(np.uint8)
    # default_transform: Resize(256) + CenterCrop(256)
    m = data.transform_mask(ind, size=256)
    assert m.shape == (1, 1, 256, 256) and m.dtype == torch.float32
    _rect_lands(m, data.default_transform(256)(photo), 1e-6)
    # where the rectangle lands, from the geometry itself: original pixel centre (i, j) -> network coordinate
    geo = data.transform_geometry(H0, W0, 256, "center")
    r0, r1 = geo.ay * 200 + geo.by, geo.ay * 419 + geo.by
    c0, c1 = geo.ax * 310 + geo.bx, geo.ax * 599 + geo.bx
    inside = m[0, 0, int(np.ceil(r0)) + 1:int(np.floor(r1)), int(np.ceil(c0)) + 1:int(np.floor(c1))]
    assert inside.numel() > 0 and float(inside.min()) == 1.0
    assert float(m[0, 0, :int(np.floor(r0)) - 1].max()) == 0.0 and float(m[0, 0, :, int(np.ceil(c1)) + 2:].max()) == 0.0
    # fit_transform / Geometry
    pt, geo_f = data.fit_transform(256, 32)(photo)
    for mf in (data.transform_mask(ind, size=256, geometry=geo_f), data.transform_mask(ind, size=256, crop="fit", multiple=32)):
        assert mf.shape == (1, 1, geo_f.h, geo_f.w)
        _rect_lands(mf, pt, 1e-6)
    # three channels, bool input, wrong sizes
    m3 = data.transform_mask(torch.from_numpy(ind > 0).expand(3, H0, W0), size=256)
    assert m3.shape == (1, 3, 256, 256) and torch.equal(m3[:, 0:1], m)
    with pytest.raises(ValueError, match="geometry describes"):
        data.transform_mask(ind[:-1], geometry=geo_f)
    with pytest.raises(ValueError, match="mask must be"):
        data.transform_mask(np.zeros((2, H0, W0), dtype=np.float32))


# ------------------------------------------------------------------------------------------------------------ autograd paths
def _inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g)).clamp(-1, 1)
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    mask = torch.rand(B, 3, H, W, generator=g)
    mask[:, :, :2] = 0.0
    return x0, y, mask


def _f64_osmosis(x0, y, mask, loss_function, weighted):
    """The masked data term restated in float64: diff_c = (y_c - (2 I_c - 1)) w M_c, norm = sqrt(sum diff^2) per image,
    mse = sum diff^2 / (3 HW); returns (per-image loss, d sum(loss) / d x0)."""
    x = x0.double().requires_grad_(True)
    pa = torch.tensor([1.1, 0.95, 0.95], dtype=torch.float64).view(1, 3, 1, 1)
    pb = torch.tensor([0.95, 0.8, 0.8], dtype=torch.float64).view(1, 3, 1, 1)
    pinf = torch.tensor([0.14, 0.29, 0.49], dtype=torch.float64).view(1, 3, 1, 1)
    d = ((x[:, 3:4] + 1.4) * 1.4) ** 1.0
    I = 0.5 * (x[:, 0:3] + 1) * torch.exp(-pa * d) + pinf * (1 - torch.exp(-pb * d))
    w = ((x[:, 3:4].detach() + 1.4) * 1.4) if weighted else 1.0
    diff = (y.double() - (2 * I - 1)) * w * mask.double()
    ss = (diff ** 2).sum(dim=(1, 2, 3))
    loss = ss.sqrt() if loss_function == "norm" else ss / (3 * x0.shape[2] * x0.shape[3])
    (g,) = torch.autograd.grad(loss.sum(), x)
    return loss.detach(), g


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("loss_function", ["norm", "mse"])
def test_loss_autograd_with_a_mask_equals_the_float64_restatement(loss_function, weighted):
    B = 1 if loss_function == "norm" else 2       # (the reference's norm is joint over the batch: compared at B = 1)
    x0, y, mask = _inputs(B, 9, 7, 5)
    cond = osmosis_cond(B, loss_function=loss_function, loss_weight="depth" if weighted else "none")
    want_l, want_g = _f64_osmosis(x0, y, mask, loss_function, weighted)
    x = x0.clone().requires_grad_(True)
    cond.set_measurement_mask(mask)
    sep, loss, _ = cond._loss_autograd(x, y)
    (g,) = torch.autograd.grad(loss, x)
    assert np.allclose(sep, want_l.numpy(), rtol=2e-6)
    assert float((g.double() - want_g).abs().max()) < 2e-6 * float(want_g.abs().max())
    # a [B,1,H,W] mask is the same mask on every channel; ones are the unmasked loss exactly; None clears
    cond.set_measurement_mask(mask[:, 1:2])
    sep1, _, _ = cond._loss_autograd(x0, y)
    assert np.allclose(sep1, _f64_osmosis(x0, y, mask[:, 1:2].expand_as(mask), loss_function, weighted)[0].numpy(), rtol=2e-6)
    cond.set_measurement_mask(torch.ones(1, 1, 9, 7))
    ones = cond._loss_autograd(x0, y)[0]
    cond.set_measurement_mask(None)
    assert np.array_equal(ones, cond._loss_autograd(x0, y)[0])
    assert not np.allclose(sep, ones, rtol=1e-3)


def test_ps_grad_and_value_with_a_mask_equals_the_float64_restatement():
    x0, y, mask = _inputs(1, 9, 7, 6)
    cond = ps_cond()
    cond.set_measurement_mask(mask)
    xp = x0.clone().requires_grad_(True)
    g, loss = cond.grad_and_value(x_prev=xp, x_0_hat=1.0 * xp, measurement=y)
    r = (y.double() - x0[:, 0:3].double())
    L = ((mask.double() * r) ** 2).sum().sqrt()
    want = torch.zeros_like(x0, dtype=torch.float64)
    want[:, 0:3] = -(mask.double() ** 2) * r / L
    assert abs(float(loss.detach()) - float(L)) < 2e-6 * float(L)
    assert float((g.double() - want).abs().max()) < 2e-7 + 1e-5 * float(want.abs().max())
    assert float(g[:, :, :2].abs().max()) == 0.0 and float(g[:, 3].abs().max()) == 0.0
    # fully masked: loss 0, gradient 0 (torch.linalg.norm's backward at 0), finite
    cond.set_measurement_mask(torch.zeros(1, 1, 9, 7))
    xp = x0.clone().requires_grad_(True)
    g, loss = cond.grad_and_value(x_prev=xp, x_0_hat=1.0 * xp, measurement=y)
    assert float(loss) == 0.0 and float(g.abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ config, CPU tensors
class _Sampler:
    def __init__(self, seen):
        self.seen = seen

    def p_sample_loop(self, **kw):
        self.seen.append(kw)
        return torch.zeros_like(kw["x_start"])


def _cfg(mask_cfg=None):
    measurement = {"operator": {"name": "noise"}, "noise": {"name": "gaussian", "sigma": 0.0}}
    if mask_cfg is not None:
        measurement["mask"] = mask_cfg
    return {"measurement": measurement, "conditioning": {"method": "ps", "params": {"scale": 0.3}}, "diffusion": {},
            "sample_pattern": {"pattern": "original"}, "aux_loss": {}, "unet_model": {"pretrain_model": "osmosis"},
            "rgb_guidance": True}


def test_no_mask_key_means_no_mask_is_passed(monkeypatch):
    seen = []
    monkeypatch.setattr(sampling, "create_sampler", lambda **kw: _Sampler(seen))
    ref = torch.rand(1, 3, 8, 8) * 2 - 1
    res = sampling.restore_image(None, ref, _cfg(), device="cpu")
    assert len(seen) == 1 and "measurement_mask" not in seen[0] and "mask" not in res[-1]
    # an explicit mask reaches the loop as [B,3,H,W], and the result carries it
    m = torch.rand(1, 1, 8, 8)
    res = sampling.restore_image(None, ref, _cfg(), device="cpu", mask=m)
    assert torch.equal(seen[1]["measurement_mask"], m.expand(1, 3, 8, 8)) and torch.equal(res[-1]["mask"], m.expand(1, 3, 8, 8))
    with pytest.raises(ValueError, match="image grid"):
        sampling.restore_image(None, ref, _cfg(), device="cpu", mask=torch.rand(1, 1, 8, 6))
    with pytest.raises(ValueError, match="unknown key"):
        sampling.restore_image(None, ref, _cfg({"auto": {}}), device="cpu")
    # restore_images: a list aligned with the images
    out = sampling.restore_images(None, [ref, ref], _cfg(), device="cpu", masks=[m, None])
    assert torch.equal(out[0]["mask"], m.expand(1, 3, 8, 8)) and "mask" not in out[1]
    with pytest.raises(ValueError, match="align"):
        sampling.restore_images(None, [ref, ref], _cfg(), device="cpu", masks=[m])


def test_kernel_path_on_cpu_tensors_still_raises(monkeypatch):
    x0, y, mask = _inputs(1, 8, 8, 7)
    cond = osmosis_cond()
    cond.set_measurement_mask(mask)
    with pytest.raises(OsmosisHipError, match="no CPU fallback"):
        cond.loss_grad_x0(x0, y, freeze_phi=True)
    ps = ps_cond()
    ps.set_measurement_mask(mask)
    for x in (x0, x0[:, 0:3]):
        with pytest.raises(OsmosisHipError, match="no CPU fallback"):
            ps.loss_grad_x0(x.contiguous(), y)
    monkeypatch.setattr(sampling, "create_sampler", lambda **kw: _Sampler([]))
    with pytest.raises(OsmosisHipError, match="no CPU fallback"):      # the exposure mask is a kernel too
        sampling.restore_image(None, y, _cfg({"auto_exposure": {"low": 0.02, "high": 0.98}}), device="cpu")
