"""Per-pixel validity masks in the guidance data term on the HIP path.

Kernel level: the masked physics kernels (osm_phys_*_m) against a masked subclass of the oracle's guidance, `mask=None` / ones
against the plain entry points bit for bit, the fully masked image, the irrelevance of masked pixels, the masked `ps` data term
and osm_exposure_mask against float64 / numpy restatements, torch.library.opcheck.
Chain level (the tiny 4 -> 8 and 3 -> 6 networks, a 16 x 24 image, a 10-index respaced chain, injected noise, `_generic_loop`
patched to raise): the fused Osmosis chain against the masked oracle, batches and chunks, fused against `_generic_loop`, masked `ps`
(inpainting), and `restore_image` with the `auto_exposure` config."""
import os

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
SHAPES = [(36, 34), (37, 29)]        # HW = 1224: two reduce workgroups, the second a ragged 200 pixels; HW = 1073: odd
OPS = {
    "underwater_physical_revised": dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8",
                                        phi_inf="0.14, 0.29, 0.49"),
    "underwater_physical": dict(depth_type="original", value="1.4,1.4,1", phi_ab="1.1,0.95,0.95", phi_inf="0.2,0.4,0.7"),
    "haze_physical": dict(depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_inf="0.14, 0.29, 0.49"),
}
AUX = {"avrg_loss": 0.5, "val_loss": 20}
OPTIMIZER_NAMES = ["sgd", "adam", "adamw", "adamax", "rmsprop", "adagrad", "adadelta", "asgd", "rprop"]     # codes 0 .. 8


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


class MaskedGuidance(D.OsmosisGuidance):
    """The oracle's guidance with the mask in the residual: diff = (y - (2 I - 1)) w M; the losses keep their normalisation."""
    mask = None

    def loss(self, x0, y):
        I = self.op.forward(x0)
        diff = (y - (2 * I - 1)) * self._weight(x0) * self.mask
        if self.loss_function == "norm":
            return torch.norm(diff.detach(), p=2, dim=[1, 2, 3]).numpy(), torch.linalg.norm(diff)
        mse = (diff ** 2).mean(dim=(1, 2, 3))
        return mse.detach().numpy(), mse.sum()


def make_masks(kind, B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    if kind == "uniform":                     # a confidence per channel
        return torch.rand(B, 3, H, W, generator=g)
    if kind == "binary":                      # about 30 % zeros
        return (torch.rand(B, 3, H, W, generator=g) > 0.3).float()
    return torch.rand(B, 1, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) > 0.3).float()      # [B,1,H,W]


def phys_inputs(B, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g)).clamp(-1.0, 1.0)      # depth >= -1: the gamma bases stay positive
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    return x0, y


def etas(okw, value):
    return {k + "_eta": value for k in ("phi_a", "phi_b", "phi_ab", "phi_inf") if k in okw}


def hip_cond(pkg, opname, B, optimizer="sgd", eta=1e-3, n_iter=5, aux=None, loss_function="norm", loss_weight="depth"):
    _, _, M, CM = pkg
    okw = OPS[opname]
    oper = M.get_operator(opname, device=DEV, batch_size=B, optimizer=optimizer, **okw, **etas(okw, eta))
    return CM.get_conditioning_method("osmosis", oper, M.get_noise("clean"), loss_function=loss_function, loss_weight=loss_weight,
                                      weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
                                      gradient_clip="False,0", n_iter=n_iter, aux_loss=aux, pattern="pcgs")


# ------------------------------------------------------------------------------------------------------------ 1: against the oracle
@pytest.mark.parametrize("loss_weight", ["none", "depth"])
@pytest.mark.parametrize("loss_function", ["norm", "mse"])
@pytest.mark.parametrize("opname", list(OPS))
def test_masked_loss_grad_x0_vs_the_masked_oracle(pkg, opname, loss_function, loss_weight):
    """B = 2 with a different mask per image, 5 inner iterations, {auxiliary losses on, off} x {sgd, adam} x {uniform per channel,
    binary with ~30 % zeros, [B,1,H,W]} on the two shapes: loss, phi after the inner iterations and dL/dx0 against autograd through
    the oracle with the mask in its residual (image by image: the oracle's norm is joint over a batch).  Bars: the ones
    tests/test_guidance_gpu.py holds the unmasked kernels to (the arithmetic gains one multiply)."""
    okw = OPS[opname]
    case = 0
    for aux in (None, AUX):
        for optimizer, eta in (("sgd", 1e-3), ("adam", 2e-3)):
            for kind in ("uniform", "binary", "b1hw"):
                H, W = SHAPES[case % 2]
                case += 1
                x0, y = phys_inputs(2, H, W, 100 + case)
                mask = make_masks(kind, 2, H, W, 200 + case)
                cond = hip_cond(pkg, opname, 2, optimizer, eta, 5, aux, loss_function, loss_weight)
                cond.set_measurement_mask(mask, batch=2, device=DEV)
                gx0, sep = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
                gx0, sep, got_phi = gx0.cpu(), sep.cpu().numpy(), {n: v.cpu() for n, v in cond.operator.variables().items()}
                tag = (opname, loss_function, loss_weight, aux is not None, optimizer, kind, (H, W))
                for b in range(2):
                    op = D.PhysOperator(opname, batch_size=1, optimizer=optimizer, **okw, **etas(okw, eta))
                    guide = MaskedGuidance(op, n_iter=5, scale="7,7,7,0.9", gradient_clip="False,0", aux=aux, loss_function=loss_function,
                                           loss_weight=loss_weight)
                    guide.mask = mask[b:b + 1].expand(1, 3, H, W)
                    xb = x0[b:b + 1].clone().requires_grad_(True)
                    op.set_requires_grad(True)
                    for it in range(5):
                        want_sep, loss = guide.loss(xb, y[b:b + 1])
                        a = D.aux_loss(xb, aux)
                        total = loss if a is None else loss + a
                        total.backward(inputs=([xb] if it == 4 else []) + list(op.phi.values()))
                        op.sgd_step()
                    e_loss = abs(float(sep[b]) - float(want_sep[0])) / float(want_sep[0])
                    e_phi = max(float((got_phi[n][b:b + 1] - op.phi[n].detach()).abs().max()) for n in op.names)
                    scale = float(xb.grad.abs().max())
                    e_g = float((gx0[b:b + 1] - xb.grad).abs().max())
                    print(f"MASKPHYS {tag} image {b}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of {scale:.2e}")
                    assert e_loss <= 3e-5, (tag, b, e_loss)
                    assert e_phi <= (5e-6 if optimizer == "adam" else 3e-6), (tag, b, e_phi)
                    assert e_g < 3e-5 * scale + 1e-9, (tag, b, e_g, scale)


# ------------------------------------------------------------------------------------------------------------ 2: no mask is today's code
@pytest.mark.parametrize("optimizer", OPTIMIZER_NAMES)
def test_no_mask_and_ones_are_the_plain_entry_points_bit_for_bit(pkg, optimizer):
    """20 inner iterations with every optimizer code: `mask=None` and M = 1 through osm_phys_optimize_m, and through the
    launch-by-launch osm_phys_reduce_m / _finalize_m / _grad_m, are torch.equal to osm_phys_optimize on loss, g and phi."""
    from osmosis_diffusion_code_amd import ops
    H, W = SHAPES[0]
    B, HW = 2, H * W
    x0, y = (t.to(DEV) for t in phys_inputs(B, H, W, 31))
    ones = torch.ones(B, 3, HW, device=DEV)
    aux = AUX if OPTIMIZER_NAMES.index(optimizer) % 2 == 0 else None
    eta = {"adadelta": 5e-2, "asgd": 2e-5}.get(optimizer, 1e-3)

    def run(mode):
        cond = hip_cond(pkg, "underwater_physical_revised", B, optimizer, eta, 20, aux)
        st = cond._prepare(B, HW, x0.device)
        d, part, red, loss, g, phi = st["desc"], st["part"], st["red"], st["loss"], st["g"], cond.operator.phi
        assert d.optimizer == OPTIMIZER_NAMES.index(optimizer)
        opt = cond._opt if d.optimizer != 0 else None
        mask = ones if mode.endswith("ones") else None
        if mode == "plain":
            ops.phys_optimize(d, x0, y, phi, part, red, loss, g, 20, False, opt_state=opt)
        elif mode.startswith("optimize"):
            ops.phys_optimize_m(d, x0, y, mask, phi, part, red, loss, g, 20, False, opt_state=opt)
        else:
            for it in range(20):
                ops.phys_reduce_m(d, x0, y, mask, phi, part)
                if it == 19:
                    ops.phys_finalize_m(d, part, red, phi, False, loss, masked=mask is not None)
                    ops.phys_grad_m(d, x0, y, mask, phi, red, g)
                    ops.phys_finalize_m(d, part, red, phi, True, None, opt_state=opt, masked=mask is not None)
                else:
                    ops.phys_finalize_m(d, part, red, phi, True, loss, opt_state=opt, masked=mask is not None)
        return loss.clone(), g.clone(), phi.clone()
    want = run("plain")
    assert all(bool(torch.isfinite(t).all()) for t in want) and not torch.equal(want[2][0], hip_cond(
        pkg, "underwater_physical_revised", B).operator.phi[0])                       # the optimizer stepped
    for mode in ("optimize_none", "optimize_ones", "steps_none", "steps_ones"):
        got = run(mode)
        for name, a, b in zip(("loss", "g", "phi"), got, want):
            assert torch.equal(a, b), (optimizer, mode, name, float((a - b).abs().max()))


def test_ps_no_mask_and_ones_are_the_plain_entry_points_bit_for_bit(pkg):
    from osmosis_diffusion_code_amd import ops
    _, _, M, CM = pkg
    H, W = SHAPES[0]
    for C in (3, 4):
        x0, y = phys_inputs(2, H, W, 33)
        x0, y = x0[:, :C].contiguous().to(DEV), y.to(DEV)
        outs = []
        for mask in ("none", None, torch.ones(2, 1, H, W)):
            cond = CM.get_conditioning_method("ps", M.get_operator("noise", device=DEV, batch_size=2), M.get_noise("gaussian", sigma=0.0),
                                              scale="0.3")
            if not isinstance(mask, str):
                cond.set_measurement_mask(mask, batch=2, device=DEV)
            g, loss = cond.loss_grad_x0(x0, y)
            outs.append((g.clone(), loss.clone()))
        part, loss, g = torch.empty(2 * ops.phys_nblk(H * W), device=DEV), torch.empty(2, device=DEV), torch.empty_like(x0)
        ops.ps_loss_grad_mc(x0, y, None, part, loss, g, 2, C, H * W)
        outs.append((g, loss))
        for g, loss in outs[1:]:
            assert torch.equal(g, outs[0][0]) and torch.equal(loss, outs[0][1]), C


# ------------------------------------------------------------------------------------------------------------ 3: fully masked image
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("aux", [None, AUX], ids=["noaux", "aux"])
def test_fully_masked_image(pkg, aux, optimizer):
    """Image 1 of a batch of 2 is masked out: its loss is 0, its phi bit-unchanged, its g exactly 0 without auxiliary losses (with
    them: what they alone give), everything finite; image 0 is bit-equal to its own B = 1 run."""
    H, W = SHAPES[0]
    x0, y = phys_inputs(2, H, W, 41)
    mask = make_masks("uniform", 2, H, W, 42)
    mask[1] = 0.0
    cond = hip_cond(pkg, "underwater_physical_revised", 2, optimizer, 1e-3, 5, aux)
    phi0 = cond.operator.phi.clone()
    cond.set_measurement_mask(mask, batch=2, device=DEV)
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
    phi = cond.operator.phi
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(phi).all())
    assert float(loss[1]) == 0.0 and torch.equal(phi[1], phi0[1]) and not torch.equal(phi[0], phi0[0])
    if cond._opt is not None:
        assert bool(torch.isfinite(cond._opt).all()) and float(cond._opt[1].abs().max()) == 0.0
    if aux is None:
        assert float(g[1].abs().max()) == 0.0
    else:                                      # the auxiliary losses act on the prediction: their gradient alone, on the colours
        xa = x0[1:2].clone().requires_grad_(True)
        (ga,) = torch.autograd.grad(D.aux_loss(xa, aux), xa)
        assert float((g[1:2].cpu() - ga).abs().max()) < 3e-5 * float(ga.abs().max()) + 1e-9 and float(g[1, 3].abs().max()) == 0.0
    one = hip_cond(pkg, "underwater_physical_revised", 1, optimizer, 1e-3, 5, aux)
    one.set_measurement_mask(mask[0:1], batch=1, device=DEV)
    g1, loss1 = one.loss_grad_x0(x0[0:1].to(DEV), y[0:1].to(DEV), freeze_phi=False)
    assert torch.equal(g1[0], g[0]) and torch.equal(loss1[0], loss[0]) and torch.equal(one.operator.phi[0], phi[0])


# ------------------------------------------------------------------------------------------------------------ 4: masked pixels have no influence
@pytest.mark.parametrize("opname", list(OPS))
def test_measurement_under_a_zero_mask_has_no_influence(pkg, opname):
    H, W = SHAPES[1]
    x0, y = phys_inputs(2, H, W, 51)
    mask = make_masks("binary", 2, H, W, 52)
    y2 = torch.where(mask == 0, torch.rand(y.shape, generator=torch.Generator().manual_seed(53)) * 40 - 20, y)
    assert not torch.equal(y, y2)
    outs = []
    for yy in (y, y2):
        cond = hip_cond(pkg, opname, 2, "adam", 2e-3, 5, AUX)
        cond.set_measurement_mask(mask, batch=2, device=DEV)
        g, loss = cond.loss_grad_x0(x0.to(DEV), yy.to(DEV), freeze_phi=False)
        outs.append((g.clone(), loss.clone(), cond.operator.phi.clone()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------------------ 5: ps
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("shape", SHAPES)
def test_masked_ps_loss_grad_vs_float64(pkg, C, shape):
    """loss[b] = ||M (y - x0[:, 0:3])||, g = -M^2 (y - x0) / loss on the colours and 0 beyond, per image, against float64 at the bars
    of the unmasked osm_ps_loss_grad_c test; a fully masked image has loss 0, g exactly 0, all finite."""
    _, _, M, CM = pkg
    H, W = shape
    B = 3
    x0, y = phys_inputs(B, H, W, 61)
    x0 = x0[:, :C].contiguous()
    mask = make_masks("uniform", B, H, W, 62)
    mask[1] = make_masks("binary", 1, H, W, 63)[0]
    mask[2] = 0.0
    cond = CM.get_conditioning_method("ps", M.get_operator("noise", device=DEV, batch_size=B), M.get_noise("gaussian", sigma=0.0),
                                      scale="0.3")
    cond.set_measurement_mask(mask, batch=B, device=DEV)
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g, loss = g.cpu().double(), loss.cpu().double()
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss).all())
    r = mask.double() * (y.double() - x0[:, 0:3].double())
    L = (r ** 2).sum(dim=(1, 2, 3)).sqrt()
    for b in range(2):
        want = -(mask[b].double() * r[b]) / L[b]
        assert abs(float(loss[b]) - float(L[b])) <= 2e-6 * float(L[b]), (b, float(loss[b]), float(L[b]))
        assert float((g[b, 0:3] - want).abs().max()) <= 2e-7 + 1e-5 * float(want.abs().max())
    assert float(g[:, 3:].abs().max() if C == 4 else 0.0) == 0.0
    assert float(loss[2]) == 0.0 and float(g[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 6: exposure mask
def exposure_np(y, lo, hi, soft, per_pixel):
    f = np.float32
    v = f(0.5) * (y + f(1.0))
    if soft > 0:
        m = np.clip((f(hi) - v) / f(soft), f(0), f(1)) * np.clip((v - f(lo)) / f(soft), f(0), f(1))
    else:
        m = ((v > f(lo)) & (v < f(hi))).astype(f)
    if per_pixel:
        m = np.broadcast_to(m.min(axis=1, keepdims=True), m.shape)
    return m.astype(f)


@pytest.mark.parametrize("per_pixel", [False, True])
@pytest.mark.parametrize("soft", [0.0, 0.02, 0.125])
def test_exposure_mask_vs_numpy(pkg, soft, per_pixel):
    from osmosis_diffusion_code_amd import ops
    H, W = SHAPES[1]
    B, lo, hi = 2, 0.25, 0.75                                        # (v = 0.25 / 0.75 exactly at y = -0.5 / 0.5)
    y = torch.rand(B, 3, H, W, generator=torch.Generator().manual_seed(71)) * 2.2 - 1.1
    y[0, 0, 0, :4] = torch.tensor([-0.5, 0.5, -1.0, 1.0])
    y[1, 2, 5, :6] = torch.tensor([-0.5, 0.5, -0.5 + 2 * soft, 0.5 - 2 * soft, -0.5 + soft, 0.5 - soft])
    out = torch.full((B, 3, H * W), -1.0, device=DEV)
    ops.exposure_mask(y.to(DEV), out, B, H * W, lo, hi, soft, per_pixel)
    got, want = out.cpu().numpy().reshape(B, 3, H, W), exposure_np(y.numpy(), lo, hi, soft, per_pixel)
    assert got.min() >= 0.0 and got.max() <= 1.0 and 0.2 < (got == 0).mean() < 0.95 and (got == 1).any()
    if soft == 0.0:
        assert np.array_equal(got, want) and set(np.unique(got)) == {0.0, 1.0}
    else:
        assert np.abs(got - want).max() <= 1e-6
    if per_pixel:
        assert np.array_equal(got, np.broadcast_to(got.min(axis=1, keepdims=True), got.shape))
    else:
        assert got[0, 0, 0, 0] == 0.0 and got[0, 0, 0, 1] == 0.0      # exactly at lo / hi: outside
    from osmosis_diffusion_code_amd._lib import OsmosisHipError
    with pytest.raises(OsmosisHipError, match="low must not exceed high"):
        ops.exposure_mask(y.to(DEV), out, B, H * W, 0.9, 0.1, 0.0, False)
    with pytest.raises(OsmosisHipError, match="soft"):
        ops.exposure_mask(y.to(DEV), out, B, H * W, 0.1, 0.9, -0.1, False)


# ------------------------------------------------------------------------------------------------------------ 7: torch.library
def test_opcheck_of_the_masked_operators(pkg):
    from osmosis_diffusion_code_amd import torch_ops
    assert {"phys_loss_grad_m", "ps_loss_grad_mc", "exposure_mask"} <= set(torch_ops.OPS)
    H, W = 12, 10
    x0, y = (t.to(DEV) for t in phys_inputs(2, H, W, 81))
    mask = make_masks("b1hw", 2, H, W, 82).to(DEV)
    cond = hip_cond(pkg, "underwater_physical_revised", 2, aux=AUX)
    icfg, fcfg = torch_ops.phys_config(cond._prepare(2, H * W, x0.device)["desc"])
    phi = cond.operator.phi.clone()
    args = (x0, y, mask, phi, icfg, fcfg, 3, False)
    loss, g, phi_new = torch.ops.osmosis.phys_loss_grad_m(*args)
    cond.set_measurement_mask(mask.cpu(), batch=2, device=DEV)
    cond.n_iter = 3
    g2, loss2 = cond.loss_grad_x0(x0, y, freeze_phi=False)
    assert torch.equal(loss, loss2) and torch.equal(g, g2) and torch.equal(phi_new, cond.operator.phi) and torch.equal(
        phi, hip_cond(pkg, "underwater_physical_revised", 2).operator.phi)
    torch.library.opcheck(torch.ops.osmosis.phys_loss_grad_m.default, args)
    torch.library.opcheck(torch.ops.osmosis.ps_loss_grad_mc.default, (x0[:, 0:3].contiguous(), y, mask))
    torch.library.opcheck(torch.ops.osmosis.ps_loss_grad_mc.default, (x0, y, mask.expand(2, 3, H, W).contiguous()))
    torch.library.opcheck(torch.ops.osmosis.exposure_mask.default, (y, 0.02, 0.98, 0.02, True))
    assert torch.ops.osmosis.exposure_mask(y, 0.02, 0.98).shape == y.shape


# ============================================================================================================ chain level
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")                   # the tiny 3 -> 6 network
COND = dict(loss_function="norm", loss_weight="depth", weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
            gradient_clip="True,0.005")
OPERATORS = {
    "underwater_physical_revised": dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_a_eta="1e-5",
                                        phi_a_learn_flag=True, phi_b="0.95, 0.8, 0.8", phi_b_eta="1e-5", phi_b_learn_flag=True,
                                        phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True),
    "haze_physical": dict(optimizer="sgd", depth_type="gamma", value="1.4,1.4,1", phi_ab="1.0", phi_ab_eta="1e-5", phi_ab_learn_flag=True,
                          phi_inf="0.14, 0.29, 0.49", phi_inf_eta="1e-5", phi_inf_learn_flag=True),
}
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)
CH, CW, T = 16, 24, 10


def make_model(unet, kw=TINY_KW):
    cfg = U.UNetConfig.from_create_model_kwargs(**kw)
    m = unet.create_model(**kw)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    m.conv_mode = "f32"
    return m


@pytest.fixture(scope="module")
def model48(pkg):
    return make_model(pkg[0])


@pytest.fixture(scope="module")
def model36(pkg):
    return make_model(pkg[0], RGB_KW)


def make_sampler(gd, name="ddpm", **kw):
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    args.update(kw)
    return gd.get_sampler(name)(**args)


def osmosis_cond(pkg, opname, pat, B=1):
    _, _, M, CM = pkg
    operator = M.get_operator(opname, device=DEV, batch_size=B, **OPERATORS[opname])
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **pat, aux_loss=AUX)


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _free_running_bar(drift):
    """As in test_pcgs_gpu.py / test_dynthr_gpu.py: tight for well-conditioned chains, the north-star 1e-3 for mildly amplifying
    ones, None (teacher-forced) for chains the oracle itself cannot reproduce to 1e-3."""
    if drift <= 1e-4:
        return max(2e-5, 10.0 * drift)
    return 1e-3 if drift <= 1e-3 else None


def chain_inputs(B, C, seed, n=T):
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, CH, CW, generator=g)
    y = torch.rand(B, 3, CH, CW, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, CH, CW, generator=g)
    mask = torch.rand(B, 3, CH, CW, generator=g) * (torch.rand(B, 1, CH, CW, generator=g) > 0.3).float()
    mask[:, :, 4:9, 6:15] = 0.0                                      # a hole: the inpainting case
    return x_T, y, noise, mask


def _replay_randn_like(monkeypatch, noise, C):
    """torch.randn_like for `_generic_loop`: the C-channel draws on the state replay `noise` in order; with C = 3 the state and the
    measurement have the same shape: p_sample draws first, q_sample second (unused by `ps`) -- the even draws replay."""
    state, orig = {"k": 0}, torch.randn_like

    def replay(t, **kw):
        if C == 3:
            k = state["k"]
            state["k"] += 1
            return noise[k // 2].clone() if k % 2 == 0 else orig(t, **kw)
        if t.shape[1] != C:
            return orig(t, **kw)
        state["k"] += 1
        return noise[state["k"] - 1].clone()
    monkeypatch.setattr(torch, "randn_like", replay)


# ------------------------------------------------------------------------------------------------------------ 8: against the oracle
def _oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask):
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    rop = D.PhysOperator(opname, batch_size=1, depth_type="gamma", value="1.4,1.4,1", **okw)
    rg = MaskedGuidance(rop, n_iter=20, scale=COND["scale"], gradient_clip=COND["gradient_clip"], aux=AUX)
    rg.mask = mask
    trace = []
    D.p_sample_loop(lambda x, t: U.unet_forward(sd, cfg, x, t), tb, x_T, y, rg, PATTERN, [noise[k] for k in range(T)], trace)
    return trace


@pytest.mark.parametrize("opname", ["underwater_physical_revised", "haze_physical"])
def test_fused_masked_osmosis_chain_vs_the_masked_oracle(pkg, monkeypatch, model48, opname):
    """The fused chain with a mask against the oracle's loop with the mask in its residual, same weights, x_T, measurement and noise.
    Bar: from the oracle's own drift under a 1e-6 perturbation of x_T (`_free_running_bar`); where the oracle cannot reproduce
    itself to 1e-3, teacher-forced per index from the oracle's x_in and phi at the north-star 1e-3."""
    _, gd, _, _ = pkg
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    x_T, y, noise, mask = chain_inputs(1, 4, 91)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ref = _oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert = _oracle_chain(opname, cfg, sd, tb, x_T + bump, y, noise, mask)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(tb.timestep_map)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)

    def hip(x_start, index_range=None, phi0=None, k0=0):
        cond = osmosis_cond(pkg, opname, PATTERN)
        if phi0 is not None:
            for name, (off, m) in cond.operator._slots().items():
                cond.operator.phi[0, off:off + m] = phi0[name].reshape(-1)[:m].to(DEV)
        trace = []
        kw = {} if index_range is None else {"index_range": index_range}
        sampler.p_sample_loop(model=model48, x_start=x_start.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k0 + k], trace=trace, measurement_mask=mask, **kw)
        return trace, cond

    def errs(a, b, slots):
        e_phi = max(float((a["phi"][0, off:off + m].cpu() - b["phi"][n].reshape(-1)[:m]).abs().max()) for n, (off, m) in slots.items())
        return (float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max()),
                abs(float(a["loss"][0]) - float(np.asarray(b["loss"]).reshape(-1)[0])) / float(np.asarray(b["loss"]).reshape(-1)[0]), e_phi)
    if bar is not None:
        trace, cond = hip(x_T)
        assert len(trace) == T
        slots = cond.operator._slots()
        e_img, e_x0, e_loss, e_phi = (max(v) for v in zip(*(errs(a, b, slots) for a, b in zip(trace, ref))))
        f_img, f_x0, f_loss, f_phi = errs(trace[-1], ref[-1], slots)
        msg = (f"MASKCHAIN {opname}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
               f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}; worst over the chain: x_out {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
               f"phi {e_phi:.2e}")
        print(msg)
        # final image and pred_xstart under the drift-derived bar; loss and phi follow them (a 1e-5 move of x0 moves the loss by
        # up to 2 w sqrt(3 HW) 1e-5 ~ 1e-4 relative): reported, and held to what such a move allows
        assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
        return
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(T):
        idx = T - 1 - k
        trace, cond = hip(ref[k]["x_in"], (idx, idx), None if k == 0 else ref[k - 1]["phi"], k0=k)
        worst = [max(w, e) for w, e in zip(worst, errs(trace[0], ref[k], cond.operator._slots()))]
    msg = (f"MASKCHAIN {opname}: oracle drift_1e-6 {drift:.2e} > 1e-3, teacher-forced per index: x_out {worst[0]:.2e} x0 {worst[1]:.2e} "
           f"loss(rel) {worst[2]:.2e} phi {worst[3]:.2e}")
    print(msg)
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 2e-5 and worst[3] < 2e-6, msg


# ------------------------------------------------------------------------------------------------------------ 9: batches
def _batch_chain(pkg, monkeypatch, model, sl, x_T, y, noise, mask):
    _, gd, _, _ = pkg
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    cond = osmosis_cond(pkg, "underwater_physical_revised", PATTERN, B=sl.stop - sl.start)
    nd = noise[:, sl].to(DEV)
    out = sampler.p_sample_loop(model=model, x_start=x_T[sl].to(DEV), measurement=y[sl].to(DEV), measurement_cond_fn=cond.conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                                noise_fn=lambda k, shape: nd[k], measurement_mask=mask[sl])
    monkeypatch.undo()
    return out


def _same_bits(a, b, what):
    e = {"img": float((a[0] - b[0]).abs().max()), "x0": float((a[3] - b[3]).abs().max()),
         "loss": float(np.abs(np.asarray(a[2]) - np.asarray(b[2])).max()),
         "phi": max(float((a[1][n] - b[1][n]).abs().max()) for n in a[1])}
    print(f"MASKBATCH {what}: max-abs differences {e}")
    assert torch.equal(a[0], b[0]) and torch.equal(a[3], b[3]) and np.array_equal(a[2], b[2]), (what, e)
    for n in a[1]:
        assert torch.equal(a[1][n], b[1][n]), (what, n, e)


def test_batch_of_two_with_per_image_masks_equals_two_single_runs(pkg, monkeypatch, model48):
    x_T, y, noise, mask = chain_inputs(2, 4, 92)
    both = _batch_chain(pkg, monkeypatch, model48, slice(0, 2), x_T, y, noise, mask)
    assert bool(torch.isfinite(both[0]).all())
    for i in range(2):
        one = _batch_chain(pkg, monkeypatch, model48, slice(i, i + 1), x_T, y, noise, mask)
        _same_bits((both[0][i:i + 1], {n: v[i:i + 1] for n, v in both[1].items()}, both[2][i:i + 1], both[3][i:i + 1]), one,
                   f"image {i} of B = 2 vs its B = 1 run")


def test_masked_batch_walked_in_two_chunks_equals_one_pass(pkg, monkeypatch, model48):
    x_T, y, noise, mask = chain_inputs(2, 4, 92)
    whole = _batch_chain(pkg, monkeypatch, model48, slice(0, 2), x_T, y, noise, mask)
    os.environ["OSM_MAX_BATCH"] = "1"
    try:
        chunked = _batch_chain(pkg, monkeypatch, model48, slice(0, 2), x_T, y, noise, mask)
    finally:
        os.environ.pop("OSM_MAX_BATCH", None)
    _same_bits(whole, chunked, "one pass vs two chunks")


# ------------------------------------------------------------------------------------------------------------ 10: fused vs generic
@pytest.mark.parametrize("case", ["local_M2", "clip_denoised", "dynamic_threshold"])
def test_masked_fused_chain_equals_the_masked_generic_loop(pkg, monkeypatch, model48, case):
    """Both loops with the same mask and the same injected noise, at the bars test_pcgs_gpu.py / test_dynthr_gpu.py hold the unmasked
    pairs to (image and pred_xstart 1e-4, loss rtol 1e-5, phi 1e-6)."""
    _, gd, _, _ = pkg
    pat = dict(PATTERN, local_M=2, s_start=0.6, s_end=0.2) if case == "local_M2" else PATTERN
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, T))
    x_T, y, noise, mask = chain_inputs(1, 4, 93, n)
    noise = noise.to(DEV)

    def run(fused):
        sampler = make_sampler(gd, clip_denoised=case == "clip_denoised", dynamic_threshold=case == "dynamic_threshold")
        cond = osmosis_cond(pkg, "underwater_physical_revised", pat)
        kw = dict(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False,
                  save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat, measurement_mask=mask)
        if fused:
            _no_generic(monkeypatch, sampler)
            out = sampler.p_sample_loop(noise_fn=lambda k, shape: noise[k], **kw)
        else:
            if case == "local_M2":
                monkeypatch.setenv("OSM_FUSED_PCGS", "0")
            elif case == "dynamic_threshold":
                monkeypatch.setenv("OSM_FUSED_DYNTHR", "0")
            else:                              # no switch for clip_denoised: the conditioner declines the fused loop, its step stays
                cond.hip_ok = lambda: False
            assert sampler._fast_path_ok(model48, cond.conditioning, "osmosis", False, pat, tuple(x_T.shape)) is None
            _replay_randn_like(monkeypatch, noise, 4)
            out = sampler.p_sample_loop(**kw)
        monkeypatch.undo()
        return out
    f, g = run(True), run(False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"MASKGENERIC {case}: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6
    assert np.allclose(f[2], g[2], rtol=1e-5)


# ------------------------------------------------------------------------------------------------------------ 11: ps = inpainting
MEASURED_RGB = {"rg.ddpm.c36": 5.960e-07, "rg.ddim.c36": 7.153e-07}      # tests/test_rgb_gpu.py MEASURED, the unmasked pairs


@pytest.mark.parametrize("net,name", [("c36", "ddpm"), ("c36", "ddim"), ("c48", "ddpm")])
def test_masked_ps_chain_fused_vs_the_generic_loop(pkg, monkeypatch, model48, model36, net, name):
    """`ps` with a mask: fused against `_generic_loop`, whose `ps` step is pure autograd (`ConditioningMethod.grad_and_value`) over
    the HIP UNet.  Bars: the fused-vs-generic bar of tests/test_rgb_gpu.py for the tiny 3 -> 6 network (`chain_bar` of the
    unmasked chain: min(5 x measured, 10 x drift_1e-6)); 1e-4 for the 4 -> 8 network (test_pcgs_gpu.py)."""
    _, gd, M, CM = pkg
    C = 3 if net == "c36" else 4
    model = model36 if C == 3 else model48
    x_T, y, noise, mask = chain_inputs(1, C, 94)
    noise = noise.to(DEV)
    if C == 3:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[f"rg.{name}.c36"], 10.0 * float(gold[f"rg.{name}.c36.drift_1e-6"]))
    else:
        bar = 1e-4
    sampler = make_sampler(gd, name)
    pretrain = "imagenet" if C == 3 else "osmosis"

    def make_cond(third_party=False):
        cls = CM.PosteriorSampling
        if third_party:
            cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {})
        return cls(M.get_operator("noise", device=DEV, batch_size=1), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    kw = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), record=False, save_root=None, pretrain_model=pretrain,
              rgb_guidance=True, sample_pattern=PATTERN, measurement_mask=mask)
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=make_cond().conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = make_cond(third_party=C == 4)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, PATTERN, tuple(x_T.shape)) is None
    _replay_randn_like(monkeypatch, noise, C)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    # the hole is not pulled towards the measurement: no data-term gradient there at any step
    hole = max(float(r["grad"][:, 0:3, 4:9, 6:15].abs().max()) for r in trace)
    unmasked = sampler.p_sample_loop(measurement_cond_fn=make_cond().conditioning, noise_fn=lambda k, shape: noise[k],
                                     **dict(kw, measurement_mask=None))
    print(f"MASKPS {net} {name}: fused vs generic {e:.3e} (bar {bar:.3e}); masked vs unmasked chain "
          f"{float((f - unmasked).abs().max()):.2e}")
    assert bool(torch.isfinite(f).all()) and e <= bar
    assert not torch.equal(f, unmasked)
    assert hole > 0.0                          # (the gradient through the network reaches the hole; the data term itself does not:)
    x0, gdat = trace[-1]["x0"], None
    cond = make_cond()
    cond.set_measurement_mask(mask, batch=1, device=DEV)
    gdat, _ = cond.loss_grad_x0(x0, y.to(DEV))
    assert float(gdat[:, :, 4:9, 6:15].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 12: restore_image
def test_restore_image_with_the_auto_exposure_config(pkg, monkeypatch, model48, tmp_path):
    """A synthetic photo with one saturated and one black patch through `restore_image` with `measurement.mask.auto_exposure`: the
    result carries the mask, 0 on both patches and 1 away from their `soft` margins; the chain ran fused; `save_outputs` writes
    `<name>_mask.png`."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(95)
    photo01 = 0.2 + 0.6 * torch.rand(1, 3, CH, CW, generator=g)              # well inside (low + soft, high - soft)
    photo01[:, :, 2:6, 3:9] = 1.0                                            # blown highlight
    photo01[:, :, 9:14, 12:20] = 0.0                                         # crushed shadow
    photo01[:, 0, 0, 0] = 0.99                                               # one clipped channel of one pixel
    ref = (2 * photo01 - 1).to(DEV)
    auto = {"low": 0.02, "high": 0.98, "soft": 0.02, "per_pixel": False}
    cfg = {"measurement": {"operator": dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised"),
                           "noise": {"name": "clean"}, "mask": {"auto_exposure": auto}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),      # (clip_denoised: a chain from t = 999 on seeded weights stays finite)
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    res = sampling.restore_image(model48, ref, cfg, noise_seed=7)[-1]
    m = res["mask"]
    assert m.shape == (1, 3, CH, CW) and m.device.type == "cpu" and bool(torch.isfinite(res["sample"]).all())
    assert float(m[:, :, 2:6, 3:9].max()) == 0.0 and float(m[:, :, 9:14, 12:20].max()) == 0.0
    away = torch.ones(1, 3, CH, CW, dtype=torch.bool)
    away[:, :, 2:6, 3:9] = False
    away[:, :, 9:14, 12:20] = False
    away[:, 0, 0, 0] = False
    assert float(m[away].min()) == 1.0 and float(m[0, 0, 0, 0]) == 0.0 and float(m[0, 1, 0, 0]) == 1.0
    # per_pixel drops the whole pixel; an explicit mask multiplies in
    cfg["measurement"]["mask"]["auto_exposure"] = dict(auto, per_pixel=True)
    extra = torch.ones(1, 1, CH, CW)
    extra[..., :, 22:] = 0.5
    m2 = sampling.restore_image(model48, ref, cfg, noise_seed=7, mask=extra)[-1]["mask"]
    assert float(m2[0, :, 0, 0].max()) == 0.0 and float(m2[..., 22:].max()) == 0.5 and float(m2[:, :, 7, 0:3].min()) == 1.0
    paths = sampling.save_outputs(res, ref, str(tmp_path), "photo")
    assert paths["mask"].endswith("photo_mask.png") and os.path.getsize(paths["mask"]) > 0
    del cfg["measurement"]["mask"]
    plain = sampling.restore_image(model48, ref, cfg, noise_seed=7)[-1]
    assert "mask" not in plain and "mask" not in sampling.save_outputs(plain, ref, str(tmp_path / "plain"), "photo")
    assert not torch.equal(plain["sample"], res["sample"])
