"""The water / haze data term through a blur / super-resolution / PSF operator on the HIP path (`degradation=` of the physical
operators; include/osmosis_physlin.h).

Kernel level: `loss_grad_x0` against the oracle of tests/physlin_oracle.py (A applied in float64 from the fp32 tables / taps the
kernels read), a delta PSF against the plain entry point, bit-equalities (one C call vs the single-launch entry points, batch vs
single images, repeats, a mask of ones), the fully masked image, a PSF whose gain is not 1, torch.library.opcheck.
Chain level (the tiny 4 -> 8 network in f32, a 16 x 24 image, a 10-index respaced chain, injected noise, `_generic_loop` patched to
raise): the fused chain against the oracle's own loop with the composed guidance, a batch walked in chunks, `restore_image` with the
config key."""
import os

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U
from physlin_oracle import DEGRADATIONS, LinGuidance, dense_operator, oracle_inner_loop
from test_mask_gpu import (AUX, COND, OPERATORS, OPS, PATTERN, TINY_KW, T, _free_running_bar, _no_generic, _same_bits, etas, make_masks,
                           make_sampler, model48, pkg)  # noqa: F401  (pkg, model48: fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# image grids: HW = 1224 (two reduce workgroups of 1024 pixels, the second a ragged 200) and 1073 (odd); the x2 operators take the
# images whose measurements have those sizes, so both grids of a chain have two workgroups with a ragged tail
SAME = [(36, 34), (37, 29)]
GRIDS = {"gaussian_blur": SAME, "motion_blur": SAME, "psf_blur": SAME, "sr2_bicubic": [(72, 68)], "sr2_box": [(74, 58)]}
# (loss_function, loss_weight, auxiliary losses, optimizer, mask): cycled over the parametrised cases, not a full product
CONFIGS = [("norm", "depth", True, "sgd", None), ("mse", "none", False, "adam", "uniform"), ("norm", "none", True, "adam", "binary"),
           ("mse", "depth", False, "sgd", "binary"), ("norm", "depth", False, "adam", "uniform"), ("mse", "depth", True, "sgd", None)]
ETA = {"sgd": 1e-3, "adam": 2e-3}


def lin_inputs(B, H, W, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g)).clamp(-1.0, 1.0)      # depth >= -1: the gamma bases stay positive
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    return x0, y


def lin_cond(pkg, opname, deg, B, optimizer="sgd", n_iter=5, aux=None, loss_function="norm", loss_weight="depth"):
    _, _, M, CM = pkg
    okw = OPS[opname]
    oper = M.get_operator(opname, device=DEV, batch_size=B, optimizer=optimizer, degradation=deg, **okw, **etas(okw, ETA[optimizer]))
    return CM.get_conditioning_method("osmosis", oper, M.get_noise("clean"), loss_function=loss_function, loss_weight=loss_weight,
                                      weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
                                      gradient_clip="False,0", n_iter=n_iter, aux_loss=aux, pattern="pcgs")


def vs_oracle(pkg, opname, degname, cfg, H, W, seed, deg=None):
    """B = 2, 5 inner iterations: (loss rel, phi abs, grad abs, grad scale) worst over the two images, each against its own oracle run
    (the oracle's norm is joint over a batch)."""
    loss_function, loss_weight, aux, optimizer, mkind = cfg
    aux = AUX if aux else None
    deg = DEGRADATIONS[degname] if deg is None else deg
    cond = lin_cond(pkg, opname, deg, 2, optimizer, 5, aux, loss_function, loss_weight)
    h, w = cond.operator.out_shape(H, W)
    x0, y = lin_inputs(2, H, W, h, w, seed)
    mask = None if mkind is None else make_masks(mkind, 2, h, w, seed + 1000)
    if mask is not None:
        cond.set_measurement_mask(mask, batch=2, device=DEV)
    gx0, sep = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
    gx0, sep, got_phi = gx0.cpu(), sep.cpu().numpy(), {n: v.cpu() for n, v in cond.operator.variables().items()}
    okw = dict(OPS[opname], **etas(OPS[opname], ETA[optimizer]))
    worst = [0.0, 0.0, 0.0, 0.0]
    for b in range(2):
        want_sep, want_phi, want_g = oracle_inner_loop(opname, okw, cond.operator.degradation, x0[b:b + 1], y[b:b + 1],
                                                       None if mask is None else mask[b:b + 1], 5, optimizer, aux, loss_function,
                                                       loss_weight)
        e_loss = abs(float(sep[b]) - want_sep) / want_sep
        e_phi = max(float((got_phi[n][b:b + 1] - want_phi[n]).abs().max()) for n in want_phi)
        scale = float(want_g.abs().max())
        e_g = float((gx0[b:b + 1] - want_g.to(torch.float32)).abs().max())
        worst = [max(worst[0], e_loss), max(worst[1], e_phi), max(worst[2], e_g / scale), scale]
    return worst


# ------------------------------------------------------------------------------------------------------------ 1: against the oracle
@pytest.mark.parametrize("degname", list(DEGRADATIONS))
@pytest.mark.parametrize("opname", list(OPS))
def test_composed_loss_grad_x0_vs_the_oracle(pkg, opname, degname):
    """Loss, phi after the inner iterations and dL/dx0 against autograd through the composed oracle.  Bars: the ones
    tests/test_guidance_gpu.py / test_mask_gpu.py hold the plain kernels to: loss 3e-5 relative, phi 3e-6 (adam 5e-6), gradient 3e-5
    of its largest entry."""
    i = list(OPS).index(opname) * len(DEGRADATIONS) + list(DEGRADATIONS).index(degname)
    grids = GRIDS[degname]
    for k in range(2):
        cfg = CONFIGS[(2 * i + k) % len(CONFIGS)]
        H, W = grids[k % len(grids)]
        e_loss, e_phi, e_g, scale = vs_oracle(pkg, opname, degname, cfg, H, W, 100 + 2 * i + k)
        print(f"PHYSLIN {opname} {degname} {cfg} {H}x{W}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of its max {scale:.2e}")
        assert e_loss <= 3e-5, (opname, degname, cfg, e_loss)
        assert e_phi <= (5e-6 if cfg[3] == "adam" else 3e-6), (opname, degname, cfg, e_phi)
        assert e_g <= 3e-5, (opname, degname, cfg, e_g)


# ------------------------------------------------------------------------------------------------------------ 2: A = identity
@pytest.mark.parametrize("masked", [False, True], ids=["nomask", "mask"])
def test_delta_psf_is_the_plain_entry_point(pkg, masked):
    """A 3 x 5 PSF that is 1 at its centre: the composed route against osm_phys_optimize(_m) on the same inputs, within the sum of the
    two bars of test 1 (not bit-equal: 2 (A I) - 1 contracts differently from the inline residual)."""
    _, _, M, CM = pkg
    k = np.zeros((3, 5))
    k[1, 2] = 1.0
    delta = {"name": "psf_blur", "kernel": k, "normalize": False}
    for n, (H, W) in enumerate(SAME):
        for loss_function in ("norm", "mse"):
            x0, y = lin_inputs(2, H, W, H, W, 300 + n)
            mask = make_masks("uniform", 2, H, W, 310 + n) if masked else None
            outs = []
            for deg in (None, delta):
                cond = lin_cond(pkg, "underwater_physical_revised", deg, 2, "sgd", 5, AUX, loss_function, "depth")
                if mask is not None:
                    cond.set_measurement_mask(mask, batch=2, device=DEV)
                g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
                outs.append((g.clone(), loss.clone(), cond.operator.phi.clone()))
            (g0, l0, p0), (g1, l1, p1) = outs
            e_loss = float(((l1 - l0).abs() / l0).max())
            e_phi = float((p1 - p0).abs().max())
            e_g = float((g1 - g0).abs().max()) / float(g0.abs().max())
            print(f"PHYSLIN delta {H}x{W} {loss_function} masked={masked}: composed vs plain loss(rel) {e_loss:.2e} phi {e_phi:.2e} "
                  f"grad {e_g:.2e} of its max")
            assert e_loss <= 6e-5 and e_phi <= 6e-6 and e_g <= 6e-5


# ------------------------------------------------------------------------------------------------------------ 3: bit-equalities
@pytest.mark.parametrize("degname,optimizer,loss_weight", [("gaussian_blur", "sgd", "depth"), ("sr2_bicubic", "adam", "depth"),
                                                           ("psf_blur", "adam", "none"), ("sr2_box", "sgd", "none")])
def test_composed_route_bit_equalities(pkg, monkeypatch, degname, optimizer, loss_weight):
    """osm_phys_optimize_lin is the same launches as the single-launch entry points (OSM_PHYS_PY_LOOP=1); B = 2 is two B = 1 calls;
    a repeated call repeats; a mask of ones is no mask."""
    H, W = GRIDS[degname][0]
    deg = DEGRADATIONS[degname]

    def run(sl=slice(0, 2), mask=None, py_loop=False, twice=False):
        B = sl.stop - sl.start
        cond = lin_cond(pkg, "underwater_physical", deg, B, optimizer, 5, AUX, "norm", loss_weight)
        h, w = cond.operator.out_shape(H, W)
        x0, y = lin_inputs(2, H, W, h, w, 400)
        if mask is not None:
            cond.set_measurement_mask(torch.ones(B, *mask, h, w), batch=B, device=DEV)
        monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1" if py_loop else "0")
        out = []
        for _ in range(2 if twice else 1):
            g, loss = cond.loss_grad_x0(x0[sl].to(DEV), y[sl].to(DEV), freeze_phi=False)
            out.append((g.clone(), loss.clone(), cond.operator.phi.clone(), None if cond._opt is None else cond._opt.clone()))
        return out
    want = run()[0]
    assert all(bool(torch.isfinite(t).all()) for t in want if t is not None)

    def same(got, want, what):
        for name, a, b in zip(("g", "loss", "phi", "opt"), got, want):
            assert (a is None and b is None) or torch.equal(a, b), (degname, what, name, float((a - b).abs().max()))
    same(run(py_loop=True)[0], want, "single-launch entry points")
    same(run()[0], want, "repeat")
    same(run(mask=(3,))[0], want, "mask of ones [B,3,h,w]")
    same(run(mask=(1,), py_loop=True)[0], want, "mask of ones [B,1,h,w], single launches")
    for b in range(2):
        one = run(slice(b, b + 1))[0]
        same(one, tuple(None if t is None else t[b:b + 1] for t in want), f"image {b} alone")
    # a second step of the same conditioner (the workspaces are reused, adam's state carries on): the same from both routes
    same(run(twice=True)[1], run(py_loop=True, twice=True)[1], "second call")


# ------------------------------------------------------------------------------------------------------------ 4: fully masked image
@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("aux", [None, AUX], ids=["noaux", "aux"])
def test_fully_masked_image_through_a_degradation(pkg, aux, optimizer):
    """Image 1 of a batch of 2 is masked out on the measurement's grid: loss 0, phi and the optimizer state bit-unchanged, g exactly 0
    without auxiliary losses (with them: what they alone give); image 0 is bit-equal to its own B = 1 run."""
    H, W = 72, 68
    cond = lin_cond(pkg, "underwater_physical_revised", DEGRADATIONS["sr2_bicubic"], 2, optimizer, 5, aux)
    h, w = cond.operator.out_shape(H, W)
    x0, y = lin_inputs(2, H, W, h, w, 500)
    mask = make_masks("uniform", 2, h, w, 501)
    mask[1] = 0.0
    phi0 = cond.operator.phi.clone()
    cond.set_measurement_mask(mask, batch=2, device=DEV)
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
    phi = cond.operator.phi
    assert bool(torch.isfinite(g).all()) and bool(torch.isfinite(loss).all()) and bool(torch.isfinite(phi).all())
    assert float(loss[1]) == 0.0 and torch.equal(phi[1], phi0[1]) and not torch.equal(phi[0], phi0[0])
    if cond._opt is not None:
        assert bool(torch.isfinite(cond._opt).all()) and float(cond._opt[1].abs().max()) == 0.0 and float(cond._opt[0].abs().max()) > 0
    if aux is None:
        assert float(g[1].abs().max()) == 0.0
    else:
        xa = x0[1:2].clone().requires_grad_(True)
        (ga,) = torch.autograd.grad(D.aux_loss(xa, aux), xa)
        assert float((g[1:2].cpu() - ga).abs().max()) < 3e-5 * float(ga.abs().max()) + 1e-9 and float(g[1, 3].abs().max()) == 0.0
    one = lin_cond(pkg, "underwater_physical_revised", DEGRADATIONS["sr2_bicubic"], 1, optimizer, 5, aux)
    one.set_measurement_mask(mask[0:1], batch=1, device=DEV)
    g1, loss1 = one.loss_grad_x0(x0[0:1].to(DEV), y[0:1].to(DEV), freeze_phi=False)
    assert torch.equal(g1[0], g[0]) and torch.equal(loss1[0], loss[0]) and torch.equal(one.operator.phi[0], phi[0])


# ------------------------------------------------------------------------------------------------------------ 5: a gain that is not 1
def test_psf_gain_is_part_of_the_model(pkg):
    """`normalize: False`: the photo is A I with A's own gain.  Doubling the kernel doubles A I and A w bit for bit (a power of two),
    the residual is y - (2 (A I) - 1), not y - A (2 I - 1), and both kernels match the oracle at the bars of test 1."""
    from osmosis_diffusion_code_amd import ops
    H, W = SAME[1]
    k1 = np.asarray(DEGRADATIONS["psf_blur"]["kernel"])
    planes = []
    for gain in (1.0, 2.0):
        deg = {"name": "psf_blur", "kernel": gain * k1, "normalize": False}
        for cfg in (CONFIGS[0], CONFIGS[3]):
            e_loss, e_phi, e_g, scale = vs_oracle(pkg, "underwater_physical_revised", "psf_blur", cfg, H, W, 600, deg=deg)
            print(f"PHYSLIN gain {gain} {cfg}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of its max {scale:.2e}")
            assert e_loss <= 3e-5 and e_phi <= 3e-6 and e_g <= 3e-5
        cond = lin_cond(pkg, "underwater_physical_revised", deg, 2)
        x0, y = (t.to(DEV) for t in lin_inputs(2, H, W, H, W, 600))
        st = cond._prepare(2, H * W, x0.device, grid=(H, W))
        assert st["F"].shape == (2, 4, H * W)                                     # the image and the depth weight
        ops.phys_forward(st["desc"], x0, cond.operator.phi, st["F"])
        ops.phys_lin_apply(st["lin"], st["F"], st["AF"], 2, 4)
        ops.phys_resid(st["desc"], H * W, st["AF"], y, None, st["u"], st["part_r"])
        planes.append((st["F"].clone(), st["AF"].clone(), st["u"].clone(), y))
    (F1, AF1, u1, y), (F2, AF2, u2, _) = planes
    assert torch.equal(F1, F2) and torch.equal(AF2, 2.0 * AF1)
    I = cond.operator.forward(x0).reshape(2, 3, H * W)
    assert float((F1[:, 0:3] - I).abs().max()) <= 2e-7
    A2 = dense_operator(cond.operator.degradation, H, W)                          # (the kernel with gain 2, sum 2.54)
    want = A2(F2.view(2, 4, H, W).cpu()).reshape(2, 4, H * W)
    assert float((AF2.cpu().double() - want).abs().max()) <= 2e-6 * float(want.abs().max()) and float(want[:, 3].min()) > 0
    wt, It = AF2[:, 3:4], AF2[:, 0:3]
    r = (y.reshape(2, 3, H * W) - (2 * It - 1)) * wt
    assert float((u2 - (-2 * wt * r)).abs().max()) <= 1e-5 * float(u2.abs().max())
    assert not torch.allclose(u2, 2 * u1, rtol=1e-2)                              # (2 (A I) - 1 is not linear in the gain)


# ------------------------------------------------------------------------------------------------------------ 6: torch.library
def test_opcheck_of_phys_loss_grad_lin(pkg):
    from osmosis_diffusion_code_amd import torch_ops
    for degname, (H, W) in (("sr2_bicubic", (12, 20)), ("motion_blur", (12, 10))):
        cond = lin_cond(pkg, "underwater_physical_revised", DEGRADATIONS[degname], 2, aux=AUX)
        h, w = cond.operator.out_shape(H, W)
        x0, y = (t.to(DEV) for t in lin_inputs(2, H, W, h, w, 700))
        mask = make_masks("b1hw", 2, h, w, 701).to(DEV)
        icfg, fcfg = torch_ops.phys_config(cond._prepare(2, H * W, x0.device, grid=(H, W))["desc"])
        family, tables, dims = torch_ops.lin_config(cond.operator.degradation, H, W, x0.device)
        phi = cond.operator.phi.clone()
        args = (x0, y, mask, phi, icfg, fcfg, 3, False, family, tables, dims)
        loss, g, phi_new = torch.ops.osmosis.phys_loss_grad_lin(*args)
        cond.set_measurement_mask(mask.cpu(), batch=2, device=DEV)
        cond.n_iter = 3
        g2, loss2 = cond.loss_grad_x0(x0, y, freeze_phi=False)
        assert torch.equal(loss, loss2) and torch.equal(g, g2) and torch.equal(phi_new, cond.operator.phi)
        assert torch.equal(phi, lin_cond(pkg, "underwater_physical_revised", None, 2).operator.phi)      # functional: phi untouched
        torch.library.opcheck(torch.ops.osmosis.phys_loss_grad_lin.default, args)
        torch.library.opcheck(torch.ops.osmosis.phys_loss_grad_lin.default, (x0, y, None, phi, icfg, fcfg, 1, True, family, tables, dims))


# ============================================================================================================ chain level
CH, CW = 16, 24
CHAINS = {
    "revised+gaussian_blur5": ("underwater_physical_revised", dict(name="gaussian_blur", kernel_size=5, intensity=1.0), False),
    "haze+super_resolution2": ("haze_physical", dict(name="super_resolution", scale_factor=2, method="bicubic"), False),
    "revised+super_resolution2+mask": ("underwater_physical_revised", dict(name="super_resolution", scale_factor=2, method="box"), True),
    "haze+motion_blur5": ("haze_physical", dict(name="motion_blur", kernel_size=5), False),
}


def lin_chain_inputs(B, h, w, seed, masked, n=T):
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, 4, CH, CW, generator=g)
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, 4, CH, CW, generator=g)
    mask = None
    if masked:
        mask = torch.rand(B, 3, h, w, generator=g) * (torch.rand(B, 1, h, w, generator=g) > 0.3).float()
        mask[:, :, 2:4, 3:7] = 0.0
    return x_T, y, noise, mask


def chain_cond(pkg, opname, deg, B=1):
    _, _, M, CM = pkg
    operator = M.get_operator(opname, device=DEV, batch_size=B, degradation=deg, **OPERATORS[opname])
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **PATTERN, aux_loss=AUX)


def _oracle_lin_chain(opname, deg_op, cfg, sd, tb, x_T, y, noise, mask):
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    rop = D.PhysOperator(opname, batch_size=1, depth_type="gamma", value="1.4,1.4,1", **okw)
    rg = LinGuidance(rop, n_iter=20, scale=COND["scale"], gradient_clip=COND["gradient_clip"], aux=AUX)
    rg.A, rg.mask = dense_operator(deg_op, CH, CW), mask
    trace = []
    D.p_sample_loop(lambda x, t: U.unet_forward(sd, cfg, x, t), tb, x_T, y, rg, PATTERN, [noise[k] for k in range(T)], trace)
    return trace


@pytest.mark.parametrize("case", list(CHAINS))
def test_fused_composed_chain_vs_the_oracle(pkg, monkeypatch, model48, case):
    """The fused chain with a degradation against the oracle's loop with the composed guidance, same weights, x_T, measurement and
    noise.  Bar: from the oracle's own drift under a 1e-6 perturbation of x_T (`_free_running_bar`); where the oracle cannot
    reproduce itself to 1e-3, teacher-forced per index from the oracle's x_in and phi at the north-star 1e-3 -- the scheme of
    test_fused_masked_osmosis_chain_vs_the_masked_oracle."""
    _, gd, M, _ = pkg
    opname, deg, masked = CHAINS[case]
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    deg_op = M.build_degradation(deg, "cpu")
    h, w = deg_op.out_shape(CH, CW)
    x_T, y, noise, mask = lin_chain_inputs(1, h, w, 191, masked)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ref = _oracle_lin_chain(opname, deg_op, cfg, sd, tb, x_T, y, noise, mask)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert = _oracle_lin_chain(opname, deg_op, cfg, sd, tb, x_T + bump, y, noise, mask)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(tb.timestep_map)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)

    def hip(x_start, index_range=None, phi0=None, k0=0):
        cond = chain_cond(pkg, opname, deg)
        if phi0 is not None:
            for name, (off, m) in cond.operator._slots().items():
                cond.operator.phi[0, off:off + m] = phi0[name].reshape(-1)[:m].to(DEV)
        trace = []
        kw = {} if index_range is None else {"index_range": index_range}
        if mask is not None:
            kw["measurement_mask"] = mask
        sampler.p_sample_loop(model=model48, x_start=x_start.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k0 + k], trace=trace, **kw)
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
        msg = (f"PHYSLINCHAIN {case}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
               f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}; worst over the chain: x_out {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
               f"phi {e_phi:.2e}")
        print(msg)
        assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
        return
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(T):
        idx = T - 1 - k
        trace, cond = hip(ref[k]["x_in"], (idx, idx), None if k == 0 else ref[k - 1]["phi"], k0=k)
        worst = [max(w_, e) for w_, e in zip(worst, errs(trace[0], ref[k], cond.operator._slots()))]
    msg = (f"PHYSLINCHAIN {case}: oracle drift_1e-6 {drift:.2e} > 1e-3, teacher-forced per index: x_out {worst[0]:.2e} x0 {worst[1]:.2e} "
           f"loss(rel) {worst[2]:.2e} phi {worst[3]:.2e}")
    print(msg)
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 2e-5 and worst[3] < 2e-6, msg


# ------------------------------------------------------------------------------------------------------------ 8: chunks
def test_composed_batch_of_three_walked_as_two_chunks_equals_one_pass(pkg, monkeypatch, model48):
    """B = 3 in one engine pass against the same chain walked as chunks of [2, 1] images (two engines, two sets of workspaces): bit
    for bit, with a per-image mask on the measurement's grid."""
    _, gd, M, _ = pkg
    deg = CHAINS["haze+super_resolution2"][1]
    h, w = M.build_degradation(deg, "cpu").out_shape(CH, CW)
    x_T, y, noise, mask = lin_chain_inputs(3, h, w, 192, True)
    nd = noise.to(DEV)

    def run(sizes):
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B, cap: list(sizes)))
        cond = chain_cond(pkg, "underwater_physical_revised", deg, B=3)
        out = sampler.p_sample_loop(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                                    record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                                    noise_fn=lambda k, shape: nd[k], measurement_mask=mask)
        n_states = len(cond._states)
        monkeypatch.undo()
        return out, n_states
    whole, n1 = run([3])
    chunked, n2 = run([2, 1])
    assert (n1, n2) == (1, 2) and bool(torch.isfinite(whole[0]).all())
    _same_bits(whole, chunked, "one pass vs chunks of [2, 1]")


# ------------------------------------------------------------------------------------------------------------ 9: the driver
def test_restore_image_with_the_degradation_config_key(pkg, monkeypatch, model48, tmp_path):
    """`measurement.operator.degradation` through `restore_image` on the tiny network: the photo (64 x 64) is the measurement of the
    network's 256 x 256 grid under x4 super-resolution; the chain runs fused; the result carries `observed` on the photo's grid,
    `norm_loss_final` against it and no `rgb_recon`; the mask lives on the photo's grid; `save_outputs` writes its files."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(195)
    photo = (torch.rand(1, 3, 64, 64, generator=g) * 1.2 - 0.6).to(DEV)
    op_cfg = dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised",
                  degradation={"name": "super_resolution", "scale_factor": 4, "method": "bicubic"})
    cfg = {"measurement": {"operator": op_cfg, "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    mask = torch.ones(1, 1, 64, 64)
    mask[..., 10:20, 30:50] = 0.0
    res = sampling.restore_image(model48, photo, cfg, noise_seed=7, mask=mask)[-1]
    assert res["sample"].shape == (1, 4, 256, 256) and bool(torch.isfinite(res["sample"]).all())
    assert res["observed"].shape == (3, 64, 64) and res["forward_predicted"].shape == (3, 256, 256) and "rgb_recon" not in res
    assert res["mask"].shape == (1, 3, 64, 64) and torch.equal(res["measurement"], photo.cpu())
    # `observed` is 2 A I - 1 at the final phi and pred_xstart, from the oracle's A in float64
    A = dense_operator(M.build_degradation(op_cfg["degradation"], "cpu"), 256, 256)
    want = 2 * A(res["forward_predicted"][None].double())[0] - 1
    assert float((res["observed"].double() - want).abs().max()) <= 1e-5
    assert res["norm_loss_final"] == float(np.round(torch.linalg.norm(res["observed"] - photo.cpu()[0]).numpy(), decimals=3))
    paths = sampling.save_outputs(res, photo, str(tmp_path), "photo")
    assert all(os.path.getsize(p) > 0 for p in paths.values()) and {"input", "rgb", "depth_color", "depth_raw", "grid", "mask"} <= set(paths)
    unmasked = sampling.restore_image(model48, photo, cfg, noise_seed=7)[-1]
    assert "mask" not in unmasked and not torch.equal(unmasked["sample"], res["sample"])
    with pytest.raises(ValueError, match="degradation"):
        sampling.restore_image(model48, torch.zeros(1, 3, 256, 256, device=DEV), cfg, noise_seed=7)


def test_restore_images_in_batches_with_a_degradation(pkg, monkeypatch, model48):
    """`restore_images(batch_size=2)` with x4 super-resolution (the photos 64 x 64, the chains on the 256 x 256 grid): every image's
    result carries its own `observed` on the photo's grid and `norm_loss_final` against it, and is what its batch-1 run gives (the
    bar of the unbatched-vs-batched driver test in tests/test_sampler_gpu.py: 2e-5 on the sample).  The chains are the 3-index
    low-noise sub-chains (`index_range=(2, 0), x_scale=0.05`) on which tests/test_configs_gpu.py compares batched Osmosis chains with
    their batch-1 runs: a 10-index chain from t = T on seeded weights amplifies the network's batch-size-dependent rounding (measured
    on it: sample 1.9e-3, observed 2.6e-5 between B = 2 and B = 1, with every per-image assertion below holding)."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(196)
    photos = [(torch.rand(1, 3, 64, 64, generator=g) * 1.2 - 0.6).to(DEV) for _ in range(2)]
    op_cfg = dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised",
                  degradation={"name": "super_resolution", "scale_factor": 4, "method": "bicubic"})
    cfg = {"measurement": {"operator": op_cfg, "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    sub = dict(index_range=(2, 0), x_scale=0.05)
    two = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=2, noise_seed=7, **sub)
    one = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=1, noise_seed=7, **sub)
    assert sorted(two) == sorted(one) == [0, 1]
    A = dense_operator(M.build_degradation(op_cfg["degradation"], "cpu"), 256, 256)
    for i in range(2):
        r = two[i]
        assert r["observed"].shape == (3, 64, 64) and "rgb_recon" not in r and r["sample"].shape == (1, 4, 256, 256)
        want = 2 * A(r["forward_predicted"][None].double())[0] - 1
        assert float((r["observed"].double() - want).abs().max()) <= 1e-5
        assert r["norm_loss_final"] == float(np.round(torch.linalg.norm(r["observed"] - photos[i].cpu()[0]).numpy(), decimals=3))
        e_s, e_o = float((r["sample"] - one[i]["sample"]).abs().max()), float((r["observed"] - one[i]["observed"]).abs().max())
        print(f"PHYSLINBATCH image {i}: batch of 2 vs alone: sample {e_s:.2e} observed {e_o:.2e}; norm_loss_final {r['norm_loss_final']} / "
              f"{one[i]['norm_loss_final']}")
        assert e_s < 2e-5 and e_o < 2e-5 and abs(r["norm_loss_final"] - one[i]["norm_loss_final"]) <= 2e-3
    assert not torch.equal(two[0]["observed"], two[1]["observed"])
