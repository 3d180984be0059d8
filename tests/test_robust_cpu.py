"""The robust data term without a GPU (include/osmosis_robust.h): the ninth header against the library and `_lib.exports("osmosis_robust.h")`, the
entry points' refusals before any launch, the oracle's self-checks (tests/robust_oracle.py), the effect of the weights on the oracle
alone, the torch route against the oracle, and the host-side refusals."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import robust_oracle as RO
from osmosis_diffusion_code_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"osm_robust_resid", "osm_robust_scale", "osm_robust_weights", "osm_robust_mask"}


# ------------------------------------------------------------------------------------------------------------ header and bindings
def test_header_exports_and_bindings_agree():
    hdr = open(os.path.join(ROOT, "include", "osmosis_robust.h")).read()
    assert set(_lib.exports("osmosis_robust.h")) == NAMES
    for rule in ("1.4826f", "(n_b - 1) >> 1", "n_b >> 1", "huber", "tukey", "cauchy", "sigma_min", "never an fma", "per_pixel"):
        assert rule in hdr, rule                                                  # the contract is stated in the header
    assert "osm_robust" not in open(os.path.join(ROOT, "include", "osmosis_hip.h")).read()    # the main header is what it was
    mk = open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "Makefile")).read()
    assert "osmosis_robust.h" in mk and "robust.hip" in mk
    from osmosis_diffusion_code_amd import ops, torch_ops
    assert all(callable(getattr(ops, n)) for n in ("robust_resid", "robust_scale", "robust_weights", "robust_mask", "robust_desc"))
    assert "robust_mask" in torch_ops.OPS and "robust_mask" not in torch_ops.OPS_C
    schema = str(torch.ops.osmosis.robust_mask.default._schema)
    for arg in ("m_eff", "omega", "sigma", "n_valid"):
        assert re.search(r"Tensor\(a\d+!\) " + arg, schema), schema
    assert schema.count("!") == 4 and schema.endswith("-> ()"), schema
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "osmosis_robust.h" in open(os.path.join(ROOT, doc)).read(), doc
    papers = open(os.path.join(ROOT, "PAPERS.md")).read()
    assert "Huber" in papers and "Beaton" in papers and "Holland" in papers
    total = sum(len(_lib.ABI[h]) for h in list(_lib.ABI)[:9])                     # the nine headers up to this one
    assert total == 125 and f"the library's {total} exports" in open(os.path.join(ROOT, "README.md")).read()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from osmosis_diffusion_code_amd import ops
    lib = _lib.load()
    p = 4096                                                                      # never dereferenced on the host

    def desc(**kw):
        d = ops.robust_desc("tukey", None, "mad", 2.0 / 255.0, False, 2, 48)
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)
    ok = dict(pred=p, bs=192, pa=2.0, pb=-1.0, y=p, M0=p, e=p, sigma=p, n=p, meff=p, omega=p)

    def mask(d=None, **kw):
        a = dict(ok, **kw)
        return lib.osm_robust_mask(d or desc(), a["pred"], a["bs"], a["pa"], a["pb"], a["y"], a["M0"], a["e"], a["sigma"], a["n"], a["meff"],
                                   a["omega"], None)
    cases = [(lambda: mask(pred=None), "null pointer"), (lambda: mask(y=None), "null pointer"), (lambda: mask(e=None), "null pointer"),
             (lambda: mask(meff=None), "null pointer"), (lambda: mask(sigma=None), "sigma / n_valid"), (lambda: mask(n=None), "sigma / n_valid"),
             (lambda: mask(bs=100), "pred_bstride"), (lambda: mask(pa=float("nan")), "pa / pb"), (lambda: mask(desc(B=0)), "bad shape"),
             (lambda: mask(desc(hw=-3)), "bad shape"), (lambda: mask(desc(B=70000)), "too many"), (lambda: mask(desc(loss=3)), "unknown loss"),
             (lambda: mask(desc(loss=-1)), "unknown loss"), (lambda: mask(desc(c=0.0)), "c must be"), (lambda: mask(desc(c=-1.0)), "c must be"),
             (lambda: mask(desc(c=float("nan"))), "c must be"), (lambda: mask(desc(sigma_min=-1e-3)), "sigma_min"),
             (lambda: mask(desc(scale_mode=2)), "scale_mode"), (lambda: mask(desc(scale_mode=1, scale=0.0)), "fixed scale"),
             (lambda: mask(desc(scale_mode=1, scale=-0.5)), "fixed scale"), (lambda: mask(desc(per_pixel=2)), "per_pixel"),
             (lambda: lib.osm_robust_mask(None, p, 192, 2.0, -1.0, p, p, p, p, p, p, p, None), "descriptor"),
             (lambda: lib.osm_robust_resid(desc(), None, 192, 2.0, -1.0, p, p, None), "null pointer"),
             (lambda: lib.osm_robust_resid(desc(), p, 143, 2.0, -1.0, p, p, None), "pred_bstride"),
             (lambda: lib.osm_robust_scale(desc(), None, p, p, p, None), "null pointer"),
             (lambda: lib.osm_robust_scale(desc(), p, p, None, p, None), "null pointer"),
             (lambda: lib.osm_robust_scale(desc(sigma_min=float("inf")), p, p, p, p, None), "sigma_min"),
             (lambda: lib.osm_robust_weights(desc(), p, p, None, p, p, None), "sigma"),
             (lambda: lib.osm_robust_weights(desc(), p, p, p, None, p, None), "null pointer"),
             (lambda: lib.osm_robust_weights(desc(c=0.0), p, p, p, p, p, None), "c must be")]
    for fn, msg in cases:
        assert fn() != 0
        assert msg in lib.osm_last_error().decode(), (msg, lib.osm_last_error().decode())
    for bad in (dict(loss="l1"), dict(c=0.0), dict(c=float("nan")), dict(scale="std"), dict(scale=0.0), dict(scale=-1.0), dict(sigma_min=-1.0)):
        kw = dict(dict(loss="tukey", c=None, scale="mad", sigma_min=2.0 / 255.0, per_pixel=False, B=1, hw=4), **bad)
        with pytest.raises(ValueError, match="robust"):
            ops.robust_desc(**kw)
    with pytest.raises(_lib.OsmosisHipError, match="CPU tensor"):                  # no CPU fall-back
        ops.robust_mask(ops.robust_desc("tukey", None, "mad", 0.0, False, 1, 4), torch.zeros(1, 3, 4), 1.0, 0.0, torch.zeros(1, 3, 4), None,
                        torch.zeros(1, 3, 4), torch.zeros(1), torch.zeros(1, dtype=torch.int32), torch.zeros(1, 3, 4))


# ------------------------------------------------------------------------------------------------------------ the oracle itself
def test_oracle_self_checks():
    rng = np.random.default_rng(0)
    for n in (1, 2, 3, 10, 11, 288, 3671, 3672):
        a = np.abs(rng.standard_normal(n))
        assert RO.median2(a) == np.median(a), n                                   # the two-rank median IS np.median in float64
    u = np.concatenate([np.linspace(0.0, 3.0, 601), [1.0, 1.0 - 1e-12, 1.0 + 1e-12]])
    w, s = RO.omega_of(u, "huber")
    assert np.array_equal(w, np.minimum(1.0, 1.0 / np.maximum(u, 1e-300))) and np.allclose(s * s, w, rtol=1e-15)
    w, s = RO.omega_of(u, "tukey")
    assert np.allclose(w, np.where(np.abs(u) < 1, (1 - u ** 2) ** 2, 0.0), rtol=0, atol=0) and np.array_equal(s, np.where(u < 1, 1 - u * u, 0.0))
    w, s = RO.omega_of(u, "cauchy")
    assert np.array_equal(w, 1.0 / (1.0 + u ** 2)) and np.allclose(s * s, w, rtol=1e-15)
    e = rng.standard_normal((2, 3, 50))
    M0 = (rng.random((2, 3, 50)) > 0.3) * rng.random((2, 3, 50))
    meff, om, sigma = RO.mask64(e, M0, "huber", c=1e30)
    assert np.array_equal(om, np.ones_like(om)) and np.array_equal(meff, M0)       # huber with c = 1e30: omega = 1
    for b in range(2):
        assert sigma[b] == max(1.4826 * np.median(np.abs(e[b][M0[b] > 0])), RO.SIGMA_MIN)
    s32, n = RO.sigma32(e.astype(np.float32), M0)
    assert np.allclose(s32, sigma, rtol=1e-6) and np.array_equal(n, (M0 > 0).sum(axis=(1, 2)))
    # validity: a non-finite e keeps M0 and is not counted; no valid entry: sigma NaN, M_eff = M0
    e[0, 0, 0], e[0, 1, 1] = np.nan, np.inf
    meff, om, sigma = RO.mask64(e, np.ones_like(e), "tukey")
    assert meff[0, 0, 0] == 1.0 and meff[0, 1, 1] == 1.0 and om[0, 0, 0] == 1.0 and np.isfinite(sigma).all()
    meff, om, sigma = RO.mask64(e, np.zeros_like(e), "tukey")
    assert np.isnan(sigma).all() and not meff.any() and (om == 1.0).all()
    # per_pixel: the worst valid channel decides
    m, o, _ = RO.mask64(e[1:], None, "cauchy", per_pixel=True)
    own = RO.mask64(e[1:], None, "cauchy")[1]
    assert np.array_equal(o, np.broadcast_to(own.min(axis=1, keepdims=True), o.shape))


def test_torch_route_is_the_oracle():
    """`robust_weights_torch` (the autograd routes' M_eff, by torch.sort) against the oracle in float64, masks and non-finite entries
    included, and in float32 against `sigma32` bit for bit."""
    from osmosis_diffusion_code_amd.guided_diffusion.condition_methods import robust_weights_torch
    g = torch.Generator().manual_seed(1)
    e = 0.05 * torch.randn(3, 3, 7, 9, generator=g, dtype=torch.float64)
    e[:, :, 2, 3] = 0.8
    e[0, 0, 0, 0], e[1, 2, 1, 1] = float("nan"), float("inf")
    M0 = (torch.rand(3, 3, 7, 9, generator=g, dtype=torch.float64) > 0.3) * torch.rand(3, 3, 7, 9, generator=g, dtype=torch.float64)
    M0[2] = 0.0
    for loss in RO.LOSSES:
        for pp in (False, True):
            for scale in ("mad", 0.04):
                meff, om, sigma, n = robust_weights_torch(e, M0, loss, RO.C_DEFAULT[loss], scale, RO.SIGMA_MIN, pp)
                wm, wo, ws = RO.mask64(e.numpy().reshape(3, 3, -1), M0.numpy().reshape(3, 3, -1), loss, None, scale, RO.SIGMA_MIN, pp)
                assert np.allclose(meff.numpy().reshape(3, 3, -1), wm, rtol=0, atol=1e-15), (loss, pp, scale)
                assert np.allclose(om.numpy().reshape(3, 3, -1), wo, rtol=0, atol=1e-15)
                assert np.allclose(sigma.numpy(), ws, rtol=1e-15, equal_nan=True) and int(n[2]) == 0
    e32 = e.float()
    _, _, sigma, n = robust_weights_torch(e32, M0.float(), "tukey", 4.685)
    want, wn = RO.sigma32(e32.numpy().reshape(3, 3, -1), M0.float().numpy().reshape(3, 3, -1))
    assert np.array_equal(sigma.numpy()[:2].view(np.int32), want[:2].view(np.int32)) and np.isnan(sigma[2]) and np.array_equal(n.numpy(), wn)


# ------------------------------------------------------------------------------------------------------------ the effect, oracle alone
def test_effect_of_the_weights_on_the_oracle_alone():
    """36 x 34, J ~ U(0.1, 0.9), d ~ U(0.2, 1.5), phi* = (1.2, 0.6, 0.4 | 1.0, 0.7, 0.5 | 0.1, 0.5, 0.6), y = 2 I - 1 + N(0, 0.02), 5 %
    of the pixels replaced on all channels by U(0.6, 1.0); the image held at the truth, loss norm, sgd on phi from (0.8 | 0.8 | 0.3),
    20 iterations per sub-step, the weights renewed every sub-step.

    What is asserted, at two step sizes (1e-3 for 2400 sub-steps, 1.5e-3 for 1200): the huber and the tukey fit have SETTLED (max |phi -
    phi*| moves by less than 1e-4 over their last 200 sub-steps) and end at most 0.5 x the smallest error the least-squares fit shows
    at ANY cut of its trajectory -- the comparison most favourable to least squares, so the ratio does not depend on where a chain
    is cut.

    Why not a fixed 400 x 20 at one step: the ratio then measures speed, not the estimate.  max |phi - phi*| (float64, this seed):

        eta      sub-steps   least squares   huber    tukey    cauchy
        2e-3     400         0.2079          0.0991   0.0957   0.0664     (0.48 x / 0.46 x: inside 0.5 by luck of the cut)
        1e-3     400         0.2235          0.1572   0.1045   0.1247     (huber 0.70 x: not there yet)
        3e-3     400         0.2059          0.0590   0.1279   0.1197     (tukey 0.62 x: cycling, see below)
        1e-3     2400        0.2900          0.0374   0.0295   0.0308
        1.5e-3   1200        0.2099          0.0374   0.0353   0.0308
        5e-4     3200        0.2057          0.0374   0.0295   0.0308

    The least-squares fit never gets below 0.2057 at any cut and any of these steps: its error falls to 0.2057 on the way and then
    GROWS (0.29 at 2e-3 / 1200, 0.50 at 2e-3 / 3200) towards the biased optimum the outliers pull it to.  The robust fits settle at
    0.0374 (huber), 0.0295 (tukey), 0.0308 (cauchy) whatever the step, once it is small enough: 0.18 x, 0.14 x, 0.15 x of the
    least-squares fit's best cut.  The step matters for tukey: the norm loss's step length is eta / ||r||, and with hard rejection
    renewed every sub-step a fixed step that is too long lands in a cycle instead of the fixed point -- 0.0353 at 1.5e-3, 0.0957 at
    2e-3, 0.128 at 3e-3 (above the bound), and at 0.02 every fit diverges.  That is a property of fixed-step sgd on this loss, which
    the kernels reproduce (tests/test_robust_gpu.py), not of the weights.  sigma settles at 0.0213 next to the injected 0.02."""
    torch.set_num_threads(1)
    x0, y, out = RO.effect_problem()
    for rb in (None, dict(loss="huber"), dict(loss="tukey")):             # the closed form IS the autograd fit over the oracle's operator
        a, _, _ = RO.effect_fit(x0, y, rb, steps=30, eta=1.5e-3)
        b, _, _ = RO.effect_fit_closed_form(x0, y, rb, steps=30, eta=1.5e-3)
        assert max(float((a[k] - b[k]).abs().max()) for k in a) <= 1e-7, rb
    o = out.expand(1, 3, *out.shape[2:]).numpy().reshape(1, 3, -1)
    for eta, steps in ((1e-3, 2400), (1.5e-3, 1200)):
        tr, rec = {}, {}
        for tag, rb in (("ls", None), ("huber", dict(loss="huber")), ("tukey", dict(loss="tukey"))):
            tr[tag] = []
            _, om, sigma = RO.effect_fit_closed_form(x0, y, rb, steps=steps, eta=eta, trace=tr[tag])
            rec[tag] = None if om is None else (float(om[o].mean()), float(sigma[0]))
        best_ls = min(tr["ls"])
        print(f"ROBUSTEFFECT oracle eta {eta} x {steps}: least squares at its best cut {best_ls:.4f} (at its end {tr['ls'][-1]:.4f}), huber "
              f"{tr['huber'][-1]:.4f}, tukey {tr['tukey'][-1]:.4f}; (mean omega on the outliers, sigma) {rec}")
        for tag in ("huber", "tukey"):
            assert max(tr[tag][-200:]) - min(tr[tag][-200:]) < 1e-4, (eta, tag)                       # settled
            assert tr[tag][-1] <= 0.5 * best_ls, (eta, tag, tr[tag][-1], best_ls)
        assert rec["huber"][0] < 0.2 and rec["tukey"][0] < 0.1 and 0.015 < rec["huber"][1] < 0.03


# ------------------------------------------------------------------------------------------------------------ host-side refusals
def _cond(method="osmosis", opname="underwater_physical_revised", **okw):
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    if method == "ps":
        return CM.get_conditioning_method("ps", M.get_operator(opname, device="cpu", batch_size=1, **okw), M.get_noise("gaussian", sigma=0.0),
                                          scale="0.3")
    op = M.get_operator(opname, device="cpu", batch_size=1, depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95",
                        phi_b="0.95,0.8,0.8", phi_inf="0.14,0.29,0.49", **okw)
    return CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), loss_function="norm", loss_weight="none", scale="7,7,7,0.9",
                                      gradient_x_prev=True, gradient_clip="False,0", n_iter=2, pattern="pcgs")


def test_set_robust_validates_on_the_host_and_refuses_what_is_not_routed():
    from osmosis_diffusion_code_amd import sampling
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    cond = _cond()
    assert cond._robust is None and cond.robust_values() is None
    rb = cond.set_robust()
    assert (rb["loss"], rb["scale"], rb["per_pixel"]) == ("tukey", "mad", False) and abs(rb["c"] - 4.685) < 1e-6
    assert abs(rb["sigma_min"] - 2.0 / 255.0) < 1e-9 and abs(cond.set_robust("huber")["c"] - 1.345) < 1e-6
    assert abs(cond.set_robust("cauchy")["c"] - 2.385) < 1e-6 and cond.set_robust("huber", scale=0.05)["scale"] == pytest.approx(0.05)
    assert cond.set_robust(None) is None and cond._robust is None
    for bad in (dict(loss="l2"), dict(c=0.0), dict(c=-2.0), dict(scale="iqr"), dict(scale=0.0), dict(scale=float("nan")), dict(sigma_min=-0.1)):
        with pytest.raises(ValueError, match="robust"):
            cond.set_robust(**bad)
    assert cond._robust is None
    # the routings that are not built: a degradation inside the physical operator, a 'ps' grid operator (blind_blur included)
    deg = _cond(degradation=dict(name="gaussian_blur", kernel_size=5, intensity=1.0))
    with pytest.raises(NotImplementedError, match="robust"):
        deg.set_robust()
    deg._robust = cond.set_robust()                                               # (set behind its back: the routes refuse too)
    x0, y = torch.zeros(1, 4, 8, 8), torch.zeros(1, 3, 8, 8)
    with pytest.raises(NotImplementedError, match="robust"):
        deg.loss_grad_x0(x0, y)
    with pytest.raises(NotImplementedError, match="robust"):
        deg._loss_autograd(x0, y)
    for name, kw in (("gaussian_blur", dict(kernel_size=5, intensity=1.0)), ("blind_blur", dict(kernel_size=5))):
        ps = _cond("ps", name, **kw)
        with pytest.raises(NotImplementedError, match="robust"):
            ps.set_robust("huber")
        ps._robust = cond._robust
        with pytest.raises(NotImplementedError, match="robust"):
            ps.loss_grad_x0(torch.zeros(1, 3, 8, 8), y)
        with pytest.raises(NotImplementedError, match="robust"):
            ps.grad_and_value(x_prev=None, x_0_hat=torch.zeros(1, 3, 8, 8), measurement=y)
    # the torch route of the identity term runs on the CPU: the weighted norm
    ps = _cond("ps", "noise")
    ps.set_robust("tukey")
    g = torch.Generator().manual_seed(2)
    xp = torch.randn(1, 3, 8, 8, generator=g).requires_grad_(True)
    yy = (xp.detach() + 0.05 * torch.randn(1, 3, 8, 8, generator=g)).contiguous()
    yy[0, :, 3, 3] = xp.detach()[0, :, 3, 3] + 3.0
    grad, loss = ps.grad_and_value(x_prev=xp, x_0_hat=xp * 1.0, measurement=yy)
    e = (yy - xp.detach()).double().numpy().reshape(1, 3, -1)
    meff, om, sigma = RO.mask64(e, None, "tukey")
    assert abs(float(loss) - float(np.linalg.norm(meff * e))) <= 1e-5 * float(loss) and om.reshape(1, 3, 8, 8)[0, 0, 3, 3] == 0.0
    assert float(grad[0, 0, 3, 3]) == 0.0 and float(ps.robust_values()["scale"][0]) == pytest.approx(float(sigma[0]), rel=1e-5)
    ps.noiser = type("Poisson", (), {"__name__": "poisson"})()                     # the poisson data term is not weighted: refused
    with pytest.raises(NotImplementedError, match="robust"):
        ps.grad_and_value(x_prev=xp, x_0_hat=xp * 1.0, measurement=yy)
    # an iteration of the autograd route that raises leaves no held weights behind
    foreign = _cond()
    foreign.set_robust("huber")
    foreign.operator.optimize = lambda **kw: 1 / 0
    with pytest.raises(ZeroDivisionError):
        foreign._conditioning_autograd(xp4 := torch.zeros(1, 4, 8, 8, requires_grad=True), torch.zeros(1, 4, 8, 8), xp4 * 1.0, y)
    assert foreign._robust_hold is None and foreign._robust_holding is False
    # p_sample_loop(robust=) and the driver's config key: unknown keys raise before anything runs
    sampler = gd.get_sampler("ddpm")(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                     model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False,
                                     rescale_timesteps=False)
    kw = dict(model=None, x_start=x0, measurement=y, measurement_cond_fn=_cond().conditioning, record=False, save_root=None)
    with pytest.raises(ValueError, match="unknown keys"):
        sampler.p_sample_loop(robust=dict(loss="tukey", k=4.0), **kw)
    with pytest.raises(ValueError, match="robust"):
        sampler.p_sample_loop(robust=dict(loss="welsch"), **kw)
    with pytest.raises(TypeError, match="set_robust"):
        sampler.p_sample_loop(robust=dict(loss="tukey"), **dict(kw, measurement_cond_fn=lambda **k: None))
    assert sampling.robust_config(None, None) is None and sampling.robust_config({}, None) is None
    assert sampling.robust_config(dict(loss="huber"), dict(loss="tukey", c=3.0)) == dict(loss="tukey", c=3.0)     # the argument wins
    with pytest.raises(ValueError, match="unknown key"):
        sampling.robust_config(dict(loss="huber", weight=1.0), None)
    with pytest.raises(ValueError, match="mapping"):
        sampling.robust_config("tukey", None)
