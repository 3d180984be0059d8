"""The range-map depth prior, host side (no GPU): the oracle's own checks (tests/depthprior_oracle.py), the seventh header of the C
ABI against the library and `_lib.exports("osmosis_depthprior.h")`, the argument checks of the entry points (they return before a launch),
`set_depth_prior` and its errors, and the autograd route against the oracle."""
import ctypes
import os

import numpy as np
import pytest
import torch

import depthprior_oracle as DO
from oracle import diffusion_ref as D
from osmosis_diffusion_code_amd import _lib
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"osm_depth_nblk", "osm_depth_reduce", "osm_depth_fit", "osm_depth_grad", "osm_depth_loss_grad"}
OKW = dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8", phi_inf="0.14, 0.29, 0.49")


def small_problem(seed=0, slope=0.7):
    """8 x 6 with 11 valid pixels, float64."""
    g = torch.Generator().manual_seed(seed)
    z = torch.rand(1, 1, 8, 6, generator=g, dtype=torch.float64) * 3 + 0.5
    d = slope * z + 0.3 + 0.1 * torch.randn(1, 1, 8, 6, generator=g, dtype=torch.float64)
    m = torch.zeros(48, dtype=torch.float64)
    m[torch.randperm(48, generator=g)[:11]] = torch.rand(11, generator=g, dtype=torch.float64) * 0.9 + 0.1
    m = m.reshape(1, 1, 8, 6)
    assert int((m > 0).sum()) == 11
    return d, z, m


def test_closed_form_fit_is_the_weighted_least_squares_solution():
    d, z, m = small_problem()
    on = (m > 0).reshape(-1)
    dv, zv, mv = d.reshape(-1)[on], z.reshape(-1)[on], m.reshape(-1)[on]
    a, c = DO.fit(dv, zv, mv, "affine")
    w = mv.sqrt()
    sol = torch.linalg.lstsq(torch.stack([zv, torch.ones_like(zv)], dim=1) * w[:, None], (dv * w)[:, None]).solution.reshape(-1)
    assert abs(float(a) - float(sol[0])) <= 1e-12 * abs(float(sol[0])) and abs(float(c) - float(sol[1])) <= 1e-12 * abs(float(sol[1]))
    a1, c1 = DO.fit(dv, zv, mv, "scale")
    sol1 = torch.linalg.lstsq((zv * w)[:, None], (dv * w)[:, None]).solution.reshape(-1)
    assert abs(float(a1) - float(sol1[0])) <= 1e-12 * abs(float(sol1[0])) and float(c1) == 0.0
    a0, c0 = DO.fit(dv, zv, mv, "none", scale=0.4)
    assert float(a0) == 0.4 and float(c0) == 0.0
    # the guards: no valid pixel, z = 0 under scale, a constant range map under affine
    assert DO.fit(dv, zv, torch.zeros_like(mv), "affine") is None
    assert DO.fit(dv, torch.zeros_like(zv), mv, "scale") is None
    assert DO.fit(dv, torch.full_like(zv, 2.5), mv, "affine") is None


@pytest.mark.parametrize("loss", ["norm", "mse"])
@pytest.mark.parametrize("case", ["affine", "scale", "none", "bound"])
def test_envelope_gradient_equals_autograd_through_the_solve(case, loss):
    """(a, c) minimise S (or a sits on scale_min and c minimises): the gradient with them held constant IS the gradient.  For `none`
    there is nothing to solve; `bound`: a negative raw slope, a == scale_min."""
    d, z, m = small_problem(seed=3, slope=-0.5 if case == "bound" else 0.7)
    align = "affine" if case == "bound" else case
    grads = []
    for envelope in (True, False):
        dd = d.clone().requires_grad_(True)
        L, info = DO.term(dd, z, m, align, loss, scale=0.9, scale_min=1e-3, envelope=envelope)
        (g,) = torch.autograd.grad(L.sum(), dd)
        grads.append(g)
        if case == "bound":
            assert info[0]["a"] == 1e-3
            on = m > 0                                              # c re-solved with a on its bound
            assert info[0]["c"] == pytest.approx(float((m * (dd.detach() - 1e-3 * z))[on].sum() / m[on].sum()), rel=1e-12)
        assert not info[0]["skipped"] and float(L.detach()) > 0
    assert float((grads[0] - grads[1]).abs().max()) <= 1e-10 * float(grads[1].abs().max())
    assert float(grads[0][m == 0].abs().max()) == 0.0 and float(grads[0].abs().max()) > 0


def test_oracle_guards():
    d, z, m = small_problem(seed=5)
    L, info = DO.term(d, z, torch.zeros_like(m), "affine", "norm")
    assert float(L) == 0.0 and info[0]["skipped"] and np.isnan(info[0]["a"])
    L, info = DO.term(d, torch.full_like(z, 2.0), m, "affine", "mse")
    assert float(L) == 0.0 and info[0]["skipped"]
    L, info = DO.term(d, torch.zeros_like(z), m, "scale", "mse")
    assert float(L) == 0.0 and info[0]["skipped"]
    bad = d.clone()
    bad.reshape(-1)[int(torch.nonzero((m > 0).reshape(-1))[0])] = float("nan")
    L, info = DO.term(bad, z, m, "affine", "norm")
    assert np.isnan(float(L)) and info[0]["nan"]
    L, info = DO.term(0.75 * z + 0.125, z, m, "affine", "norm")            # a perfect fit
    assert float(L) == 0.0 and not info[0]["skipped"] and info[0]["a"] == pytest.approx(0.75, rel=1e-9)
    zn = torch.where(m > 0, z, torch.full_like(z, float("nan")))           # z where m = 0 is never read
    assert torch.equal(DO.term(d, zn, m, "affine", "norm")[0], DO.term(d, z, m, "affine", "norm")[0])


def test_header_exports_and_bindings_agree():
    assert set(_lib.exports("osmosis_depthprior.h")) == NAMES
    for other in ("osmosis_hip.h", "osmosis_linop.h", "osmosis_psf.h", "osmosis_physlin.h", "osmosis_physgroup.h", "osmosis_blind.h"):
        assert "osm_depth" not in open(os.path.join(ROOT, "include", other)).read(), other
    mk = open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "Makefile")).read()
    assert "depthprior.hip" in mk and "osmosis_depthprior.h" in mk and "depth_conv.h" in mk
    src = os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc")
    assert "conv_depth(float D" not in open(os.path.join(src, "guidance.hip")).read()        # ONE definition, in the shared header
    assert '#include "depth_conv.h"' in open(os.path.join(src, "guidance.hip")).read()
    assert '#include "depth_conv.h"' in open(os.path.join(src, "depthprior.hip")).read()
    from osmosis_diffusion_code_amd import ops, torch_ops
    assert ops.depth_nblk(36 * 34) == 2 and ops.depth_nblk(1024) == 1 and ops.depth_nblk(74 * 58) == 5 == ops.phys_nblk(74 * 58)
    assert "depth_prior_loss_grad" in torch_ops.OPS and "depth_prior_loss_grad" not in torch_ops.OPS_C
    schema = str(torch.ops.osmosis.depth_prior_loss_grad.default._schema)
    assert "Tensor(a3!) g" in schema and schema.count("!") == 1 and schema.endswith("-> (Tensor, Tensor)"), schema
    for doc in ("INTEGRATION.md", "README.md"):
        assert "osmosis_depthprior.h" in open(os.path.join(ROOT, doc)).read(), doc


def test_entry_points_refuse_bad_arguments_before_any_launch():
    lib = _lib.load()
    p = 4096                                                                               # never dereferenced on the host

    def desc(**kw):
        d = _lib.DepthDesc()
        d.align, d.loss_type, d.lam, d.scale, d.scale_min, d.depth_type, d.B, d.HW = 2, 0, 0.5, 1.0, 1e-3, 0, 2, 48
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)
    bad_desc = [(dict(align=3), "align"), (dict(align=-1), "align"), (dict(loss_type=2), "loss_type"), (dict(depth_type=3), "depth_type"),
                (dict(lam=-0.1), "lambda"), (dict(lam=float("nan")), "lambda"), (dict(lam=float("inf")), "lambda"),
                (dict(scale=float("nan")), "scale"), (dict(scale_min=0.0), "scale_min"), (dict(scale_min=-1.0), "scale_min"),
                (dict(B=0), "shape"), (dict(HW=0), "shape"), (dict(HW=-4), "shape")]
    # (descriptor), then the pointers of each entry point, then the stream
    entries = {"osm_depth_reduce": 4, "osm_depth_fit": 3, "osm_depth_grad": 5, "osm_depth_loss_grad": 7}
    for fn, nptr in entries.items():
        f = getattr(lib, fn)
        for kw, word in bad_desc:
            rc = f(desc(**kw), *([p] * nptr), None)
            msg = lib.osm_last_error().decode()
            assert rc != 0 and msg.startswith(fn + ":") and word in msg, (fn, kw, rc, msg)
        rc = f(None, *([p] * nptr), None)
        assert rc != 0 and "null" in lib.osm_last_error().decode()
        for pos in range(nptr):
            args = [p] * nptr
            args[pos] = None
            rc = f(desc(), *args, None)
            msg = lib.osm_last_error().decode()
            assert rc != 0 and msg.startswith(fn + ":") and "null" in msg, (fn, pos, rc, msg)
    assert lib.osm_depth_nblk(0) == 0 and lib.osm_depth_nblk(1) == 1 and lib.osm_depth_nblk(1025) == 2


def _cond(method="osmosis", **okw):
    op = M.get_operator("underwater_physical_revised", device="cpu", **dict(OKW, **okw))
    return CM.get_conditioning_method(method, op, M.get_noise("clean"), gradient_x_prev=True, loss_function="norm", loss_weight="none")


def test_set_depth_prior_shapes_ranges_and_grid():
    cond = _cond()
    assert cond._depth is None and cond.depth_prior_values() is None and cond.depth_prior_rows(2, 8, 6, "cpu") is None
    z = torch.rand(2, 1, 8, 6) + 0.5
    dp = cond.set_depth_prior(z, weight=0.3, align="scale", loss="mse", batch=2)
    assert dp["z"].shape == (2, 1, 48) and dp["m"].shape == (2, 1, 48) and dp["z"].is_contiguous() and dp["m"].dtype == torch.float32
    assert torch.equal(dp["m"], torch.ones(2, 1, 48)) and (dp["weight"], dp["align"], dp["loss"]) == (0.3, "scale", "mse")
    vals = cond.depth_prior_values()                                                       # per batch, undefined before a guided sub-step
    assert set(vals) == {"loss", "scale", "shift"} and all(tuple(v.shape) == (2,) and bool(torch.isnan(v).all()) for v in vals.values())
    zr, mr = cond.depth_prior_rows(2, 8, 6, "cpu")
    x0, y = torch.zeros(2, 4, 8, 6), torch.zeros(2, 3, 8, 6)
    with pytest.raises(ValueError, match="open_batch"):                                    # a chunk's place is its range of the OPEN batch
        cond._batch_rows((0, 2), x0, y)
    cond.open_batch(2, (8, 6), (8, 6), "cpu")
    assert cond._batch_rows((0, 2), x0, y) == (0, 2) and cond._batch_rows((1, 2), x0[1:2], y[1:2]) == (1, 2)
    assert cond._batch_rows(None, x0, y) == (0, 2) and cond._depth["z"].data_ptr() == zr.data_ptr()
    with pytest.raises(ValueError, match="rows must be"):
        cond._batch_rows((1, 2), x0, y)                                                    # one row for two images
    with pytest.raises(ValueError, match="rows must be"):
        cond._batch_rows((1, 3), x0, y)                                                    # past the prior's rows
    assert cond.set_depth_prior(z[:, 0])["z"].shape == (2, 1, 48)                          # [B,H,W]
    assert cond.set_depth_prior(z[:1], batch=3)["z"].shape == (3, 1, 48)                   # [1,1,H,W] broadcasts
    zr, mr = cond.depth_prior_rows(3, 8, 6, "cpu")
    assert zr.shape == mr.shape == (3, 1, 48)
    with pytest.raises(ValueError, match="does not fit"):
        cond.depth_prior_rows(3, 6, 8, "cpu")
    with pytest.raises(ValueError, match="does not fit"):
        cond.depth_prior_rows(2, 8, 6, "cpu")
    # invalid range becomes m = 0 and z = 0, whatever confidence says
    zz = z.clone()
    zz[0, 0, 0, 0], zz[0, 0, 1, 1], zz[1, 0, 2, 2], zz[1, 0, 3, 3] = float("nan"), float("inf"), 0.0, -2.0
    conf = torch.rand(2, 1, 8, 6) * 0.5 + 0.5
    conf[0, 0, 4, 4] = 0.0
    dp = cond.set_depth_prior(zz, confidence=conf)
    m, zs = dp["m"].view(2, 8, 6), dp["z"].view(2, 8, 6)
    for b, i, j in ((0, 0, 0), (0, 1, 1), (1, 2, 2), (1, 3, 3), (0, 4, 4)):
        assert m[b, i, j] == 0 and zs[b, i, j] == 0
    assert int((m == 0).sum()) == 5 and bool(torch.isfinite(zs).all()) and torch.equal(m[m > 0], conf.view(2, 8, 6)[m > 0])
    for bad, word in ((torch.rand(2, 3, 8, 6), "must be"), (torch.rand(8, 6), "must be"), (torch.rand(2, 1, 8, 6, 1), "must be")):
        with pytest.raises(ValueError, match=word):
            cond.set_depth_prior(bad)
    with pytest.raises(ValueError, match="batch"):
        cond.set_depth_prior(z, batch=3)
    with pytest.raises(ValueError, match="shape of the depth prior"):
        cond.set_depth_prior(z, confidence=torch.rand(2, 1, 6, 8))
    with pytest.raises(ValueError, match=r"\[0, 1\]"):
        cond.set_depth_prior(z, confidence=torch.full((2, 1, 8, 6), 1.5))
    with pytest.raises(ValueError, match="finite"):
        cond.set_depth_prior(z, confidence=torch.full((2, 1, 8, 6), float("nan")))
    for kw, word in ((dict(align="log"), "align"), (dict(loss="huber"), "loss"), (dict(weight=-1.0), "weight"),
                     (dict(weight=float("nan")), "weight"), (dict(scale_min=0.0), "scale_min"), (dict(scale=float("inf")), "scale")):
        with pytest.raises(ValueError, match=word):
            cond.set_depth_prior(z, **kw)
    assert cond.set_depth_prior(None) is None and cond._depth is None
    # the 'ps' branch has no depth model
    ps = CM.get_conditioning_method("ps", M.get_operator("noise", device="cpu"), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="depth model"):
        ps.set_depth_prior(z)
    assert ps.set_depth_prior(None) is None


class Foreign:
    """An image-formation model the kernels do not know (no fill_desc): the autograd route's case.  Depth conversion: 'original'."""
    depth_type, value = "original", None

    def forward(self, data, **kw):
        d = 0.5 * (data[:, 3:4] + 1.0)
        return 0.5 * (data[:, 0:3] + 1.0) * torch.exp(-0.8 * d) + 0.2 * (1 - torch.exp(-0.8 * d))


class ForeignGamma(Foreign):
    """The same model with the kernels' gamma conversion ((D + 1.4) 0.9)^1.3 declared the way the package's operators declare it."""
    depth_type, value, depth_code, depth_vals = "gamma", np.array([1.4, 0.9, 1.3]), 1, (1.4, 0.9, 1.3)


class ForeignGammaLinear(Foreign):
    depth_type, value, depth_code, depth_vals = "gamma", np.array([1.4, 1.4, 1.0]), 1, (1.4, 1.4, 1.0)       # v2 = 1: no pow


class ForeignMove(Foreign):
    depth_type, value, depth_code, depth_vals = "move", 0.7, 2, (0.7, 1.0, 1.0)


@pytest.mark.parametrize("opcls", [Foreign, ForeignGamma, ForeignGammaLinear, ForeignMove])
@pytest.mark.parametrize("align,loss", [("affine", "norm"), ("scale", "mse"), ("none", "norm")])
def test_loss_autograd_with_a_prior_is_the_oracles_objective(align, loss, opcls):
    """`_loss_autograd` on a foreign operator, float32, against the float64 oracle: the total and d total / d x0 to 1e-5 (the
    autograd route's bar); the reported per-image loss stays the data loss."""
    H, W = 12, 10
    x0, z, m = DO.problem(2, H, W, seed=7, frac=0.4, fractional=True)
    y = torch.rand(2, 3, H, W, generator=torch.Generator().manual_seed(1)) * 1.6 - 0.8
    op = opcls()
    cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), gradient_x_prev=True, loss_function="mse", loss_weight="none")
    assert not cond._has_kernels()
    xa = x0.clone().requires_grad_(True)
    sep0, loss0, _ = cond._loss_autograd(xa, y)
    cond.set_depth_prior(z, confidence=m, weight=0.7, align=align, loss=loss, scale=0.2)
    sep, total, _ = cond._loss_autograd(xa, y)
    (ga,) = torch.autograd.grad(total, xa)
    assert np.array_equal(sep, sep0)
    xb = x0.double().requires_grad_(True)
    Ld, info = DO.term(D.convert_depth(xb[:, 3:4], op.depth_type, op.value), z.double(), m.double(), align, loss, scale=0.2)
    data = (((y.double() - (2 * op.forward(xb) - 1)) ** 2).mean(dim=(1, 2, 3))).sum()
    want = data + 0.7 * Ld.sum()
    (gb,) = torch.autograd.grad(want, xb)
    assert abs(float(loss0.detach()) - float(data.detach())) <= 1e-5 * float(data.detach())
    assert abs(float(total.detach()) - float(want.detach())) <= 1e-5 * abs(float(want.detach()))
    assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())
    assert float((ga - torch.autograd.grad(loss0, xa)[0])[:, 0:3].abs().max()) == 0.0       # the colour planes are the data term's
    vals = cond.depth_prior_values()
    assert np.allclose(vals["loss"].numpy(), Ld.detach().numpy(), rtol=1e-5)
    assert np.allclose(vals["scale"].numpy(), [i["a"] for i in info], rtol=1e-4)
    assert np.allclose(vals["shift"].numpy(), [i["c"] for i in info], rtol=1e-4, atol=1e-6)
    assert float(Ld.detach().min()) > 0 and all(not i["skipped"] for i in info)


# ------------------------------------------------------------------------------------------------------------ data and driver
def test_transform_range_is_hole_aware():
    from osmosis_diffusion_code_amd.osmosis_utils import data as datao
    # a fully valid constant map stays constant
    z, m = datao.transform_range(torch.full((96, 128), 3.25), size=32)
    assert z.shape == m.shape == (1, 1, 32, 32) and float((z - 3.25).abs().max()) <= 1e-6 and torch.equal(m, torch.ones_like(m))
    # a hole keeps the range beside it: no bleed towards 0
    full = torch.full((96, 128), 3.25)
    full[30:60, 40:90] = float("nan")
    full[0:10, :] = -1.0
    z, m = datao.transform_range(full, size=32)
    assert float(z[m > 0].min()) >= 3.25 - 1e-5 and float(z[m > 0].max()) <= 3.25 + 1e-5
    assert int((m == 0).sum()) > 0 and float(z[m == 0].abs().max()) == 0.0 and bool(torch.isfinite(z).all())
    zc, mc = datao.transform_range(full, confidence=torch.full((96, 128), 0.5), size=32)
    assert torch.equal(zc, z) and float(mc.max()) <= 0.5 and torch.equal(mc > 0, m > 0)
    # min_cover: a pixel whose footprint is mostly hole is dropped
    loose = datao.transform_range(full, size=32, min_cover=0.05)[1]
    assert int((loose > 0).sum()) > int((m > 0).sum())
    # geometries: the center crop and the `fit` grid
    assert datao.transform_range(torch.ones(96, 128), size=32)[0].shape == (1, 1, 32, 32)
    geo = datao.transform_geometry(96, 128, 64, "fit", 32)
    zf, mf = datao.transform_range(torch.ones(1, 96, 128), geometry=geo)
    assert zf.shape == mf.shape == (1, 1, geo.h, geo.w) == (1, 1, 64, 64)
    ramp = torch.linspace(1, 5, 200)[None, :].expand(96, 200).contiguous()                 # a geometry carries its own resize
    geo2 = datao.transform_geometry(96, 200, 64, "fit", 32)
    assert torch.equal(datao.transform_range(ramp, geometry=geo2)[0], datao.transform_range(ramp, size=64, crop="fit")[0])
    assert datao.transform_range(torch.ones(96, 200), size=64, crop="fit")[0].shape == (1, 1, 64, 128)
    with pytest.raises(ValueError, match="geometry"):
        datao.transform_range(torch.ones(90, 128), geometry=geo)
    with pytest.raises(ValueError, match="range map must be"):
        datao.transform_range(torch.ones(3, 96, 128))
    with pytest.raises(ValueError, match="confidence"):
        datao.transform_range(torch.ones(96, 128), confidence=torch.full((96, 128), 2.0))


def test_config_key_and_result_keys():
    from osmosis_diffusion_code_amd import sampling
    params, path = sampling.depth_prior_config(dict(weight="0.5", align="scale", loss="mse", scale=2, scale_min=0.01, path="r.npy"))
    assert params == dict(weight=0.5, align="scale", loss="mse", scale=2.0, scale_min=0.01) and path == "r.npy"
    assert sampling.depth_prior_config(None) == ({}, None)
    with pytest.raises(ValueError, match="unknown key"):
        sampling.depth_prior_config(dict(weight=1.0, huber=0.1))
    assert sampling.depth_prior_inputs((8, 6)) is None
    with pytest.raises(ValueError, match="comes with a range map"):
        sampling.depth_prior_inputs((8, 6), depth_confidence=torch.ones(1, 1, 8, 6))
    with pytest.raises(ValueError, match="image grid"):
        sampling.depth_prior_inputs((8, 6), depth=torch.ones(1, 1, 6, 8))
    got = sampling.depth_prior_inputs((8, 6), dict(weight=0.5), depth=torch.ones(1, 1, 8, 6))
    assert got["weight"] == 0.5 and got["confidence"] is None and "align" not in got
    # postprocess-level outputs from a hand-made fit: depth_metric inverts a z + c exactly
    H, W = 8, 6
    g = torch.Generator().manual_seed(2)
    z = (torch.rand(H, W, generator=g) * 4 + 1).double()
    a, c = 0.25, 0.125
    depth_calc = (a * z + c).float()[None].repeat(3, 1, 1)
    phi = {"phi_a": torch.tensor([[1.1, 0.9, 0.8]]).view(1, 3, 1, 1), "phi_b": torch.tensor([[0.9, 0.8, 0.7]]).view(1, 3, 1, 1),
           "phi_inf": torch.tensor([[0.1, 0.3, 0.5]]).view(1, 3, 1, 1)}
    m = torch.ones(H, W)
    post = sampling.attach_depth_prior(dict(depth_calc=depth_calc, phi=phi), z.float(), m, a, c, 0.75, "affine")
    assert {"depth_prior", "depth_confidence", "depth_scale", "depth_shift", "depth_loss_final", "depth_metric"} <= set(post)
    assert "phi_metric" not in post and post["depth_loss_final"] == 0.75
    assert float((post["depth_metric"].double() - (depth_calc[0].double() - c) / a).abs().max()) == 0.0
    assert float((post["depth_metric"].double() - z).abs().max()) <= 1e-6 * 5
    for align in ("scale", "none"):
        post = sampling.attach_depth_prior(dict(depth_calc=depth_calc, phi=phi), z.float(), m, a, 0.0, 0.75, align)
        assert torch.equal(post["phi_metric"]["phi_a"], phi["phi_a"] * a) and torch.equal(post["phi_metric"]["phi_b"], phi["phi_b"] * a)
        assert torch.equal(post["phi_metric"]["phi_inf"], phi["phi_inf"])
    skipped = sampling.attach_depth_prior(dict(depth_calc=depth_calc, phi=phi), z.float(), 0 * m, float("nan"), float("nan"), 0.0, "scale")
    assert bool(torch.isnan(skipped["depth_metric"]).all()) and "phi_metric" not in skipped
    post = sampling.attach_depth_prior(dict(depth_calc=depth_calc, phi=phi), z.float(), m, a, c, 0.75, "affine")
    metric_u8, prior_u8 = sampling.depth_metric_images_u8(post)
    assert metric_u8.shape == prior_u8.shape == (H, W, 3) and metric_u8.dtype == np.uint8
    assert int(np.abs(metric_u8.astype(int) - prior_u8.astype(int)).max()) <= 1            # one normalisation: equal ranges, equal colours


def test_p_sample_loop_refuses_a_bad_depth_prior_before_anything_runs():
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    sampler = gd.get_sampler("ddpm")(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000),
                                     model_mean_type="epsilon", model_var_type="learned_range", dynamic_threshold=False,
                                     clip_denoised=False, rescale_timesteps=False)
    cond = _cond()
    x, y = torch.zeros(1, 4, 8, 6), torch.zeros(1, 3, 8, 6)
    kw = dict(model=None, x_start=x, measurement=y, measurement_cond_fn=cond.conditioning, record=False, save_root=None)
    with pytest.raises(ValueError, match="unknown keys"):
        sampler.p_sample_loop(depth_prior=dict(z=torch.ones(1, 1, 8, 6), huber=1.0), **kw)
    with pytest.raises(ValueError, match="image grid"):
        sampler.p_sample_loop(depth_prior=dict(z=torch.ones(1, 1, 6, 8)), **kw)
    with pytest.raises(ValueError, match="range map"):
        sampler.p_sample_loop(depth_prior=dict(weight=1.0), **kw)
    with pytest.raises(TypeError, match="set_depth_prior"):
        sampler.p_sample_loop(depth_prior=dict(z=torch.ones(1, 1, 8, 6)), **dict(kw, measurement_cond_fn=lambda **k: None))
    ps = CM.get_conditioning_method("ps", M.get_operator("noise", device="cpu"), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="depth model"):
        sampler.p_sample_loop(depth_prior=dict(z=torch.ones(1, 1, 8, 6)), **dict(kw, measurement_cond_fn=ps.conditioning))


@pytest.mark.skipif(__import__("shutil").which("gcc") is None, reason="no gcc")
def test_depthprior_header_is_strict_c99(tmp_path):
    import subprocess
    src = tmp_path / "use.c"
    src.write_text('#include "osmosis_depthprior.h"\nint main(void) {\n  osm_depth_desc d;\n'
                   '  int (*f)(const osm_depth_desc*, const float*, const float*, const float*, double*, double*, float*, float*, void*) = '
                   'osm_depth_loss_grad;\n'
                   '  d.align = 2;\n  d.loss_type = 0;\n  d.lambda = 1.0f;\n  d.scale = 1.0f;\n  d.scale_min = 0.001f;\n  d.depth_type = 1;\n'
                   '  d.dval[2] = 1.0f;\n  d.B = 1;\n  d.HW = 48;\n  return d.align - 2 + (f ? 0 : 1);\n}\n')
    subprocess.run(["gcc", "-std=c99", "-pedantic", "-Werror", "-Wall", "-I", os.path.join(ROOT, "include"), "-c", str(src), "-o",
                    str(tmp_path / "use.o")], check=True)


def test_torch_term_reports_nan_for_a_poisoned_image_and_keeps_it_out_of_the_objective():
    """A NaN in the depth plane of a valid pixel: the reported loss of that image is NaN (as the kernels and the oracle report it),
    the objective and its gradient are those of the other image alone."""
    H, W = 8, 6
    x0, z, m = DO.problem(2, H, W, seed=9, frac=0.6)
    z = torch.where(m > 0, z, torch.zeros_like(z))
    bad = x0.clone()
    bad[0, 3].reshape(-1)[int(torch.nonzero(m[0].reshape(-1) > 0)[0])] = float("nan")
    d = 0.5 * (bad[:, 3:4].double() + 1.0)
    d.requires_grad_(True)
    L, reported, a, c = CM.depth_prior_term(d, z.double(), m.double(), "affine", "norm")
    assert float(L[0]) == 0.0 and np.isnan(float(reported[0])) and np.isnan(float(a[0])) and np.isnan(float(c[0]))
    want, info = DO.term(d.detach(), z.double(), m.double(), "affine", "norm")
    assert info[0]["nan"] and np.isnan(float(want[0])) and float(reported[1]) == pytest.approx(float(want[1]), rel=1e-12)
    (g,) = torch.autograd.grad(L.sum(), d)
    assert float(g[0].abs().max()) == 0.0 and bool(torch.isfinite(g).all()) and float(g[1].abs().max()) > 0
    cond = CM.get_conditioning_method("osmosis", Foreign(), M.get_noise("clean"), gradient_x_prev=True, loss_function="mse", loss_weight="none")
    cond.set_depth_prior(z, confidence=m, weight=0.5)
    cond._depth_autograd(bad)
    vals = cond.depth_prior_values()
    assert np.isnan(float(vals["loss"][0])) and float(vals["loss"][1]) == pytest.approx(float(want[1]), rel=1e-5)


def test_range_map_file_goes_through_the_photos_geometry(tmp_path):
    from osmosis_diffusion_code_amd import sampling
    from osmosis_diffusion_code_amd.osmosis_utils import data as datao
    full = torch.rand(96, 200, generator=torch.Generator().manual_seed(4)) * 3 + 1
    np.save(str(tmp_path / "r.npy"), full.numpy())
    geo = datao.transform_geometry(96, 200, 64, "fit", 32)
    got = sampling.depth_prior_inputs((geo.h, geo.w), dict(path=str(tmp_path / "r.npy"), weight=2.0), geometry=geo)
    want_z, want_m = datao.transform_range(full, geometry=geo)
    assert torch.equal(got["z"], want_z) and torch.equal(got["confidence"], want_m) and got["weight"] == 2.0
    guessed = sampling.depth_prior_inputs((geo.h, geo.w), dict(path=str(tmp_path / "r.npy")))            # the default transform for the grid
    assert torch.equal(guessed["z"], want_z)
    with pytest.raises(ValueError, match="geometry"):
        sampling.depth_prior_inputs((64, 64), dict(path=str(tmp_path / "r.npy")), geometry=datao.transform_geometry(90, 200, 64, "fit", 32))
