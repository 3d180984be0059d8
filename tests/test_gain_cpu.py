"""The learnt vignetting gain field without a GPU (include/osmosis_gain.h): the tenth header against the library and
`_lib.exports("osmosis_gain.h")`, the host refusals, the identity the design rests on, the oracle's self-checks (tests/gain_oracle.py), the effect
of the field on the oracle alone, and the torch route against the oracle."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

import gain_oracle as GA
import physgroup_oracle as GO
from oracle import diffusion_ref as D
from osmosis_diffusion_code_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"osm_gain_expand", "osm_gain_rows", "osm_gain_step", "osm_gain_prepare"}
OPS = {"underwater_physical_revised": dict(depth_type="gamma", value="1.4,1.4,1", phi_a="1.1,0.95,0.95", phi_b="0.95, 0.8, 0.8",
                                           phi_inf="0.14, 0.29, 0.49"),
       "underwater_physical": dict(depth_type="original", value="1.4,1.4,1", phi_ab="1.1,0.95,0.95", phi_inf="0.2,0.4,0.7"),
       "haze_physical": dict(depth_type="gamma", value="1.4,1.4,1", phi_ab="0.9", phi_inf="0.8,0.8,0.85")}
AUX = {"avrg_loss": 0.5, "val_loss": 20}


def etas(okw, value):
    return {k + "_eta": value for k in ("phi_a", "phi_b", "phi_ab", "phi_inf") if k in okw}


# ------------------------------------------------------------------------------------------------------------ header and bindings
def test_header_exports_and_bindings_agree():
    hdr = open(os.path.join(ROOT, "include", "osmosis_gain.h")).read()
    body = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert set(_lib.exports("osmosis_gain.h")) == NAMES
    assert '#include "osmosis_hip.h"' in body
    for rule in ("The reference has no such term", "G = b top + fy bot", "never an fma", "(y_c + 1) / G - 1", "max n = 1", "g_min > 0",
                 "S = 0 under the norm loss", "max(u) not finite", "2 / (3 HW)", "1 / sqrt(S)", "ascending x", "ascending y", "2^-23"):
        assert rule in hdr, rule                                                  # the contract is stated in the header
    assert "osm_gain" not in open(os.path.join(ROOT, "include", "osmosis_hip.h")).read()      # the main header is what it was
    mk = open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "Makefile")).read()
    assert "osmosis_gain.h" in mk and "gainfield.hip" in mk and "-ffp-contract=off" in mk
    src = open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "gainfield.hip")).read()
    assert "#pragma clang fp contract(off)" in src and "atomicAdd" not in src
    from osmosis_diffusion_code_amd import ops, torch_ops
    assert all(callable(getattr(ops, n)) for n in ("gain_expand", "gain_rows", "gain_step", "gain_prepare", "gain_desc", "gain_tables"))
    assert "gain_prepare" in torch_ops.OPS and "gain_prepare" not in torch_ops.OPS_C
    schema = str(torch.ops.osmosis.gain_prepare.default._schema)
    for arg in ("nodes", "y_eff", "m_eff", "field", "t", "s", "cs"):
        assert re.search(r"Tensor\(a\d+!\) " + arg + r"\b", schema), schema
    assert schema.count("!") == 7 and schema.endswith("-> ()"), schema
    for doc in ("INTEGRATION.md", "README.md", "DESIGN.md"):
        assert "osmosis_gain.h" in open(os.path.join(ROOT, doc)).read(), doc
    papers = open(os.path.join(ROOT, "PAPERS.md")).read()
    assert "Goldman" in papers and "cos" in papers
    total = sum(len(_lib.ABI[h]) for h in list(_lib.ABI)[:10])                    # the ten headers up to this one
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert total == 129 and "the library's 125 exports" in readme and f"{total} exports" in readme


def test_tables_are_the_oracles_and_the_field_is_align_corners_bilinear():
    from osmosis_diffusion_code_amd import ops
    g = torch.Generator().manual_seed(0)
    for H, W, gh, gw in ((36, 34, 5, 5), (74, 58, 3, 7), (8, 12, 5, 5), (5, 7, 2, 2), (36, 34, 32, 32), (33, 33, 5, 5), (17, 25, 3, 4)):
        tabs = GA.tables(H, W, gh, gw)
        for a, b in zip(tabs, ops.gain_tables_host(H, W, gh, gw)):
            assert a.dtype == b.dtype and np.array_equal(a, b)
        iy0, fy, ix0, fx = tabs
        assert iy0.min() == 0 and iy0.max() == gh - 2 and ix0.max() == gw - 2 and fy[0] == 0 and fy[-1] == 1 and fx[-1] == 1
        assert (np.diff(iy0) >= 0).all() and (np.diff(ix0) >= 0).all() and 0 <= fx.min() and fx.max() <= 1
        n = torch.rand(2, gh, gw, generator=g, dtype=torch.float64) + 0.1
        G = GA.field64(n, tabs)
        ref = Fn.interpolate(n[:, None], size=(H, W), mode="bilinear", align_corners=True)
        # where the fractions are exact in fp32 (node spacing a power of two) the tables round nothing: 1e-12; elsewhere the fp32
        # rounding of a fraction (<= 2^-25 of a cell, twice per pixel) times the largest node difference is the distance
        exact = (H, W, gh, gw) in ((33, 33, 5, 5), (17, 25, 3, 4))
        bar = 1e-12 if exact else 2.0 ** -23 * float(n.max() - n.min())
        assert float((G - ref).abs().max()) <= bar, (H, W, gh, gw, float((G - ref).abs().max()), bar)
        # the float32 restatement is the float64 field to a few ulp
        assert np.abs(GA.field32(n.float().numpy(), tabs) - GA.field64(n.float(), tabs)[:, 0].numpy()).max() <= 8 * 2.0 ** -24 * 1.1


def test_host_refusals():
    from osmosis_diffusion_code_amd import ops, sampling
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    okw = OPS["underwater_physical_revised"]

    def cond(**kw):
        op = M.get_operator("underwater_physical_revised", device="cpu", batch_size=1, **okw, **kw)
        return CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), loss_function="norm", loss_weight="none",
                                          gradient_x_prev=True)
    c = cond()
    for bad in ((1, 5), (5, 1), (33, 5), (5, 40), (5,), 5, (2.5, 3), "5x5"):
        with pytest.raises(ValueError, match="gain_field"):
            c.set_gain_field(grid=bad)
    for kw in (dict(g_min=0.0), dict(g_min=-0.1), dict(g_min=float("nan")), dict(eta=-1.0), dict(eta=float("inf")), dict(smooth=-1.0),
               dict(n_iter=0), dict(n_iter=1.5), dict(init=np.ones((4, 5))), dict(init=-np.ones((5, 5))), dict(init=np.full((5, 5), np.nan))):
        with pytest.raises(ValueError, match="gain_field"):
            c.set_gain_field(**kw)
    assert c._gain is None
    st = c.set_gain_field(grid=(3, 4), init=2.0 * np.ones((3, 4)), learn=False)
    assert st["grid"] == (3, 4) and float(st["init"].max()) == 1.0 and st["learn"] is False       # the gauge: scaled to max = 1
    with pytest.raises(ValueError, match="more nodes than"):
        c.gain_open(1, 2, 8, "cpu")
    assert c.gain_values() is None
    vals = c.gain_open(1, 6, 8, "cpu") and c.gain_values()
    assert tuple(vals["nodes"].shape) == (1, 3, 4) and tuple(vals["field"].shape) == (1, 1, 48) and float(vals["field"].min()) == 1.0
    assert c.set_gain_field(None) is None and c._gain is None and c.gain_values() is None
    # robust and gain together, either order
    c.set_robust(loss="tukey")
    with pytest.raises(NotImplementedError, match="gain_field"):
        c.set_gain_field()
    c = cond()
    c.set_gain_field()
    with pytest.raises(NotImplementedError, match="gain_field"):
        c.set_robust(loss="huber")
    # a degradation inside the physical operator
    c = cond(degradation=dict(name="gaussian_blur", kernel_size=5, intensity=1.0))
    with pytest.raises(NotImplementedError, match="gain_field"):
        c.set_gain_field()
    # the 'ps' branch has no such model
    ps = CM.get_conditioning_method("ps", M.get_operator("noise", device="cpu"), M.get_noise("gaussian", sigma=0.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="gain_field"):
        ps.set_gain_field()
    assert ps.set_gain_field(None) is None
    # unknown keys: the loop's keyword and the config
    sampler = gd.create_sampler(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type="learned_range",
                                dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False, timestep_respacing="10")
    x = torch.zeros(1, 4, 8, 8)
    c = cond()
    with pytest.raises(ValueError, match="unknown keys"):
        sampler.p_sample_loop(None, x, x[:, :3], c.conditioning, False, None, gain_field=dict(grid=(3, 3), rate=0.1))
    with pytest.raises(ValueError, match="dict"):
        sampler.p_sample_loop(None, x, x[:, :3], c.conditioning, False, None, gain_field=(3, 3))
    with pytest.raises(NotImplementedError, match="gain_field"):
        sampler.p_sample_loop(None, x, x[:, :3], ps.conditioning, False, None, gain_field=dict(grid=(3, 3)))
    with pytest.raises(ValueError, match="unknown key"):
        sampling.gain_config(dict(grid=[5, 5], rate=0.1))
    with pytest.raises(ValueError, match="mapping"):
        sampling.gain_config([5, 5])
    assert sampling.gain_config(None) is None and sampling.gain_config({}) is None
    assert sampling.gain_config(dict(grid=[3, 4], eta=0.1), dict(grid=(2, 2)))["grid"] == (2, 2)       # the argument wins
    with pytest.raises(ValueError, match="gain_field"):
        ops.gain_desc((5, 5), 0.01, 1, 0.0, 0.05, True, 0, 3, 1, 4, 8)                 # more nodes than rows


def test_entry_points_refuse_bad_arguments_before_any_launch():
    from osmosis_diffusion_code_amd import ops
    lib = _lib.load()
    p = 4096                                                                      # never dereferenced on the host

    def desc(**kw):
        d = ops.gain_desc((5, 5), 0.01, 1, 0.0, 0.05, True, 0, 3, 2, 36, 34)
        for k, v in kw.items():
            setattr(d, k, v)
        return ctypes.byref(d)

    def prep(d=None, F=p, y=p, nodes=p, t=p, cs=p, ye=p, iy0=p, freeze=0):
        return lib.osm_gain_prepare(d or desc(), iy0, p, p, p, F, y, p, nodes, t, p, cs, ye, p, p, freeze, None)
    cases = [(lambda: prep(y=None), "null pointer"), (lambda: prep(nodes=None), "null pointer"), (lambda: prep(ye=None), "null pointer"),
             (lambda: prep(iy0=None), "tables"), (lambda: prep(F=None), "learning sub-step"), (lambda: prep(t=None), "learning sub-step"),
             (lambda: prep(cs=None), "learning sub-step"), (lambda: prep(desc(B=0)), "bad shape"), (lambda: prep(desc(H=1)), "bad shape"),
             (lambda: prep(desc(B=70000)), "too many"), (lambda: prep(desc(gh=1)), "bad grid"), (lambda: prep(desc(gw=33)), "bad grid"),
             (lambda: prep(desc(gh=32, H=20)), "bad grid"), (lambda: prep(desc(P=5)), "P must be"), (lambda: prep(desc(loss_type=2)), "loss_type"),
             (lambda: prep(desc(eta=-1.0)), "eta"), (lambda: prep(desc(eta=float("nan"))), "eta"), (lambda: prep(desc(**{"lambda": -1.0})), "lambda"),
             (lambda: prep(desc(g_min=0.0)), "g_min"), (lambda: prep(desc(g_min=float("nan"))), "g_min"), (lambda: prep(desc(n_iter=0)), "n_iter"),
             (lambda: prep(desc(learn=2)), "learn"), (lambda: prep(desc(W=5000, H=8)), "wider"),
             (lambda: lib.osm_gain_prepare(None, p, p, p, p, p, p, p, p, p, p, p, p, p, p, 0, None), "descriptor"),
             (lambda: lib.osm_gain_expand(desc(), p, p, p, p, None, p, p, p, p, p, None), "null pointer"),
             (lambda: lib.osm_gain_expand(desc(), p, p, p, None, p, p, p, p, p, p, None), "tables"),
             (lambda: lib.osm_gain_rows(desc(), p, p, p, p, p, None, p, p, p, p, None), "null pointer"),
             (lambda: lib.osm_gain_rows(desc(W=5000, H=8), p, p, p, p, p, p, p, p, p, p, None), "wider"),
             (lambda: lib.osm_gain_step(desc(), p, p, p, p, None, p, None), "null pointer"),
             (lambda: lib.osm_gain_step(desc(), p, p, p, p, p, None, None), "null pointer"),
             (lambda: lib.osm_gain_step(desc(g_min=-1.0), p, p, p, p, p, p, None), "g_min")]
    for fn, msg in cases:
        assert fn() != 0
        assert msg in lib.osm_last_error().decode(), (msg, lib.osm_last_error().decode())
    with pytest.raises(_lib.OsmosisHipError, match="CPU tensor"):                  # no CPU fall-back
        d = ops.gain_desc((2, 2), 0.01, 1, 0.0, 0.05, False, 0, 3, 1, 4, 4)
        tabs = tuple(torch.from_numpy(a) for a in ops.gain_tables_host(4, 4, 2, 2))
        ops.gain_expand(d, tabs, torch.ones(1, 2, 2), torch.zeros(1, 3, 16), None, torch.zeros(1, 3, 16), torch.zeros(1, 3, 16),
                        torch.zeros(1, 1, 16))


# ------------------------------------------------------------------------------------------------------------ the identity
def problem(B, H, W, seed, grid=(5, 5)):
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g, dtype=torch.float64)).clamp(-1.0, 1.0)
    y = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * 1.6 - 0.8
    mask = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * (torch.rand(B, 1, H, W, generator=g) > 0.3).double()
    nodes = 0.3 + 0.7 * torch.rand(B, *grid, generator=g, dtype=torch.float64)
    nodes = nodes / nodes.flatten(1).max(dim=1).values[:, None, None]
    return x0, y, mask, nodes


IDENTITY = [(op, lf, lw, masked, aux) for op in OPS for lf in ("norm", "mse") for lw in ("none", "depth") for masked in (False, True)
            for aux in ((AUX,) if (lf, lw, masked) == ("norm", "depth", True) else (None,))] + \
           [("underwater_physical_revised", "mse", "none", False, AUX), ("haze_physical", "norm", "none", True, AUX)]


@pytest.mark.parametrize("case", IDENTITY, ids=lambda c: "-".join(str(v if not isinstance(v, dict) else "aux") for v in c))
def test_identity_masked_oracle_on_the_expanded_measurement_is_the_model_written_out(case):
    """In float64, 5 inner iterations: the masked oracle on (y', M G) against the oracle of I = G F written out directly -- loss, phi
    and dL/dx0 to 1e-12 (relative to each quantity's largest entry)."""
    opname, lf, lw, masked, aux = case
    H, W = 12, 10
    x0, y, mask, nodes = problem(1, H, W, 3 + IDENTITY.index(case))
    okw = dict(OPS[opname], **etas(OPS[opname], 1e-3))
    G = GA.field64(nodes, GA.tables(H, W, 5, 5))
    m0 = mask if masked else None
    me = (mask if masked else torch.ones_like(y)) * G
    a = GO.group_inner_loop(opname, okw, None, x0, (y + 1) / G - 1, me, 5, None, aux, lf, lw, "mean")
    b = GA.direct_inner_loop(opname, okw, x0, y, m0, G, 5, aux, lf, lw)
    assert abs(a[0][0] - b[0][0]) <= 1e-12 * abs(b[0][0]), (a[0], b[0])
    for k in a[1]:
        assert float((a[1][k].double() - b[1][k].double()).abs().max()) <= 1e-12, k
        assert float((b[1][k].double() - D.PhysOperator(opname, **okw).phi[k].double()).abs().max()) > 1e-7      # phi has moved
    assert float((a[2] - b[2]).abs().max()) <= 1e-12 * float(b[2].abs().max())


@pytest.mark.parametrize("lf", ["norm", "mse"])
@pytest.mark.parametrize("masked,weighted", [(False, False), (True, True)])
def test_oracle_gradient_is_autograd_of_its_loss(lf, masked, weighted):
    H, W = 14, 11
    x0, y, mask, nodes = problem(2, H, W, 11, grid=(3, 4))
    tabs = GA.tables(H, W, 3, 4)
    F, w = GA.model_image("underwater_physical_revised", OPS["underwater_physical_revised"], x0, "depth" if weighted else "none")
    n = nodes.clone().requires_grad_(True)
    r = (y - (2 * GA.field64(n, tabs) * F - 1)) * w * (mask if masked else 1)
    L = torch.sqrt((r * r).sum(dim=(1, 2, 3))).sum() if lf == "norm" else (r * r).mean(dim=(1, 2, 3)).sum()
    (g,) = torch.autograd.grad(L, n)
    c = GA.grad64(nodes, tabs, F, w, y, mask if masked else None, lf)[0]
    assert float((g - c).abs().max()) <= 1e-10


def test_step_gauge_floor_and_guards():
    rng = np.random.default_rng(2)
    n = (0.2 + 0.8 * rng.random((4, 5, 5))).astype(np.float32)
    c_raw = rng.standard_normal((4, 5, 5)) * 40
    S = np.array([4.0, np.nan, 0.0, 9.0])
    out = GA.step64(n, c_raw, S, "norm", 100, 0.1, 0.3, 0.05)
    assert out[0].max() == 1.0 and out[3].max() == 1.0 and out.min() >= float(np.float32(0.05)) and (out[0] == float(np.float32(0.05))).any()
    assert np.array_equal(out[1], n[1].astype(np.float64)) and np.array_equal(out[2], n[2].astype(np.float64))      # the guards
    assert not np.array_equal(GA.step64(n, c_raw, S, "mse", 100, 0.1, 0.3, 0.05)[2], n[2])         # S = 0 guards the norm loss only
    for bad in (-np.inf, np.nan):                                                                  # max(u) not finite
        c_bad = c_raw.copy()
        c_bad[3, 2, 2] = bad
        assert np.array_equal(GA.step64(n, c_bad, S, "norm", 100, 0.1, 0.0, 0.05)[3], n[3])
    flat = np.ones((1, 4, 4))
    assert np.array_equal(GA.laplacian(flat), np.zeros_like(flat))
    bump = flat.copy()
    bump[0, 1, 1] = 2.0
    assert GA.laplacian(bump)[0, 1, 1] == 4.0 and GA.laplacian(bump)[0, 0, 1] == -1.0 and GA.laplacian(bump).sum() == 0.0


# ------------------------------------------------------------------------------------------------------------ the effect
def test_effect_a_cos4_vignette_is_learnt_on_the_oracle_alone():
    """36 x 34, 5 x 5 nodes, G* = cos^4(atan(0.7 rho)) over its maximum, phi* = (1.2, 0.6, 0.4 | 1.0, 0.7, 0.5 | 0.1, 0.5, 0.6), noise
    0.01, image and phi held at the truth, norm loss, eta 0.01, smooth 0, 200 sub-steps from a flat field: max |G - G*| at most 0.25 x
    the flat field's (measured: 0.730 -> 0.0879, 0.12 x; the least-squares floor of a 5 x 5 bilinear field on this G* is 0.054)."""
    x0, y, Gs, F = GA.effect_problem()
    G = GA.effect_fit(F, y)
    flat, got = float(np.abs(1.0 - Gs).max()), float(np.abs(G - Gs).max())
    print(f"GAINEFFECT norm eta 0.01, 200 sub-steps: max |G - G*| {flat:.4f} -> {got:.4f} ({got / flat:.3f} x)")
    assert got <= 0.25 * flat, (flat, got)
    assert G.max() <= 1.0 + 1e-12 and G.min() >= 0.05


# ------------------------------------------------------------------------------------------------------------ the torch route
class Foreign:
    """An image-formation model the kernels do not know (no fill_desc): the autograd route's case.  Depth conversion: 'original'."""
    depth_type, value = "original", None

    def forward(self, data, **kw):
        d = 0.5 * (data[:, 3:4] + 1.0)
        return 0.5 * (data[:, 0:3] + 1.0) * torch.exp(-0.8 * d) + 0.2 * (1 - torch.exp(-0.8 * d))


@pytest.mark.parametrize("lf", ["norm", "mse"])
@pytest.mark.parametrize("masked", [False, True])
def test_loss_autograd_with_the_field_is_the_oracles_objective(lf, masked):
    """`_loss_autograd` on a foreign operator with the field, float32, against the float64 oracle (the nodes stepped at the start,
    then the model G F): loss, d loss / d x0 and the nodes to 1e-5."""
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    from osmosis_diffusion_code_amd.guided_diffusion import measurements as M
    H, W = 12, 10
    x0, y, mask, nodes = problem(2, H, W, 21, grid=(3, 4))
    eta = 0.05 if lf == "norm" else 5.0
    op = Foreign()
    cond = CM.get_conditioning_method("osmosis", op, M.get_noise("clean"), gradient_x_prev=True, loss_function=lf, loss_weight="none")
    assert not cond._has_kernels()
    if masked:
        cond.set_measurement_mask(mask.float())
    cond.set_gain_field(grid=(3, 4), eta=eta, n_iter=2, smooth=0.1, init=nodes.numpy())
    xa = x0.float().clone().requires_grad_(True)
    sep, loss, _ = cond._loss_autograd(xa, y.float())
    (ga,) = torch.autograd.grad(loss, xa)
    tabs = GA.tables(H, W, 3, 4)
    xb = x0.float().double().requires_grad_(True)
    Fb = op.forward(xb)
    m0 = mask.float().double() if masked else None
    n0 = nodes.float().double().numpy()
    new = GA.learn64(n0, tabs, Fb.detach(), 1, y.float().double(), m0, lf, eta, 2, 0.1, 0.05)
    assert np.abs(new - n0).max() > 1e-3                                          # the nodes have moved
    r = (y.float().double() - (2 * GA.field64(torch.from_numpy(new), tabs) * Fb - 1)) * (1 if m0 is None else m0)
    per = torch.linalg.vector_norm(r, dim=(1, 2, 3)) if lf == "norm" else (r * r).mean(dim=(1, 2, 3))
    want = torch.linalg.norm(r) if lf == "norm" else per.sum()
    (gb,) = torch.autograd.grad(want, xb)
    assert np.allclose(sep, per.detach().numpy(), rtol=1e-5)
    assert abs(float(loss.detach()) - float(want.detach())) <= 1e-5 * float(want.detach())
    assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max())
    vals = cond.gain_values()
    assert float((vals["nodes"].double() - torch.from_numpy(new)).abs().max()) <= 1e-5
    assert float((vals["field"].double().view(2, 1, H, W) - GA.field64(torch.from_numpy(new), tabs)).abs().max()) <= 1e-5
    # learn=False keeps the nodes: a measured flat field
    cond.set_gain_field(grid=(3, 4), init=nodes.numpy(), learn=False)
    cond._loss_autograd(xa, y.float())
    assert torch.equal(cond.gain_values()["nodes"], nodes.float())


def test_flat_field_to_nodes_by_least_squares(tmp_path):
    from osmosis_diffusion_code_amd import sampling
    H, W = 36, 34
    tabs = GA.tables(H, W, 5, 5)
    n = 0.3 + 0.7 * torch.rand(1, 5, 5, generator=torch.Generator().manual_seed(4), dtype=torch.float64)
    n = n / n.max()
    flat = GA.field64(n, tabs)[0, 0].numpy()
    got = sampling.gain_nodes_from_flat_field(3.0 * flat, (5, 5))
    assert np.abs(got - n[0].numpy()).max() <= 1e-9                              # a field in the span comes back, scaled to max = 1
    Gs = GA.vignette(H, W)
    fit = GA.field64(torch.from_numpy(sampling.gain_nodes_from_flat_field(Gs, (5, 5)))[None], tabs)[0, 0].numpy()
    scale = float((fit * Gs).sum() / (fit * fit).sum())                           # (the nodes come back scaled to max = 1)
    err = float(np.abs(scale * fit - Gs).max())
    assert 0.054 <= err <= 0.1, err                 # above the minimax floor of a 5 x 5 bilinear field on this G*, and near it
    np.save(tmp_path / "flat.npy", Gs)
    np.save(tmp_path / "nodes.npy", n[0].numpy())
    a = sampling.gain_config(dict(grid=[5, 5], learn=False, path=str(tmp_path / "flat.npy")), None, (H, W))
    b = sampling.gain_config(dict(grid=[5, 5], path=str(tmp_path / "nodes.npy")), None, (H, W))
    assert a["learn"] is False and "path" not in a and a["init"].shape == (5, 5) and np.array_equal(b["init"], n[0].numpy())
    with pytest.raises(ValueError, match="neither nodes"):
        sampling.gain_config(dict(grid=[5, 5], path=str(tmp_path / "flat.npy")), None, (32, 32))
    with pytest.raises(ValueError, match="flat field"):
        sampling.gain_nodes_from_flat_field(-Gs, (5, 5))
