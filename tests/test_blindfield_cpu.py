"""Blind spatially varying deblurring without a GPU: the `blind_field_blur` operator (registry, validation, init fields, `learn: False`
against `field_blur`, `reset()`), every refusal, the layout of the per-node tap partials against a brute-force enumeration from the
tables, and the oracle of tests/blindfield_oracle.py against itself: its tap correlation against the definition and against autograd
of Q, the two identities that tie it to blind's c and to <r, A(w) x>, and the recovery of a known field on a convex problem; and
what of the three entry points needs no GPU: their place in the ABI table, the header's macros, every validation that fails before
a launch, and how the Makefile builds the two field sources into the one library."""
import ctypes
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import blind_oracle as BO
import blindfield_oracle as O
import psffield_oracle as FO
from osmosis_diffusion_code_amd import _lib, ops, torch_ops
from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INC = os.path.join(ROOT, "include")


def bfield(**kw):
    return M.get_operator("blind_field_blur", device="cpu", **kw)


def test_operator_is_registered_a_field_operator_and_couples_the_batch():
    op = bfield()
    assert isinstance(op, M.PSFFieldOperator) and isinstance(op, M.GRID_OPERATORS) and op.__name__ == "blind_field_blur"
    assert M.GRID_OPERATORS == (M.SeparableOperator, M.PSFOperator)
    assert op.couples_batch is True and op.weight_sets == (1, 1)
    assert (op.kernel_size, op.grid, op.eta, op.n_iter, op.l1, op.smooth, op.learn) == (31, (3, 3), 0.1, 1, 0.0, 0.0, True)
    assert op.radius() == (15, 15) and op.out_shape(40, 50) == (40, 50)
    dy, dx, w = op.taps("cpu")
    assert dy.dtype == dx.dtype == torch.int32 and w.dtype == torch.float32 and dy.shape == dx.shape == (961,) and w.shape == (3, 3, 961)
    assert dy[:32].tolist() == [-15] * 31 + [-14] and dx[:32].tolist() == list(range(-15, 16)) + [-15]          # dense, row-major
    init = M.blind_init_kernel(31)
    assert all(np.array_equal(op.kernels()[jy, jx], init.astype(np.float32).astype(np.float64)) for jy in range(3) for jx in range(3))
    with pytest.raises(ValueError, match="kernels"):
        op.kernel2d()
    with pytest.raises(ValueError, match="reflection"):
        op.out_shape(15, 64)
    with pytest.raises(ValueError, match="more nodes"):
        bfield(kernel_size=1, grid=[5, 5]).out_shape(4, 64)
    assert "field_tap_grad" in torch_ops.OPS and "field_tap_step" in torch_ops.OPS and "field_tap_grad" not in torch_ops.OPS_C
    assert "Tensor(a0!) w" in str(torch.ops.osmosis.field_tap_step.default._schema)


def test_learn_false_is_field_blur_with_the_init_field():
    rng = np.random.default_rng(0)
    init = rng.random((2, 3, 3, 5))
    init[:, :, 0, 0] = 0.0                                                                  # a tap no node carries: not in the union
    a = bfield(kernel_size=7, grid=[2, 3], init=init, learn=False)
    b = M.get_operator("field_blur", device="cpu", kernels=a.kernels(), normalize=False)
    assert a.couples_batch is False and a.learn is False and a.grid == b.grid == (2, 3)
    for s, t in zip(a.host_taps(), b.host_taps()):
        assert np.array_equal(s, t)
    assert a.radius() == b.radius() == (1, 2) and len(a.host_taps()[0]) == 14
    assert np.array_equal(a.kernels(), b.kernels()) and np.allclose(a.kernels().sum(axis=(2, 3)), 1.0, rtol=0, atol=1e-15)
    one = bfield(kernel_size=5, init="delta", learn=False)
    assert one.radius() == (0, 0) and one.host_taps()[2].reshape(-1).tolist() == [1.0] * 9


def test_init_fields_and_reset(tmp_path):
    f = M.blind_field_init(5, (2, 3), "gaussian", 1.0)
    assert f.shape == (2, 3, 5, 5) and f.dtype == np.float64 and np.array_equal(f[1, 2], M.blind_init_kernel(5, "gaussian", 1.0))
    nodes = np.zeros((2, 2, 1, 3))
    nodes[..., 0, :] = [[[1.0, 3.0, 0.0], [0.0, 1.0, 0.0]], [[2.0, 2.0, 0.0], [0.0, 0.0, 5.0]]]
    f = M.blind_field_init(3, (2, 2), nodes)
    assert f.shape == (2, 2, 3, 3) and f[0, 0, 1].tolist() == [0.25, 0.75, 0.0] and f[1, 1, 1].tolist() == [0.0, 0.0, 1.0] and f[:, :, 0].sum() == 0
    path = os.path.join(tmp_path, "f.npy")
    np.save(path, nodes)
    assert np.array_equal(bfield(kernel_size=3, grid=[2, 2], init=path).kernels(), f.astype(np.float32).astype(np.float64))
    np.save(path, np.array([[1.0, 3.0, 0.0]]))
    assert bfield(kernel_size=3, grid=[2, 2], init=path).kernels()[1, 0, 1].tolist() == [0.25, 0.75, 0.0]      # one kernel for every node
    # the live weights: kernels() reads them, reset puts the init back into the SAME tensor
    op = bfield(kernel_size=5, grid=[2, 3])
    w = op.taps("cpu")[2]
    first = op.kernels()
    assert first.shape == (2, 3, 5, 5) and np.array_equal(first.reshape(2, 3, 25), op.host_taps()[2].astype(np.float64))
    w.fill_(0.04)
    assert np.all(op.kernels() == np.float64(np.float32(0.04)))
    assert op.reset() is op and op.taps("cpu")[2] is w and np.array_equal(op.kernels(), first)
    assert np.array_equal(op.host_taps()[2].astype(np.float64).reshape(2, 3, 5, 5), first)      # (the host copy was never aliased)


def test_validation_errors():
    for bad in (8, 0, -3, 2.5, "9", True, 63):
        with pytest.raises(ValueError, match="blind_field_blur: kernel_size"):
            bfield(kernel_size=bad)
    assert bfield(kernel_size=61).radius() == (30, 30)
    for bad in ([1, 3], [3, 33], [3], "33", [2.5, 3]):
        with pytest.raises(ValueError, match="blind_field_blur: grid"):
            bfield(grid=bad)
    with pytest.raises(ValueError, match="blind_field_blur: init_sigma"):
        bfield(init_sigma=0.0)
    with pytest.raises(ValueError, match="blind_field_blur: init"):
        bfield(init="box")
    with pytest.raises(ValueError, match="2 x 2 nodes, the grid is 3 x 3"):
        bfield(kernel_size=3, init=np.ones((2, 2, 3, 3)))
    with pytest.raises(ValueError, match="non-negative"):
        bfield(kernel_size=3, grid=[2, 2], init=-np.ones((2, 2, 3, 3)))
    with pytest.raises(ValueError, match="larger"):
        bfield(kernel_size=3, grid=[2, 2], init=np.ones((2, 2, 5, 5)))
    for key in ("eta", "l1", "smooth"):
        for bad in (-1.0, float("nan"), float("inf")):
            with pytest.raises(ValueError, match=f"blind_field_blur: {key}"):
                bfield(**{key: bad})
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="blind_field_blur: n_iter"):
            bfield(n_iter=bad)
    with pytest.raises(ValueError, match=r"blind_field_blur: unknown config key\(s\) \['n_iters'\]"):
        bfield(n_iters=3)
    with pytest.raises(ValueError, match=r"blind_field_blur: unknown config key\(s\) \['kernels'\]"):
        bfield(kernels=np.ones((2, 2, 3, 3)))
    for key in ("per_image", "per_channel"):
        with pytest.raises(ValueError, match=f"blind_field_blur: {key} is not supported"):
            bfield(**{key: False})
    assert bfield(simulate=False, simulate_with=dict(name="field_blur")).n_iter == 1          # the driver's keys pass through
    # field_blur itself is what it was
    with pytest.raises(ValueError, match="field_blur: unknown config key"):
        M.get_operator("field_blur", device="cpu", model="radial_defocus", eta=0.1)


def test_refusals_name_the_operator():
    from osmosis_diffusion_code_amd import sampling
    with pytest.raises(ValueError, match="blind_field_blur"):
        M.build_degradation({"name": "blind_field_blur", "kernel_size": 5}, "cpu")
    with pytest.raises(ValueError, match="blind_field_blur"):
        M.build_degradation(bfield(kernel_size=5), "cpu")
    with pytest.raises(_lib.OsmosisHipError, match="lin_desc: 'blind_field_blur'"):
        ops.lin_desc(bfield(kernel_size=5), 16, 24, "cpu")
    with pytest.raises(_lib.OsmosisHipError, match="lin_config: 'blind_field_blur'"):
        torch_ops.lin_config(bfield(kernel_size=5), 16, 24, "cpu")
    with pytest.raises(ValueError, match="field_blur"):                                       # ... and field_blur's own still stand
        M.build_degradation({"name": "field_blur", "model": "radial_defocus"}, "cpu")
    gauss = M.get_noise("gaussian", sigma=0.0)
    cond = CM.get_conditioning_method("ps", bfield(kernel_size=5), M.get_noise("poisson", rate=1.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="blind_field_blur.*poisson"):
        cond.hip_ok(3)
    cond = CM.get_conditioning_method("ps", bfield(kernel_size=5), gauss, scale="0.3")
    assert cond.hip_ok(3) and cond._blind() is cond.operator and cond._blind_field() is cond.operator
    fixed = CM.get_conditioning_method("ps", bfield(kernel_size=5, learn=False), gauss, scale="0.3")
    assert fixed._blind() is None and fixed.hip_ok(3)                                         # a fixed field: field_blur's three launches
    assert CM.get_conditioning_method("ps", M.get_operator("blind_blur", device="cpu", kernel_size=5), gauss, scale="0.3")._blind_field() is None
    with pytest.raises(NotImplementedError, match="BlindFieldOperator"):
        cond.set_robust("tukey")
    cond.set_robust(None)
    # rows= that is not the whole open batch
    cond.open_batch(3, (16, 24), (16, 24), "cpu")
    with pytest.raises(ValueError, match="blind_field_blur: the learnt field is shared by the batch.*rows 0:2"):
        cond.loss_grad_x0(torch.zeros(2, 3, 16, 24), torch.zeros(2, 3, 16, 24), rows=(0, 2))

    def cfg(**okw):
        return {"measurement": {"operator": dict(name="blind_field_blur", kernel_size=5, **okw), "noise": {"name": "gaussian", "sigma": 0.0}},
                "conditioning": {"method": "ps", "params": dict(scale="0.3")},
                "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                                  model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                                  timestep_respacing="4"),
                "sample_pattern": dict(pattern="original"), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "imagenet"},
                "manual_seed": 0, "rgb_guidance": True}
    ref = torch.zeros(1, 3, 16, 24)
    with pytest.raises(ValueError, match="blind_field_blur: `simulate: True` needs `simulate_with"):
        sampling.restore_image(None, ref, cfg(), device="cpu")
    with pytest.raises(ValueError, match="blind_field_blur: simulate_with 'super_resolution' changes"):
        sampling.restore_image(None, ref, cfg(simulate_with=dict(name="super_resolution", scale_factor=2)), device="cpu")
    with pytest.raises(NotImplementedError, match="blind_field_blur: tiling"):
        sampling.restore_image(None, ref, cfg(simulate=False), device="cpu", tiling=dict(tile=16))
    with pytest.raises(ValueError, match="per_image"):
        sampling.restore_image(None, ref, cfg(per_image=True), device="cpu")
    assert sampling.measurement_grid({"name": "blind_field_blur", "kernel_size": 5}, (16, 24)) == (16, 24)


# ---------------------------------------------------------------------------------------------------- the layout
def brute_layout(H, W, gh, gw, P):
    """The layout from the tables by enumeration: for every node the set of tiles it reaches, then the ranges and offsets."""
    iy0, _, ix0, _ = ops.gain_tables_host(H, W, gh, gw)
    nty, ntx = -(-H // 32), -(-W // 32)
    rows = [sorted({ty for ty in range(nty) if any(iy0[i] in (jy - 1, jy) for i in range(32 * ty, min(32 * ty + 32, H)))}) for jy in range(gh)]
    cols = [sorted({tx for tx in range(ntx) if any(ix0[j] in (jx - 1, jx) for j in range(32 * tx, min(32 * tx + 32, W)))}) for jx in range(gw)]
    for s in rows + cols:
        assert s and s == list(range(s[0], s[-1] + 1))                                       # an interval, never empty
    off = [0]
    for jy in range(gh):
        for jx in range(gw):
            off.append(off[-1] + P * len(rows[jy]) * len(cols[jx]))
    return [s[0] for s in rows] + [s[-1] + 1 for s in rows] + [s[0] for s in cols] + [s[-1] + 1 for s in cols] + off


@pytest.mark.parametrize("H,W,gh,gw", [(36, 34, 2, 2), (70, 66, 5, 5), (8, 12, 2, 3), (36, 34, 32, 32)])
def test_layout_matches_a_brute_force_enumeration_from_the_tables(H, W, gh, gw):
    _, NP, lay = ops.field_tap_layout(H, W, gh, gw, 3)
    want = brute_layout(H, W, gh, gw, 3)
    assert lay.dtype == np.int32 and lay.tolist() == want and NP == want[-1]
    assert ops.field_tap_layout(H, W, gh, gw, 1)[1] * 3 == NP
    # every (tile, plane) is reached by at least four nodes, so the compact layout holds at least four times blind's partials
    assert NP >= 4 * ops.tap_grad_nparts(3, H, W)
    print(f"{H}x{W} / {gh}x{gw}: {NP} partials per image ({ops.tap_grad_nparts(3, H, W)} tiles x planes)")


def test_layout_refuses_bad_grids():
    for H, W, gh, gw in ((8, 12, 1, 3), (8, 12, 9, 3), (64, 64, 33, 3)):
        with pytest.raises(_lib.OsmosisHipError, match="osm_field_tap_layout: the node grid"):
            ops.field_tap_layout(H, W, gh, gw, 3)


# ---------------------------------------------------------------------------------------------------- the oracle against itself
def _problem(seed=3, B=2, H=8, W=6, gh=3, gw=2, k=5):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * 2 - 1
    y = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * 2 - 1
    K = torch.rand(gh, gw, k, k, generator=g, dtype=torch.float64)
    K = K / K.sum(dim=(2, 3), keepdim=True)
    return x, y, K


def test_tap_correlation_of_the_oracle_equals_the_definition_autograd_of_q_and_blinds_c():
    x, y, K = _problem()
    B, _, H, W = x.shape
    gh, gw, k, _ = K.shape
    dy, dx = BO.dense_taps(k)
    loss, r = BO.loss_and_r(FO.forward_sum(x, K), y)
    c = O.tap_corr(r, x, gh, gw, k, k).reshape(B, gh, gw, k * k).numpy()
    direct = O.tap_corr_direct(r, x, gh, gw, dy, dx)
    scale = np.abs(direct).max()
    assert np.abs(c - direct).max() <= 1e-12 * scale
    # autograd of Q = sum_b ||rho_b||^2 / (2 * 3 h w) through the float64 field operator: dQ/dK_n = sum_b loss_b c_n[b] / (3 h w)
    Kl = K.clone().requires_grad_(True)
    Q = ((y - FO.forward_sum(x, Kl)) ** 2).sum() / (2 * 3 * H * W)
    (dQ,) = torch.autograd.grad(Q, Kl)
    want = np.einsum("b,bnmt->nmt", loss.numpy(), direct) / (3 * H * W)
    assert np.abs(dQ.reshape(gh, gw, -1).numpy() - want).max() <= 1e-12 * np.abs(want).max()
    # the hats sum to one at every pixel: the node partials add up to blind's c
    blind_c = BO.tap_corr_direct(r, x, dy, dx)
    assert np.abs(direct.sum(axis=(1, 2)) - blind_c).max() <= 1e-12 * np.abs(blind_c).max()
    # sum_n sum_t w_n c_n = <r, A(w) x>
    lhs = np.einsum("nmt,bnmt->b", K.reshape(gh, gw, -1).numpy(), direct)
    rhs = (r * FO.forward_sum(x, K)).sum(dim=(1, 2, 3)).numpy()
    assert np.abs(lhs - rhs).max() <= 1e-12 * np.abs(rhs).max()


def test_step_of_the_oracle_is_blinds_per_node_and_keeps_the_simplex():
    rng = np.random.default_rng(5)
    gh, gw, T, B = 2, 3, 49, 2
    w = rng.random((gh, gw, T)).astype(np.float32)
    w /= w.sum(axis=2, keepdims=True)
    c = rng.standard_normal((B, gh, gw, T)) * 40
    loss = rng.random(B).astype(np.float32)
    new = O.step(w, c, loss, 300, 0.5, 1e-3, 0.0)
    for jy in range(gh):
        for jx in range(gw):
            assert np.array_equal(new[jy, jx], BO.step(w[jy, jx], c[:, jy, jx], loss, 300, 0.5, 1e-3)[0])
    sm = O.step(w, c, loss, 300, 0.5, 1e-3, 0.2)
    assert not np.array_equal(sm, new) and (sm >= 0).all() and np.abs(sm.sum(axis=2) - 1).max() < 1e-6 and (sm == 0).any()
    # the smoothing term pulls the nodes together: with no data gradient the field's spread shrinks
    flat = O.step(w, np.zeros_like(c), loss, 300, 0.5, 0.0, 0.2)
    assert np.abs(flat - flat.mean(axis=(0, 1))).sum() < np.abs(w - w.mean(axis=(0, 1))).sum()
    # a corner has two neighbours, an edge node three
    lap = O.laplace(w.astype(np.float64))
    assert np.allclose(lap[0, 0], 2 * w[0, 0].astype(np.float64) - w[1, 0] - w[0, 1], rtol=0, atol=1e-15)
    assert np.allclose(lap[0, 1], 3 * w[0, 1].astype(np.float64) - w[0, 0] - w[0, 2] - w[1, 1], rtol=0, atol=1e-15)
    # a non-finite loss leaves every node as it was
    assert np.array_equal(O.step(w, c, np.array([np.nan, 1.0], np.float32), 300, 0.5), w)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_oracle_recovers_a_radial_defocus_field_when_the_image_is_known(seed):
    """36 x 44, 3 x 3 nodes, k = 5, eta = 4, 200 steps, y = A(K*) x + 0.005 N(0, 1), a gaussian of sigma 1 at every node.  Measured:
    seed 0: loss 3.028 -> 0.398 (0.132 x), mean per-node L1 0.493 -> 0.0964 (0.196 x), worst node 0.139, ONE shared PSF 2.469 (the
    field's last loss is 0.161 x that); seed 1: 3.050 -> 0.398 (0.130 x), 0.0965 (0.196 x), worst 0.164, shared 2.510 (0.158 x)."""
    prob = O.recovery_problem(seed)
    res = O.recover(*prob, 200, 4.0)
    one = O.recover(*prob, 200, 4.0, shared=True)
    print(f"seed {seed}: loss {res['first']:.4f} -> {res['last']:.4f} ({res['last'] / res['first']:.4f} x), mean L1 "
          f"{res['err_first'].mean():.4f} -> {res['err_last'].mean():.4f} ({res['err_last'].mean() / res['err_first'].mean():.4f} x), worst "
          f"{res['err_first'].max():.4f} -> {res['err_last'].max():.4f}; one shared PSF {one['last']:.4f} ({res['last'] / one['last']:.4f} x), "
          f"its mean L1 {one['err_last'].mean():.4f}")
    assert res["last"] <= 0.25 * res["first"]
    assert res["err_last"].mean() <= 0.5 * res["err_first"].mean()
    assert res["last"] <= 0.5 * one["last"]
    w = res["w"]
    assert (w >= 0).all() and np.abs(w.astype(np.float64).sum(axis=2) - 1).max() < 1e-6


# ---------------------------------------------------------------------------------------------------- the entry points
def test_entry_points_take_the_stream_last_the_layout_returns_long_long_and_the_header_has_no_struct():
    assert _lib.exports("osmosis_blindfield.h") == ["osm_field_tap_grad", "osm_field_tap_layout", "osm_field_tap_step"]
    # the stream stays the last argument of a launching entry point: a Recorder re-targets it on capture
    for name in ("osm_field_tap_grad", "osm_field_tap_step"):
        assert _lib.SIGS[name][-1] is ctypes.c_void_p
    assert _lib.SIGS["osm_field_tap_layout"].restype is ctypes.c_longlong
    assert "struct" not in re.sub(r"/\*.*?\*/", " ", open(os.path.join(INC, "osmosis_blindfield.h")).read(), flags=re.S)


@pytest.mark.skipif(shutil.which("gcc") is None, reason="no gcc")
def test_the_headers_macros_compile_as_c99(tmp_path):
    (tmp_path / "only.c").write_text('#include "osmosis_blindfield.h"\nint n = OSM_FIELD_LAY_INTS(3, 4) + OSM_FIELD_MAX_TAPS;\n')
    r = subprocess.run(["gcc", "-std=c99", "-pedantic", "-Wall", "-Werror", "-I", INC, "-fsyntax-only", str(tmp_path / "only.c")],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def test_the_loaded_library_binds_the_entry_points_to_the_table():
    lib = _lib.load()
    assert lib is _lib.load()
    for name in _lib.exports("osmosis_blindfield.h"):
        fn, argtypes = getattr(lib, name), _lib.SIGS[name]
        assert fn.argtypes == argtypes and fn.restype is getattr(argtypes, "restype", ctypes.c_int), name


@pytest.mark.skipif(shutil.which("nm") is None, reason="no nm")
def test_the_library_exports_no_name_of_any_prefix_beside_the_table():
    """Every dynamic symbol that starts with `osm`, whatever follows (the staging libraries' prefixes were osm + a letter), is in the table."""
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(re.findall(r"\s(osm\w+)$", nm, flags=re.M))
    assert exported == _lib.exports() and len(exported) == 136, set(exported) ^ set(_lib.exports())
    assert not [f for f in os.listdir(os.path.dirname(_lib.LIB_PATH)) if f.startswith("libosmosis_") and f != "libosmosis_hip.so"]


def test_a_null_pointer_fails_validation_and_leaves_its_text_in_osm_last_error():
    """A null pointer fails through validation: nothing is launched, so no GPU is needed."""
    lib = _lib.load()
    grad = [None] * 4 + [25, 2, 2, 3, 3] + [None] * 5 + [1, 3, 48, 48, 4, 4, None, None]
    with pytest.raises(_lib.OsmosisHipError, match=r"osm_field_tap_grad failed \(-1\): osm_field_tap_grad: null pointer"):
        _lib.call("osm_field_tap_grad", *grad)
    assert lib.osm_last_error().decode().startswith("osm_field_tap_grad: null pointer")
    assert _lib.last_error("osm_field_tap_grad") == lib.osm_last_error().decode()
    # ... one text for the library: a later failure of another entry point replaces it
    step = [None] * 5 + [3, 3, 1, 25, 100, 0.1, 0.0, 0.0, None]
    with pytest.raises(_lib.OsmosisHipError, match=r"osm_field_tap_step failed \(-1\): osm_field_tap_step: null pointer"):
        _lib.call("osm_field_tap_step", *step)
    assert lib.osm_last_error().decode().startswith("osm_field_tap_step: null pointer")
    assert _lib.last_error("osm_field_tap_grad") == _lib.last_error("osm_field_tap_step") == lib.osm_last_error().decode()
    with pytest.raises(_lib.OsmosisHipError, match="osm_psf_apply"):
        _lib.call("osm_psf_apply", *([None] * 5), 1, 0, 0, 1, 3, 48, 48, 4, 4, 0, 0, None)
    assert lib.osm_last_error().decode().startswith("osm_psf_apply")
    with pytest.raises(_lib.OsmosisHipError, match="osm_field_nothing"):
        _lib.call("osm_field_nothing")
    # a Recorder sees nothing of a failed call
    with _lib.Recorder() as rec:
        with pytest.raises(_lib.OsmosisHipError):
            _lib.call("osm_field_tap_grad", *grad)
    assert len(rec) == 0


def test_every_validation_of_the_step_and_the_layout_fails_before_a_launch():
    """The arguments are checked in full before anything is launched: non-null pointers that are never read stand in for buffers."""
    lib = _lib.load()
    p = ctypes.c_void_p(64)
    q = ctypes.c_void_p(128)
    ok = dict(w=p, w_new=q, gh=3, gw=3, B=1, T=25, hw3=100, eta=0.1, l1=0.0, smooth=0.0)

    def step(**kw):
        a = dict(ok, **kw)
        rc = lib.osm_field_tap_step(a["w"], a["w_new"], p, p, p, a["gh"], a["gw"], a["B"], a["T"], a["hw3"], a["eta"], a["l1"], a["smooth"], None)
        return rc, lib.osm_last_error().decode()
    for kw, text in ((dict(w_new=p), "must not alias"), (dict(gh=1), "node grid"), (dict(gw=33), "node grid"), (dict(B=0), "bad batch"),
                     (dict(T=0), "tap count"), (dict(T=4226), "tap count"), (dict(hw3=0), "hw3"), (dict(eta=float("nan")), "NaN"),
                     (dict(smooth=-1.0), "smooth"), (dict(smooth=float("inf")), "smooth"), (dict(smooth=float("nan")), "smooth")):
        rc, msg = step(**kw)
        assert rc == -1 and text in msg, (kw, rc, msg)
    iy0, ix0 = np.zeros(8, np.int32), np.zeros(12, np.int32)
    lay = np.zeros(64, np.int32)
    args = lambda gh=2, gw=3, H=8, W=12, P=3, B=1, T=25: (gh, gw, iy0.ctypes.data_as(ctypes.c_void_p), ix0.ctypes.data_as(ctypes.c_void_p),
                                                           H, W, P, B, T, lay.ctypes.data_as(ctypes.c_void_p))
    assert lib.osm_field_tap_layout(*args()) > 0
    for kw in (dict(gh=1), dict(gh=9), dict(gw=13), dict(P=0), dict(B=0), dict(T=0), dict(T=4226)):
        assert lib.osm_field_tap_layout(*args(**kw)) == -1, kw


def test_the_makefile_builds_the_field_sources_into_the_one_library_without_contraction():
    mk = open(os.path.join(ROOT, "osmosis_diffusion_code_amd", "csrc", "Makefile")).read()
    srcs = re.search(r"^SRCS = (.*)$", mk, flags=re.M).group(1).split()
    assert "psffield.hip" in srcs and "blindfield.hip" in srcs
    rules = re.findall(r"^([\w. ]+\.o): CXXFLAGS \+= (.*)$", mk, flags=re.M)
    for obj in ("psffield.o", "blindfield.o"):
        assert any(obj in targets.split() and "-ffp-contract=off" in flags for targets, flags in rules), obj
    assert set(re.findall(r"libosmosis_\w+", mk)) == {"libosmosis_hip"} and "-fvisibility=hidden" not in mk       # one library, nothing hidden
    assert not os.path.exists(os.path.join(INC, "ext")) and not os.path.exists(os.path.join(INC, "ext2"))
