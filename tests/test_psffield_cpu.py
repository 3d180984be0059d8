"""Spatially varying blur (`field_blur`, include/osmosis_psffield.h) without a GPU: the float64 oracle of tests/psffield_oracle.py
against itself (the per-pixel definition, the sum over nodes, the gather-form adjoint, autograd), the two field generators, and the
registry: config keys, the refusals, what a field must never be read as; and what of the entry point needs no GPU: its place in
the ABI table and the validation that fails before a launch."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import psffield_oracle as O
from osmosis_diffusion_code_amd import _lib
from osmosis_diffusion_code_amd.guided_diffusion import measurements as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _field(gh, gw, kh, kw, seed):
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((gh, gw, kh, kw)))


def _images(B, P, H, W, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(B, P, H, W, generator=g, dtype=torch.float64), torch.randn(B, P, H, W, generator=g, dtype=torch.float64)


# ------------------------------------------------------------------------------------------------------------ 1: the oracle
# (H, W, gh, gw, kh, kw): ragged sizes; an 8 x 12 image under 9 x 9 kernels on a 2 x 3 grid (both mirrors reach, cells narrower than
# the reach); kh != kw; a grid as fine as the image
ORACLE_CASES = [(13, 17, 2, 2, 5, 5), (8, 12, 2, 3, 9, 9), (20, 27, 3, 4, 3, 7), (6, 7, 6, 7, 3, 3)]


@pytest.mark.parametrize("H,W,gh,gw,kh,kw", ORACLE_CASES)
def test_pixelwise_definition_is_the_sum_over_nodes_and_the_gather_adjoint_is_its_vjp(H, W, gh, gw, kh, kw):
    K = _field(gh, gw, kh, kw, 1)
    x, v = _images(2, 3, H, W, 2)
    a, b = O.forward_pixelwise(x, K), O.forward_sum(x, K)
    assert float((a - b).abs().max()) <= 1e-12
    ga, gb = O.adjoint_gather(v, K), O.adjoint_vjp(v, K)
    assert float((ga - gb).abs().max()) <= 1e-12
    assert abs(float((a * v).sum() - (x * ga).sum())) <= 1e-10


@pytest.mark.parametrize("H,W,gh,gw", [(13, 17, 2, 2), (8, 12, 2, 3), (36, 34, 5, 5), (32, 32, 32, 32), (256, 256, 5, 5)])
def test_hats_are_a_partition_of_unity_on_the_gain_fields_nodes(H, W, gh, gw):
    from osmosis_diffusion_code_amd import ops
    hy, hx = O.hats(H, W, gh, gw)
    assert float((hy.sum(0) - 1).abs().max()) <= 1e-15 and float((hx.sum(0) - 1).abs().max()) <= 1e-15
    assert float((O.hat_field(H, W, gh, gw).sum((0, 1)) - 1).abs().max()) <= 1e-15 and float(hy.min()) >= 0 and float(hx.min()) >= 0
    # a node's hat is 1 at the node itself: node j of a row sits at x = j (W - 1) / (gw - 1) -- exactly on a pixel here when that is an integer
    for j in range(gw):
        pos = j * (W - 1) / (gw - 1)
        if pos == int(pos):
            assert abs(float(hx[j, int(pos)]) - 1.0) <= 1e-6
    # `field_tables` are the gain tables, after the grid limits
    for bad in ((1, 2), (2, 33), (H + 1, 2)):
        with pytest.raises(ValueError, match="node grid"):
            ops.field_tables(H, W, *bad, "cpu")
    tabs = ops.field_tables(H, W, gh, gw, "cpu")
    for got, want in zip(tabs, ops.gain_tables_host(H, W, gh, gw)):
        assert np.array_equal(got.numpy(), want)


def test_a_field_of_identical_nodes_is_psf_blur():
    k = torch.from_numpy(np.random.default_rng(3).standard_normal((5, 7)))
    x, _ = _images(2, 3, 20, 27, 4)
    K = k.expand(3, 4, 5, 7).contiguous()
    assert float((O.forward_pixelwise(x, K) - O.conv_reflect(x, k)).abs().max()) <= 1e-12
    assert float((O.adjoint_gather(x, K) - O.psf_adjoint_gather(x, k)).abs().max()) <= 1e-12


# ------------------------------------------------------------------------------------------------------------ 2: the generators
def _moment(k):
    a = np.arange(k.shape[0]) - k.shape[0] // 2
    return float((k * (a[:, None] ** 2 + a[None, :] ** 2)).sum())


def test_generators_reproduce_the_golden_instance():
    gold = np.load(os.path.join(GOLD, "psf_field.npz"))
    for name, fn in (("radial_defocus", M.radial_defocus_field), ("roll_shake", M.roll_shake_field)):
        kw = {k.split(".", 1)[1]: gold[k].tolist() for k in gold.files if k.startswith(name + ".")}
        got = fn(**kw)
        assert got.shape == gold[name].shape and got.dtype == np.float64
        assert float(np.abs(got - gold[name]).max()) <= 1e-13, name


def test_every_node_is_a_probability_kernel():
    for ks in (M.radial_defocus_field(), M.roll_shake_field(), M.roll_shake_field(kernel_size=9, angle_deg=20.0, grid=(4, 6), image_size=(64, 48))):
        assert ks.min() >= 0.0 and float(np.abs(ks.sum(axis=(2, 3)) - 1.0).max()) <= 1e-12


def test_roll_shake_centre_is_a_delta_and_streaks_grow_with_the_radius():
    ks = M.roll_shake_field(kernel_size=31, angle_deg=3.0, grid=(5, 5), image_size=(256, 256))
    delta = np.zeros((31, 31))
    delta[15, 15] = 1.0
    assert np.array_equal(ks[2, 2], delta)
    # the streak's second moment about the centre grows with the node radius: centre < edge midpoints < corners, on every ray
    m = np.array([[_moment(ks[jy, jx]) for jx in range(5)] for jy in range(5)])
    assert m[2, 2] == 0.0
    assert m[2, 2] < m[2, 3] < m[2, 4] and m[2, 2] < m[3, 2] < m[4, 2] and m[2, 2] < m[3, 3] < m[4, 4] and m[2, 4] < m[4, 4]
    # tangential: the node right of the centre is streaked vertically, the node below it horizontally
    assert ks[2, 4].sum(axis=0)[15] == pytest.approx(1.0) and ks[4, 2].sum(axis=1)[15] == pytest.approx(1.0)
    # length = angle r: the corner node at r = 127.5 sqrt 2 under 3 degrees spans 9.44 px, i.e. 9 samples of MOTION_STEP each way
    n = int(np.floor(np.deg2rad(3.0) * 127.5 * np.sqrt(2.0) / (2 * M.MOTION_STEP)))
    reach = n * M.MOTION_STEP / np.sqrt(2.0)
    iy, ix = np.nonzero(ks[0, 0])
    assert np.abs(iy - 15).max() == int(np.ceil(reach)) and np.abs(ix - 15).max() == int(np.ceil(reach))


def test_radial_defocus_second_moment_is_monotone_in_rho():
    gh, gw = 5, 7
    ks = M.radial_defocus_field(kernel_size=31, sigma_center=0.5, sigma_corner=3.0, grid=(gh, gw))
    rho = np.array([[np.sqrt(((2 * jy / (gh - 1) - 1) ** 2 + (2 * jx / (gw - 1) - 1) ** 2) / 2) for jx in range(gw)] for jy in range(gh)])
    m = np.array([[_moment(ks[jy, jx]) for jx in range(gw)] for jy in range(gh)])
    order = np.argsort(rho.reshape(-1), kind="stable")
    r, mm = rho.reshape(-1)[order], m.reshape(-1)[order]
    for a in range(len(r) - 1):
        assert (mm[a + 1] > mm[a]) if r[a + 1] > r[a] + 1e-12 else abs(mm[a + 1] - mm[a]) <= 1e-9
    assert rho.min() == 0.0 and rho.max() == pytest.approx(1.0)
    assert _moment(ks[gh // 2, gw // 2]) == pytest.approx(2 * 0.25, rel=0.15)          # sigma 0.5, sampled: about 2 sigma^2


def test_generators_refuse_bad_arguments():
    for fn, kw in ((M.radial_defocus_field, dict(kernel_size=8)), (M.radial_defocus_field, dict(kernel_size=63)),
                   (M.radial_defocus_field, dict(sigma_center=0.0)), (M.radial_defocus_field, dict(grid=(1, 5))),
                   (M.radial_defocus_field, dict(grid=(5, 33))), (M.roll_shake_field, dict(angle_deg=-1.0)),
                   (M.roll_shake_field, dict(angle_deg=float("nan"))), (M.roll_shake_field, dict(image_size=(1, 5))),
                   (M.roll_shake_field, dict(image_size=5)), (M.roll_shake_field, dict(grid=5))):
        with pytest.raises(ValueError, match="field_blur"):
            fn(**kw)


# ------------------------------------------------------------------------------------------------------------ 3: the registry
def _op(**kw):
    return M.get_operator("field_blur", device="cpu", **kw)


def test_field_blur_is_registered_as_a_psf_operator_and_the_grid_operators_stay():
    assert M.__OPERATOR__["field_blur"] is M.PSFFieldOperator and issubclass(M.PSFFieldOperator, M.PSFOperator)
    assert M.GRID_OPERATORS == (M.SeparableOperator, M.PSFOperator)
    from osmosis_diffusion_code_amd import torch_ops
    assert "psf_field_apply" in torch_ops.OPS and "psf_field_apply" not in torch_ops.OPS_C
    assert str(torch.ops.osmosis.psf_field_apply.default._schema) == (
        "osmosis::psf_field_apply(Tensor x, Tensor dy, Tensor dx, Tensor w, Tensor iy0, Tensor fy, Tensor ix0, Tensor fx, SymInt Ry, SymInt Rx, "
        "bool adjoint) -> Tensor")
    with pytest.raises((NotImplementedError, RuntimeError)):          # no CPU kernel: the product path fails loudly
        _op(model="radial_defocus", kernel_size=5, grid=[2, 2]).forward(torch.zeros(1, 3, 8, 8))


def test_config_keys_and_methods(tmp_path):
    ks = np.random.default_rng(5).random((2, 3, 3, 5))
    ks[0, 1, 0, 0] = ks[1, 2, 2, 4] = 0.0
    ks[:, :, 1, 2] = 0.0                                          # a tap no node has: not in the union
    op = _op(kernels=ks.tolist())
    assert op.grid == (2, 3) and op.weight_sets == (1, 1) and op.model is None
    k = op.kernels()
    assert k.shape == (2, 3, 3, 5) and k.dtype == np.float64 and np.allclose(k, ks / ks.sum(axis=(2, 3), keepdims=True), rtol=0, atol=1e-15)
    k[0, 0] = 7.0
    assert not np.array_equal(op.kernels(), k)                   # a copy
    assert np.array_equal(_op(kernels=ks, normalize=False).kernels(), ks)
    np.save(tmp_path / "f.npy", ks)
    assert np.array_equal(_op(kernels=str(tmp_path / "f.npy")).kernels(), op.kernels())
    assert np.array_equal(_op(kernels=torch.from_numpy(ks)).kernels(), op.kernels())
    dy, dx, w = op.host_taps()
    iy, ix = np.nonzero((ks != 0).any(axis=(0, 1)))
    assert len(dy) == 14 and np.array_equal(dy, iy - 1) and np.array_equal(dx, ix - 2) and dy.dtype == dx.dtype == np.int32
    assert w.shape == (2, 3, 14) and w.dtype == np.float32 and np.array_equal(w, op.kernels()[:, :, iy, ix].astype(np.float32))
    assert w[0, 1, 0] == 0.0 and op.radius() == (1, 2)
    with pytest.raises(ValueError, match=r"kernels\(\)"):
        op.kernel2d()
    assert op.out_shape(8, 9) == (8, 9)
    with pytest.raises(ValueError, match="reflection"):
        _op(kernels=np.ones((2, 2, 3, 7))).out_shape(8, 3)
    with pytest.raises(ValueError, match="node grid"):
        _op(model="radial_defocus", kernel_size=3, grid=[5, 5]).out_shape(4, 9)
    for a, b in zip(op.field_tables(8, 9), __import__("osmosis_diffusion_code_amd").ops.gain_tables_host(8, 9, 2, 3)):
        assert np.array_equal(a.numpy(), b)
    # the models, their defaults and their keys
    rd = _op(model="radial_defocus")
    assert rd.grid == (5, 5) and np.array_equal(rd.kernels(), M.radial_defocus_field()) and rd.radius() == (15, 15)
    rs = _op(model="roll_shake", kernel_size=9, angle_deg=2.0, grid=[3, 4], image_size=[64, 96], simulate=False)
    assert np.array_equal(rs.kernels(), M.roll_shake_field(9, 2.0, (3, 4), (64, 96))) and rs.model == "roll_shake"


@pytest.mark.parametrize("kw,match", [
    (dict(), "either"), (dict(kernels=np.ones((2, 2, 3, 3)), model="roll_shake"), "either"), (dict(model="zoom"), "model must be"),
    (dict(model="roll_shake", sigma_center=1.0), "unknown config key"), (dict(model="radial_defocus", image_size=[8, 8]), "unknown config key"),
    (dict(kernels=np.ones((2, 2, 3, 3)), grid=[2, 2]), "unknown config key"), (dict(kernels=np.ones((2, 2, 3, 3)), kernel_size=3), "unknown config key"),
    (dict(kernels=np.ones((2, 2, 3, 3)), per_image=True), "per_image"), (dict(model="roll_shake", per_channel=False), "per_channel"),
    (dict(kernels=np.ones((2, 3, 3))), "gh,gw,kh,kw"), (dict(kernels=np.ones((1, 2, 3, 3))), "grid"), (dict(kernels=np.ones((2, 33, 3, 3))), "grid"),
    (dict(kernels=np.ones((2, 2, 4, 3))), "odd"), (dict(kernels=np.full((2, 2, 3, 3), np.nan)), "non-finite"),
    (dict(kernels=np.ones((2, 2, 63, 3))), "larger than"), (dict(kernels="nope"), "array of numbers"),
    (dict(kernels=np.stack([np.ones((2, 3, 3)), np.zeros((2, 3, 3))])), "all zero"),
    (dict(kernels=np.stack([np.ones((2, 3, 3)), np.tile(np.array([[0, 1.0, 0], [0, -1.0, 0], [0, 0, 0]]), (2, 1, 1))])), "normalize")])
def test_bad_configs_raise_naming_field_blur(kw, match):
    with pytest.raises(ValueError, match=match) as e:
        _op(**kw)
    assert "field_blur" in str(e.value)


def test_a_field_is_refused_where_one_psf_is_expected():
    """Before any launch, by name: as a `degradation` of the water / haze operators (config dict or instance), in `lin_desc` and
    `lin_config`; tiling and `set_robust` refuse it as they refuse every grid operator."""
    from osmosis_diffusion_code_amd import _lib, ops, torch_ops
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods as CM
    op = _op(model="radial_defocus", kernel_size=5, grid=[2, 2])
    for deg in (dict(name="field_blur", model="radial_defocus"), op):
        with pytest.raises(ValueError, match="field_blur"):
            M.build_degradation(deg, "cpu")
    with pytest.raises(ValueError, match="field_blur"):
        M.get_operator("haze_physical", device="cpu", phi_ab="1,1,1", phi_inf="0.5,0.5,0.5", degradation=dict(name="field_blur", model="roll_shake"))
    with pytest.raises(_lib.OsmosisHipError, match="field_blur"):
        ops.lin_desc(op, 16, 16, "cpu")
    with pytest.raises(_lib.OsmosisHipError, match="field_blur"):
        torch_ops.lin_config(op, 16, 16, "cpu")
    cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="grid operator"):
        cond.set_robust("tukey")
    assert cond.hip_ok(3) and not CM.get_conditioning_method("ps", op, M.get_noise("poisson", rate=1.0), scale="0.3").hip_ok(3)
    # the driver knows the measurement's grid without a device
    from osmosis_diffusion_code_amd import sampling
    assert sampling.measurement_grid(dict(name="field_blur", model="radial_defocus", kernel_size=5, grid=[2, 2]), (16, 24)) == (16, 24)


def test_kernel_picture_of_a_field_is_the_mosaic_over_the_common_maximum():
    from osmosis_diffusion_code_amd import sampling
    ks = np.zeros((2, 3, 3, 5))
    ks[0, 0, 1, 2], ks[1, 2, 0, 4], ks[0, 1, 2, 0] = 1.0, 0.5, 0.25
    pic = sampling.kernel_image_u8(torch.from_numpy(ks), side=30)
    z = 30 // 15
    assert pic.shape == (2 * 3 * z, 3 * 5 * z) and pic.dtype == np.uint8
    want = np.zeros((6, 15), dtype=np.uint8)
    want[1, 2], want[3 + 0, 10 + 4], want[2, 5 + 0] = 255, 128, 64
    assert np.array_equal(pic, np.repeat(np.repeat(want, z, axis=0), z, axis=1))


# ------------------------------------------------------------------------------------------------------------ 4: the entry point
def test_entry_point_takes_the_stream_last_and_its_header_has_no_struct():
    # the stream stays the last argument of a launching entry point: a Recorder re-targets it on capture
    assert _lib.exports("osmosis_psffield.h") == ["osm_psf_field_apply"] and _lib.SIGS["osm_psf_field_apply"][-1] is ctypes.c_void_p
    header = open(os.path.join(ROOT, "include", "osmosis_psffield.h")).read()
    assert "struct" not in re.sub(r"/\*.*?\*/", " ", header, flags=re.S)


def test_the_loaded_library_binds_the_entry_point_to_the_table():
    lib = _lib.load()
    assert lib is _lib.load()
    fn, argtypes = lib.osm_psf_field_apply, _lib.SIGS["osm_psf_field_apply"]
    assert fn.argtypes == argtypes and len(argtypes) == 23 and fn.restype is ctypes.c_int


def test_a_null_pointer_fails_validation_and_leaves_its_text_in_osm_last_error():
    """A null pointer fails through validation: nothing is launched, so no GPU is needed."""
    lib = _lib.load()
    null = [None] * 5 + [1, 0, 0, 2, 2] + [None] * 4 + [1, 3, 48, 48, 4, 4, 0, 0, None]
    with pytest.raises(_lib.OsmosisHipError, match=r"osm_psf_field_apply failed \(-1\): osm_psf_field_apply: null pointer"):
        _lib.call("osm_psf_field_apply", *null)
    assert lib.osm_last_error().decode().startswith("osm_psf_field_apply: null pointer")
    assert _lib.last_error("osm_psf_field_apply") == lib.osm_last_error().decode()
    # ... one text for the library: a later failure of another entry point replaces it
    with pytest.raises(_lib.OsmosisHipError, match="osm_psf_apply"):
        _lib.call("osm_psf_apply", *([None] * 5), 1, 0, 0, 1, 3, 48, 48, 4, 4, 0, 0, None)
    assert lib.osm_last_error().decode().startswith("osm_psf_apply")
    assert _lib.last_error("osm_psf_field_apply") == lib.osm_last_error().decode()
    with pytest.raises(_lib.OsmosisHipError, match="osm_nothing"):
        _lib.call("osm_nothing")
    # a Recorder sees nothing of a failed call
    with _lib.Recorder() as rec:
        with pytest.raises(_lib.OsmosisHipError):
            _lib.call("osm_psf_field_apply", *null)
    assert len(rec) == 0
