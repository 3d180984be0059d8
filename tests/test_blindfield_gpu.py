"""Blind spatially varying deblurring on the GPU (operator `blind_field_blur`, include/osmosis_blindfield.h): the per-node
tap-gradient kernel bit for bit against osm_psf_tap_grad on q_n = fl(hat_n r) and against the float64 oracle of
tests/blindfield_oracle.py, the step of every node against the numpy restatement and against osm_psf_tap_step, the data term
`loss_grad_x0` with its inner loop, the recovery of a known field, the fused sampler loop against `_generic_loop` and against the
oracle's chain, and `restore_image`.

Tap-gradient bar (the header's): a partial is an fp32 chain of at most 1024 fmas on q_n = fl(fl(haty hatx) r) with a = fl(1 - fx),
b = fl(1 - fy): four roundings in q_n (three of them count against float64 hats that are exact products of the fp32 fractions), so
per tap |err| <= (1024 + 3) 2^-24 sum hat_n |r| |x|; the partials are added in fp64.

Field-estimate bar: 5 x the distance between the float64 oracle and the SAME oracle with its image side in float32 on the CPU."""
import os

import numpy as np
import pytest
import torch

import blind_oracle as BO
import blindfield_oracle as O
import psffield_oracle as FO
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from test_blind_gpu import (CHAIN_CASES, GOLD, H0, MEASURED_RGB, PATTERN, RGB_KW, TINY_KW, W0, _free_running_bar, _no_generic,
                            _replay_p_sample_draws, chain_inputs, make_model, make_sampler, term_inputs)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


@pytest.fixture(scope="module")
def model36(pkg):
    return make_model(pkg[0], RGB_KW)


@pytest.fixture(scope="module")
def model48(pkg):
    return make_model(pkg[0], TINY_KW)


# ------------------------------------------------------------------------------------------------------------ 1: the tap gradient
def _dense(kh, kw):
    dy, dx = np.repeat(np.arange(kh) - kh // 2, kw).astype(np.int32), np.tile(np.arange(kw) - kw // 2, kh).astype(np.int32)
    return dy, dx, kh, kw


# case -> (H, W, (gh, gw), (kh, kw))
TAP_CASES = {"tiles5": (36, 34, (2, 2), (5, 5)),                 # two tiles per axis, ragged tails
             "asym3x7": (40, 72, (3, 4), (3, 7)),
             "both_mirrors": (8, 12, (2, 3), (9, 9)),            # smaller than a tile, both mirrors, cells narrower than the reach
             "nine_tiles": (70, 66, (5, 5), (9, 9)),             # nine tiles, ragged, nodes spanning several
             "dense_grid": (36, 34, (32, 32), (3, 3)),           # about a thousand nodes on a tile
             "dense61": (64, 64, (2, 2), (61, 61))}              # the LDS-capacity case, T = 3721 > 256 lanes
_TAPREF = {}


def tap_inputs(case):
    if case not in _TAPREF:
        H, W, grid, (kh, kw) = TAP_CASES[case]
        dy, dx, _, _ = _dense(kh, kw)
        g = torch.Generator().manual_seed(17)
        x, r = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
        _TAPREF[case] = dict(H=H, W=W, grid=grid, k=(kh, kw), dy=dy, dx=dx, R=(kh // 2, kw // 2), x=x, r=r)
    return _TAPREF[case]


def tap_reference(case):
    """The float64 c_n [2,gh,gw,T] of a case and the magnitude sum hat_n |r| |x|, once."""
    ref = tap_inputs(case)
    if "c" not in ref:
        (gh, gw), (kh, kw) = ref["grid"], ref["k"]
        x64, r64 = ref["x"][:, 0:3].double(), ref["r"].double()
        ref["c"] = O.tap_corr(r64, x64, gh, gw, kh, kw).reshape(2, gh, gw, -1)
        ref["mag"] = O.tap_corr(r64.abs(), x64.abs(), gh, gw, kh, kw).reshape(2, gh, gw, -1)
    return ref


def run_field_tap_grad(ref, x, r, R=None):
    """osm_field_tap_grad into a NaN-filled workspace -> part [B, NP, T] (device)."""
    from osmosis_diffusion_code_amd import ops
    B, C, H, W = x.shape[0], x.shape[1], ref["H"], ref["W"]
    gh, gw = ref["grid"]
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, 3, DEV)
    part = torch.full((B, NP, dy.numel()), float("nan"), device=DEV)
    ops.field_tap_grad(x, r, dy, dx, ops.field_tables(H, W, gh, gw, DEV), lay, NP, gh, gw, *(R or ref["R"]), B, 3, C * H * W, 3 * H * W,
                       H, W, part)
    return part


def node_sums(ref, part):
    """c_n [B,gh,gw,T] float64 (CPU) of part [B,NP,T]: every node's partials added in layout order."""
    from osmosis_diffusion_code_amd import ops
    gh, gw = ref["grid"]
    off = ops.field_tap_layout(ref["H"], ref["W"], gh, gw, 3)[2][2 * gh + 2 * gw:]
    p = part.double().cpu()
    return torch.stack([p[:, off[n]:off[n + 1]].sum(dim=1) for n in range(gh * gw)], dim=1).reshape(p.shape[0], gh, gw, -1)


def fp32_hats(H, W, gh, gw):
    """(haty fp32 [gh,H], hatx fp32 [gw,W]) on the device, as the header defines them: a = fl(1 - f) where the cell is the node's, f
    where it is the one before, 0 (absent) elsewhere."""
    from osmosis_diffusion_code_amd import ops
    iy0, fy, ix0, fx = ops.field_tables(H, W, gh, gw, DEV)

    def axis(i0, f, g):
        j = torch.arange(g, device=DEV)[:, None]
        zero = torch.zeros((), device=DEV)
        return torch.where(i0[None, :] == j, 1.0 - f[None, :], torch.where(i0[None, :] == j - 1, f[None, :], zero))
    return axis(iy0, fy, gh), axis(ix0, fx, gw)


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", list(TAP_CASES))
def test_tap_gradient_is_bit_equal_to_psf_tap_grad_on_q_n(pkg, case, C):
    """Node by node and tile by tile: the partial of (node, plane, tile) is what osm_psf_tap_grad writes for that tile when handed
    q_n = fl(hat_n r) built in torch fp32 in r's place; outside the node's tile rectangle osm_psf_tap_grad's partials are zero.  A
    repeat, and the batch as two calls of one image: the same bits."""
    from osmosis_diffusion_code_amd import ops
    ref = tap_inputs(case)
    H, W, (gh, gw) = ref["H"], ref["W"], ref["grid"]
    x, r = ref["x"][:, 0:C].contiguous().to(DEV), ref["r"].to(DEV)
    part = run_field_tap_grad(ref, x, r)
    assert bool(torch.isfinite(part).all()), "a partial was not written"
    _, NP, lay = ops.field_tap_layout(H, W, gh, gw, 3)
    ty0, ty1, tx0, tx1, off = lay[:gh], lay[gh:2 * gh], lay[2 * gh:2 * gh + gw], lay[2 * gh + gw:2 * gh + 2 * gw], lay[2 * gh + 2 * gw:]
    nty, ntx = -(-H // 32), -(-W // 32)
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    haty, hatx = fp32_hats(H, W, gh, gw)
    full = torch.empty(2, 3 * nty * ntx, dy.numel(), device=DEV)
    bad = []
    for jy in range(gh):
        for jx in range(gw):
            n = jy * gw + jx
            q = (haty[jy][:, None] * hatx[jx][None, :]) * r                                   # ONE fp32 product for the hat, one with r
            ops.psf_tap_grad(x, q.contiguous(), dy, dx, *ref["R"], 2, 3, C * H * W, 3 * H * W, H, W, full)
            tiles = full.view(2, 3, nty, ntx, -1)
            mine = part[:, off[n]:off[n + 1]].view(2, 3, ty1[jy] - ty0[jy], tx1[jx] - tx0[jx], -1)
            inside = tiles[:, :, ty0[jy]:ty1[jy], tx0[jx]:tx1[jx]]
            if not torch.equal(mine, inside) or int((tiles != 0).sum()) != int((inside != 0).sum()):
                bad.append((jy, jx))
    assert not bad, (case, bad[:8])
    assert torch.equal(run_field_tap_grad(ref, x, r), part)
    for b in range(2):
        assert torch.equal(run_field_tap_grad(ref, x[b:b + 1].contiguous(), r[b:b + 1].contiguous())[0], part[b])


@pytest.mark.parametrize("case", list(TAP_CASES))
def test_tap_gradient_vs_float64_under_the_derived_bound(pkg, case):
    ref = tap_reference(case)
    part = run_field_tap_grad(ref, ref["x"].to(DEV), ref["r"].to(DEV))
    c = node_sums(ref, part)
    bound = (1024 + 3) * U24 * ref["mag"]
    err = (c - ref["c"]).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"FIELDTAP {case}: worst |err| / bound {ratio:.4f} (max |err| {float(err.max()):.2e}, nodes {c.shape[1] * c.shape[2]}, T {c.shape[3]})")
    assert ratio <= 1.0, (case, ratio)
    # the node partials add up to blind's c (the hats sum to one), within both bounds
    from osmosis_diffusion_code_amd import ops
    H, W = ref["H"], ref["W"]
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    plain = torch.empty(2, ops.tap_grad_nparts(3, H, W), dy.numel(), device=DEV)
    ops.psf_tap_grad(ref["x"].to(DEV), ref["r"].to(DEV), dy, dx, *ref["R"], 2, 3, 4 * H * W, 3 * H * W, H, W, plain)
    both = (2 * 1024 + 5) * U24 * ref["mag"].sum(dim=(1, 2))
    assert bool(((c.sum(dim=(1, 2)) - plain.double().sum(dim=1).cpu()).abs() <= both).all())


def test_tap_gradient_is_exact_on_small_integers(pkg):
    """33 x 33 under 5 x 5 nodes: the fractions are multiples of 1/8, so every hat is a multiple of 1/64, exact in fp32; with x and r
    integers in [-3, 3] every product and every partial sum of a tile is a multiple of 1/64 of magnitude at most 1024 x 9 (a
    numerator below 2^20), exact in fp32 whatever the order, so each PARTIAL must equal the float64 sum over its tile bit for bit: a
    single wrong pixel or hat shows."""
    from osmosis_diffusion_code_amd import ops
    H = W = 33
    gh = gw = 5
    dy, dx, kh, kw = _dense(5, 5)
    ref = dict(H=H, W=W, grid=(gh, gw), dy=dy, dx=dx, R=(2, 2))
    g = torch.Generator().manual_seed(23)
    x = torch.randint(-3, 4, (2, 4, H, W), generator=g).float()
    r = torch.randint(-3, 4, (2, 3, H, W), generator=g).float()
    _, fy, _, fx = ops.gain_tables_host(H, W, gh, gw)
    assert np.array_equal(fy * 8, np.round(fy * 8)) and np.array_equal(fx * 8, np.round(fx * 8))
    part = run_field_tap_grad(ref, x.to(DEV), r.to(DEV)).cpu().double()
    _, NP, lay = ops.field_tap_layout(H, W, gh, gw, 3)
    ty0, ty1, tx0, tx1, off = lay[:gh], lay[gh:2 * gh], lay[2 * gh:2 * gh + gw], lay[2 * gh + gw:2 * gh + 2 * gw], lay[2 * gh + 2 * gw:]
    seen = 0
    for p in range(3):
        for ty in range(2):
            for tx in range(2):
                rt = torch.zeros(2, 1, H, W, dtype=torch.float64)
                rt[:, 0, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32] = r[:, p, 32 * ty:32 * ty + 32, 32 * tx:32 * tx + 32].double()
                want = O.tap_corr_direct(rt, x[:, p:p + 1].double(), gh, gw, dy, dx)        # [2,gh,gw,T]
                for jy in range(gh):
                    for jx in range(gw):
                        if ty0[jy] <= ty < ty1[jy] and tx0[jx] <= tx < tx1[jx]:
                            n = jy * gw + jx
                            slot = off[n] + (p * (ty1[jy] - ty0[jy]) + ty - ty0[jy]) * (tx1[jx] - tx0[jx]) + tx - tx0[jx]
                            assert np.array_equal(part[:, slot].numpy(), want[:, jy, jx]), (p, ty, tx, jy, jx)
                            seen += 1
                        else:
                            assert not want[:, jy, jx].any(), (p, ty, tx, jy, jx)            # a node that does not reach the tile adds nothing
    assert seen == NP


@pytest.mark.parametrize("case", ["tiles5", "both_mirrors", "nine_tiles"])
def test_linearity_identity_against_psf_field_apply(pkg, case):
    """<r, A(w) x> = sum_n sum_t w_n[t] c_n[t], both sides from the kernels, within the two derived bounds."""
    from osmosis_diffusion_code_amd import ops
    ref = tap_reference(case)
    H, W, (gh, gw), T = ref["H"], ref["W"], ref["grid"], len(ref["dy"])
    x, r = ref["x"].to(DEV), ref["r"].to(DEV)
    w = torch.rand(gh, gw, T, generator=torch.Generator().manual_seed(3)) - 0.3
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    Ax = torch.empty(2, 3, H, W, device=DEV)
    ops.psf_field_apply(x, Ax, dy, dx, w.to(DEV), ops.field_tables(H, W, gh, gw, DEV), *ref["R"], 2, 3, 4 * H * W, 3 * H * W, H, W)
    lhs = (ref["r"].double() * Ax.cpu().double()).sum(dim=(1, 2, 3))
    c = node_sums(ref, run_field_tap_grad(ref, x, r))
    rhs = (c * w.double()[None]).sum(dim=(1, 2, 3))
    mag = (ref["mag"] * w.double().abs()[None]).sum(dim=(1, 2, 3))                       # sum_n hat_n |r| |w_n| |x|
    bound = ((T + 8) + (1024 + 3)) * U24 * mag
    print(f"FIELDTAP identity {case}: |lhs - rhs| / bound {float(((lhs - rhs).abs() / bound).max()):.4f}")
    assert bool(((lhs - rhs).abs() <= bound).all())


def test_a_tap_beyond_the_radius_is_written_as_zero_and_bad_arguments_launch_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    ref = tap_inputs("nine_tiles")
    H, W, (gh, gw) = ref["H"], ref["W"], ref["grid"]
    x, r = ref["x"].to(DEV), ref["r"].to(DEV)
    full = run_field_tap_grad(ref, x, r)
    cut = run_field_tap_grad(ref, x, r, R=(4, 2))                         # the list's |dx| reaches 4
    out = torch.from_numpy(np.abs(ref["dx"]) > 2)
    assert float(cut[:, :, out].abs().max()) == 0.0 and not bool(torch.signbit(cut[:, :, out]).any())
    assert torch.equal(cut[:, :, ~out], full[:, :, ~out])
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, 3, DEV)
    tabs = ops.field_tables(H, W, gh, gw, DEV)
    part = torch.full((2, NP, 81), float("nan"), device=DEV)
    lib, p = _lib.load(), _lib.ptr
    good = [p(x), p(r), p(dy), p(dx), 81, 4, 4, gh, gw] + [p(t) for t in tabs] + [p(lay), 2, 3, 4 * H * W, 3 * H * W, H, W, p(part), None]
    for pos, val in ((0, None), (20, None), (13, None), (9, None), (4, 0), (4, 4226), (5, 33), (5, H), (6, W), (7, 1), (8, 33), (7, H + 1),
                     (14, 0), (15, 0), (16, 10), (17, 10)):
        args = list(good)
        args[pos] = val
        assert lib.osm_field_tap_grad(*args) == -1 and lib.osm_last_error().decode().startswith("osm_field_tap_grad"), (pos, val)
    torch.cuda.synchronize()
    assert bool(torch.isnan(part).all())
    with pytest.raises(_lib.OsmosisHipError, match="smaller"):
        ops.field_tap_grad(x, r, dy, dx, tabs, lay, NP, gh, gw, 4, 4, 3, 3, 4 * H * W, 3 * H * W, H, W, part)
    with pytest.raises(_lib.OsmosisHipError, match="layout"):
        ops.field_tap_grad(x, r, dy, dx, tabs, lay[:-1].contiguous(), NP, gh, gw, 4, 4, 2, 3, 4 * H * W, 3 * H * W, H, W, part)
    with pytest.raises(_lib.OsmosisHipError, match="partial count"):
        ops.field_tap_grad(x, r, dy, dx, tabs, lay, NP - 1, gh, gw, 4, 4, 2, 3, 4 * H * W, 3 * H * W, H, W, part)
    assert lib.osm_field_tap_grad(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(part, full)


# ------------------------------------------------------------------------------------------------------------ 2: the step
def _step_case(T, B, grid, seed):
    """A random field, random partials in the layout of a 70 x 66 image under `grid`, losses."""
    from osmosis_diffusion_code_amd import ops
    gh, gw = grid
    lay, NP, host = ops.field_tap_layout(70, 66, gh, gw, 3, DEV)
    rng = np.random.default_rng(seed)
    w = rng.random((gh, gw, T)).astype(np.float32)
    w /= w.sum(axis=2, keepdims=True)
    part = rng.standard_normal((B, NP, T)).astype(np.float32)
    loss = (rng.random(B) + 0.5).astype(np.float32)
    return w, part, loss, lay, NP, host[2 * gh + 2 * gw:]


def _c_of(part, off, gh, gw):
    """c [B,gh,gw,T] float64: every node's partials added ascending, as the header states."""
    c = np.zeros((part.shape[0], gh * gw, part.shape[2]))
    for n in range(gh * gw):
        for q in range(off[n], off[n + 1]):
            c[:, n] = c[:, n] + part[:, q].astype(np.float64)
    return c.reshape(part.shape[0], gh, gw, -1)


def run_field_step(w, part, loss, lay, NP, hw3, eta, l1, smooth):
    from osmosis_diffusion_code_amd import ops
    wd = torch.from_numpy(w.copy()).to(DEV)
    scratch = torch.full_like(wd, float("nan"))
    ops.field_tap_step(wd, scratch, torch.from_numpy(part).to(DEV), torch.from_numpy(loss).to(DEV), lay, NP, part.shape[0], hw3, eta, l1, smooth)
    assert torch.equal(scratch, wd)                                      # every element of the workspace was written, then copied
    return wd.cpu().numpy()


@pytest.mark.parametrize("smooth", [0.0, 0.3])
@pytest.mark.parametrize("T,B,grid", [(25, 2, (2, 2)), (81, 1, (3, 4)), (1024, 3, (2, 2)), (3721, 2, (5, 5))])
def test_step_vs_the_numpy_step(pkg, T, B, grid, smooth):
    """At most 1 fp32 ulp per tap (measured: 0), exact where u = 0; l1 > 0 and a large eta so that about half the taps clamp.  With
    smooth = 0 every node is bit for bit osm_psf_tap_step on its partials repacked as [B][nparts][T]."""
    from osmosis_diffusion_code_amd import ops
    gh, gw = grid
    w, part, loss, lay, NP, off = _step_case(T, B, grid, T)
    hw3, eta = 3 * 70 * 66, 400.0                                       # large enough for the step to reach the clamp
    l1 = 0.2 / (eta * T)                                                # a shrinkage of a fifth of the mean weight
    want = O.step(w, _c_of(part, off, gh, gw), loss, hw3, eta, l1, smooth)
    got = run_field_step(w, part, loss, lay, NP, hw3, eta, l1, smooth)
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-30))).astype(np.float64)
    clamped = float((want == 0).mean())
    print(f"FIELDSTEP T={T} B={B} {gh}x{gw} smooth={smooth}: worst {ulps.max():.2f} ulp, {clamped:.2f} of the taps clamped")
    assert 0.2 <= clamped <= 0.8 and not np.array_equal(want, w)
    assert ulps.max() <= 1.0 and np.all(got[want == 0] == 0.0)
    assert np.abs(got.astype(np.float64).sum(axis=2) - 1.0).max() <= 1e-6 and (got >= 0).all()
    if smooth == 0.0:
        for n in range(gh * gw):
            wn = torch.from_numpy(w[n // gw, n % gw].copy()).to(DEV)
            rep = torch.from_numpy(np.ascontiguousarray(part[:, off[n]:off[n + 1]])).to(DEV)
            ops.psf_tap_step(wn, rep, torch.from_numpy(loss).to(DEV), B, int(off[n + 1] - off[n]), hw3, eta, l1)
            assert np.array_equal(wn.cpu().numpy(), got[n // gw, n % gw]), n
    else:
        assert not np.array_equal(got, run_field_step(w, part, loss, lay, NP, hw3, eta, l1, 0.0))


@pytest.mark.parametrize("smooth", [0.0, 0.3])
def test_step_guards_leave_that_node_alone_while_its_neighbours_step(pkg, smooth):
    gh, gw = 3, 4
    w, part, loss, lay, NP, off = _step_case(81, 2, (gh, gw), 5)
    hw3 = 3 * 70 * 66
    clean = run_field_step(w, part, loss, lay, NP, hw3, 40.0, 0.0, smooth)
    assert all(not np.array_equal(clean[jy, jx], w[jy, jx]) for jy in range(gh) for jx in range(gw))
    for n, bad in ((5, np.nan), (0, np.inf), (11, -np.inf)):
        pb = part.copy()
        pb[1, off[n] + 1, 7] = bad
        got = run_field_step(w, pb, loss, lay, NP, hw3, 40.0, 0.0, smooth)
        for m in range(gh * gw):                                         # (the neighbours read w, which the guard never changed)
            assert np.array_equal(got[m // gw, m % gw], w[m // gw, m % gw] if m == n else clean[m // gw, m % gw]), (n, m)
    assert np.array_equal(run_field_step(w, part, loss, lay, NP, hw3, 0.1, 1e9, smooth), w)        # every u clamped to 0, at every node
    lb = loss.copy()
    lb[1] = np.nan
    assert np.array_equal(run_field_step(w, part, lb, lay, NP, hw3, 0.1, 0.0, smooth), w)


def test_opcheck_of_the_two_operators(pkg):
    from osmosis_diffusion_code_amd import ops
    ref = tap_inputs("tiles5")
    H, W, (gh, gw) = ref["H"], ref["W"], ref["grid"]
    x, r = ref["x"][:, 0:3].contiguous().to(DEV), ref["r"].to(DEV)
    dy, dx = torch.from_numpy(ref["dy"]).to(DEV), torch.from_numpy(ref["dx"]).to(DEV)
    tabs = ops.field_tables(H, W, gh, gw, DEV)
    args = (x, r, dy, dx, *tabs, gh, gw, 2, 2)
    torch.library.opcheck(torch.ops.osmosis.field_tap_grad.default, args)
    part = torch.ops.osmosis.field_tap_grad(*args)
    assert torch.equal(part, run_field_tap_grad(ref, x, r))
    w = torch.rand(gh, gw, 25, device=DEV)
    w /= w.sum(dim=2, keepdim=True)
    loss = torch.tensor([0.7, 1.1], device=DEV)
    torch.library.opcheck(torch.ops.osmosis.field_tap_step.default, (w.clone(), part, loss, H, W, 3, 2.0, 0.0, 0.1))
    w1 = w.clone()
    torch.ops.osmosis.field_tap_step(w1, part, loss, H, W, 3, 2.0, 0.0, 0.1)
    lay, NP, _ = ops.field_tap_layout(H, W, gh, gw, 3, DEV)
    assert np.array_equal(w1.cpu().numpy(), run_field_step(w.cpu().numpy(), part.cpu().numpy(), loss.cpu().numpy(), lay, NP, 3 * H * W, 2.0, 0.0, 0.1))
    assert not torch.equal(w1, w)


# ------------------------------------------------------------------------------------------------------------ 3: the data term
def field_cond(pkg, B=1, third_party=False, **okw):
    _, _, M, CM = pkg
    kw = dict(kernel_size=5, grid=[3, 3], n_iter=3, eta=0.5, init_sigma=1.0)
    kw.update(okw)
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    return cls(M.get_operator("blind_field_blur", device=DEV, batch_size=B, **kw), M.get_noise("gaussian", sigma=0.0), scale="0.3")


def field_bar(x0, y, mask, w0, k, n_iter, eta, l1=0.0, smooth=0.0):
    """(float64 oracle result, 5 x its distance to the float32 evaluation of the same oracle, that distance)."""
    r64 = O.inner_loop(x0, y, mask, w0, k, k, n_iter, eta, l1, smooth)
    r32 = O.inner_loop(x0, y, mask, w0, k, k, n_iter, eta, l1, smooth, dtype=torch.float32)
    d = float(np.abs(r64["w"].astype(np.float64) - r32["w"].astype(np.float64)).max())
    return r64, 5.0 * d, d


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
def test_data_term_with_three_inner_iterations_vs_the_oracle(pkg, masked, C):
    """B = 2 at 36 x 34, k = 5, 3 x 3 nodes, n_iter = 3, smooth > 0: loss (2e-6 relative) and x0-gradient (2e-7 + 1e-5 max |want|) at the
    identity term's bars, the field after three steps under `field_bar`; a repeat from reset() bit for bit; `learn: False` against
    field_blur with the init field, bit for bit."""
    _, _, M, CM = pkg
    B, H, W = 2, 36, 34
    x0, y, mask = term_inputs(B, C, H, W, masked)
    cond = field_cond(pkg, B, eta=4.0, smooth=0.05)
    op = cond.operator
    if masked:
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    w0 = op.host_taps()[2]
    g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g, loss, w = g.clone(), loss.clone(), op.taps(DEV)[2].clone()
    ref, bar, d = field_bar(x0, y, mask, w0, 5, 3, 4.0, 0.0, 0.05)
    for b in range(B):
        el = abs(float(loss[b]) - float(ref["loss"][b])) / float(ref["loss"][b])
        eg = float((g[b, 0:3].cpu().double() - ref["g"][b, 0:3]).abs().max())
        assert el <= 2e-6 and eg <= 2e-7 + 1e-5 * float(ref["g"][b, 0:3].abs().max()), (b, el, eg)
    if C == 4:
        assert float(g[:, 3].abs().max()) == 0.0
    ew = float(np.abs(w.cpu().numpy().astype(np.float64) - ref["w"].astype(np.float64)).max())
    moved = float(np.abs(ref["w"] - w0).max())
    print(f"FIELDTERM masked={masked} C={C}: field vs float64 oracle {ew:.3e}; oracle float64 vs float32 {d:.3e} (bar {bar:.3e}); moved {moved:.2e}")
    assert moved > 1e-4 and ew <= bar
    assert np.array_equal(op.kernels().reshape(3, 3, 25), w.cpu().numpy().astype(np.float64))
    live = op.taps(DEV)[2]
    op.reset()
    assert np.array_equal(live.cpu().numpy(), w0)
    g2, loss2 = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    assert op.taps(DEV)[2] is live and torch.equal(g2, g) and torch.equal(loss2, loss) and torch.equal(live, w)
    # learn: False is field_blur with the init field
    fixed = field_cond(pkg, B, learn=False)
    plain = CM.PosteriorSampling(M.get_operator("field_blur", device=DEV, kernels=M.blind_field_init(5, (3, 3), "gaussian", 1.0), normalize=False),
                                 M.get_noise("gaussian", sigma=0.0), scale="0.3")
    for c in (fixed, plain):
        if masked:
            c.set_measurement_mask(mask, batch=B, device=DEV)
    gf, lf = fixed.loss_grad_x0(x0.to(DEV), y.to(DEV))
    gp, lp = plain.loss_grad_x0(x0.to(DEV), y.to(DEV))
    assert torch.equal(gf, gp) and torch.equal(lf, lp)


def test_a_fully_masked_member_changes_nothing_in_the_field(pkg):
    B, H, W = 3, 36, 34
    x0, y, mask = term_inputs(B, 3, H, W, True)
    mask[2] = 0.0
    three, two = field_cond(pkg, 3), field_cond(pkg, 2)
    three.set_measurement_mask(mask, batch=3, device=DEV)
    two.set_measurement_mask(mask[:2], batch=2, device=DEV)
    g3, l3 = three.loss_grad_x0(x0.to(DEV), y.to(DEV))
    g2, l2 = two.loss_grad_x0(x0[:2].to(DEV), y[:2].to(DEV))
    assert torch.equal(three.operator.taps(DEV)[2], two.operator.taps(DEV)[2])
    assert torch.equal(g3[:2], g2) and torch.equal(l3[:2], l2) and float(l3[2]) == 0.0 and float(g3[2].abs().max()) == 0.0
    with pytest.raises(ValueError, match="blind_field_blur: the learnt field is shared"):
        three.loss_grad_x0(x0[:2].to(DEV), y[:2].to(DEV), rows=(0, 2))


# ------------------------------------------------------------------------------------------------------------ 4: recovery
@pytest.mark.parametrize("seed", [0, 1])
def test_recovery_of_a_radial_defocus_field_when_the_image_is_known(pkg, seed):
    """The convex problem of tests/test_blindfield_cpu.py through the kernels: last loss <= 0.25 x the first, mean per-node L1 to the
    true field <= 0.5 x the init's, last loss <= 0.5 x that of ONE shared PSF fitted by blind_blur's kernels to the same data, and
    the final field against the float64 oracle's under `field_bar`."""
    _, _, M, CM = pkg
    x, y, kstar, w0 = O.recovery_problem(seed)
    xd, yd = x.float().to(DEV), y.float().to(DEV)
    first = float(field_cond(pkg, 1, n_iter=1, eta=4.0).loss_grad_x0(xd, yd)[1][0])
    cond = field_cond(pkg, 1, n_iter=200, eta=4.0)
    cond.loss_grad_x0(xd, yd)
    K = cond.operator.kernels()
    final = float(field_cond(pkg, 1, init=K, learn=False).loss_grad_x0(xd, yd)[1][0])    # the loss AT the final field
    shared = CM.PosteriorSampling(M.get_operator("blind_blur", device=DEV, kernel_size=5, n_iter=200, eta=4.0, init_sigma=1.0),
                                  M.get_noise("gaussian", sigma=0.0), scale="0.3")
    shared.loss_grad_x0(xd, yd)
    probe = CM.PosteriorSampling(M.get_operator("blind_blur", device=DEV, kernel_size=5, init=shared.operator.kernel2d(), learn=False),
                                 M.get_noise("gaussian", sigma=0.0), scale="0.3")
    one = float(probe.loss_grad_x0(xd, yd)[1][0])
    e0, e1 = O.node_l1(w0, kstar), O.node_l1(K, kstar)
    ref, bar, d = field_bar(x.float(), y.float(), None, w0, 5, 200, 4.0)
    ew = float(np.abs(K.reshape(3, 3, 25) - ref["w"].astype(np.float64)).max())
    print(f"FIELDRECOVERY gpu seed {seed}: loss {first:.4f} -> {final:.4f} ({final / first:.4f} x), mean L1 {e0.mean():.4f} -> {e1.mean():.4f} "
          f"({e1.mean() / e0.mean():.4f} x), worst {e0.max():.4f} -> {e1.max():.4f}; one shared PSF {one:.4f} ({final / one:.4f} x); field vs "
          f"float64 oracle {ew:.3e}; oracle float64 vs float32 {d:.3e} (bar {bar:.3e})")
    assert final <= 0.25 * first and e1.mean() <= 0.5 * e0.mean() and final <= 0.5 * one
    assert ew <= bar


# ------------------------------------------------------------------------------------------------------------ 5: the chains
CHAIN_OKW = dict(kernel_size=5, grid=[2, 2], n_iter=2, eta=0.5, init_sigma=1.0, smooth=0.02)
_ORACLE = {}


def oracle_chain():
    """The oracle's DDPM chain on the tiny 3 -> 6 network (once): the final image and field, its drift under a 1e-6 perturbation of
    x_T, and the field's distance to the same chain with the data term's image side in float32."""
    if not _ORACLE:
        from osmosis_diffusion_code_amd.guided_diffusion.measurements import blind_field_init
        cfg = U.UNetConfig.from_create_model_kwargs(**RGB_KW)
        sd = U.seeded_state_dict(cfg, 1234)
        tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
        x_T, y, noise, _ = chain_inputs(1, 3, 10)
        w0 = blind_field_init(5, (2, 2), "gaussian", 1.0).reshape(2, 2, 25).astype(np.float32)

        def net(x, t):
            return U.unet_forward(sd, cfg, x, t)

        def run(x_start):
            return O.ps_chain(net, tb, x_start, y, list(noise), w0, 5, 5, 2, 0.5, 0.0, 0.02, 0.3)
        img, w = run(x_T)
        pimg, pw = run(x_T + 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99)))
        orig = O.inner_loop
        try:
            O.inner_loop = lambda *a, **k: orig(*a, **dict(k, dtype=torch.float32))
            _, w32 = run(x_T)
        finally:
            O.inner_loop = orig
        _ORACLE.update(img=img, w=w, w0=w0, tb=tb, drift=float((pimg - img).abs().max()),
                       d_field=float(np.abs(w.astype(np.float64) - w32.astype(np.float64)).max()),
                       d_field_drift=float(np.abs(w.astype(np.float64) - pw.astype(np.float64)).max()))
    return _ORACLE


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_field_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """The fused loop against `_generic_loop` on the same injected draws at the fused-vs-generic bars of tests/test_rgb_gpu.py (1e-4
    for 4 -> 8), and the two routes' final fields under 5 x the oracle chain's float64 / float32 field distance."""
    _, gd, M, CM = pkg
    sname, skw, pat_kw, net, masked, ref_tag = CHAIN_CASES[tag]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    kbar = 5.0 * oracle_chain()["d_field"]
    pat = dict(PATTERN, **pat_kw)
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, sampler.num_timesteps))
    x_T, y, noise, mask = chain_inputs(1, C, n)
    x_T, y, noise = x_T.to(DEV), y.to(DEV), noise.to(DEV)
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=True,
              sample_pattern=pat, measurement_mask=mask if masked else None)
    cond = field_cond(pkg, **CHAIN_OKW)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, pat, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    kf = cond.operator.kernels()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = field_cond(pkg, third_party=C == 4, **CHAIN_OKW)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, pat, tuple(x_T.shape)) is None
    _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    kg = cond.operator.kernels()
    e, ek = float((f.cpu() - g.detach().cpu()).abs().max()), float(np.abs(kf - kg).max())
    moved = float(max(r["grad"].abs().max() for r in trace))
    kmoved = float(np.abs(kf.reshape(2, 2, 25) - cond.operator.host_taps()[2]).max())
    print(f"FIELDCHAIN {tag}: fused vs generic image {e:.3e} (bar {bar:.3e}), field {ek:.3e} (bar {kbar:.3e}); largest guidance "
          f"gradient {moved:.2e}, the field moved {kmoved:.2e}")
    assert moved > 0.0 and kmoved > 1e-4
    assert e <= bar and ek <= kbar
    assert np.abs(kf.sum(axis=(2, 3)) - 1.0).max() < 1e-6 and (kf >= 0).all()


def test_fused_field_chain_vs_the_oracle_chain(pkg, monkeypatch, model36):
    """One 10-index DDPM chain, free-running against the oracle's driver with the same weights, x_T, measurement and noise, under
    10 x the oracle's own drift for a 1e-6 perturbation of x_T -- the image's drift for the image, the field's for the field."""
    _, gd, M, CM = pkg
    o = oracle_chain()
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(o["tb"].timestep_map)
    x_T, y, noise, _ = chain_inputs(1, 3, 10)
    nd = noise.to(DEV)
    cond = field_cond(pkg, **CHAIN_OKW)
    _no_generic(monkeypatch, sampler)
    f = sampler.p_sample_loop(model=model36, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k])
    bar, kbar = _free_running_bar(o["drift"]), 10.0 * o["d_field_drift"]
    e = float((f.cpu() - o["img"]).abs().max())
    ek = float(np.abs(cond.operator.kernels().reshape(2, 2, 25) - o["w"].astype(np.float64)).max())
    print(f"FIELDCHAIN oracle: image {e:.3e} (oracle drift_1e-6 {o['drift']:.2e}, bar {bar:.2e}); field {ek:.3e} (oracle float64 vs "
          f"float32 {o['d_field']:.3e}, under the perturbation {o['d_field_drift']:.3e}, bar {kbar:.3e})")
    assert e <= bar and ek <= kbar


def test_batch_of_three_walked_as_two_and_one_equals_one_pass(pkg, monkeypatch, model36):
    """The field couples the batch: every chunk's forward, ONE data term over the three images, every chunk's backward.  Image and
    field agree with the one-pass chain bit for bit."""
    _, gd, M, CM = pkg
    x_T, y, noise, mask = chain_inputs(3, 3, 10, seed=32)
    x_T, y, noise = x_T.to(DEV), y.to(DEV), noise.to(DEV)
    calls = []

    def run():
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        cond = field_cond(pkg, 3, **CHAIN_OKW)
        orig = cond.loss_grad_x0

        def counted(x0, *a, **k):
            calls.append(x0.shape[0])
            return orig(x0, *a, **k)
        cond.loss_grad_x0 = counted
        img = sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                    save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                    noise_fn=lambda k, shape: noise[k], measurement_mask=mask, index_range=(9, 5))
        return img, cond.operator.kernels()
    whole, kw = run()
    assert bool(torch.isfinite(whole).all()) and calls == [3] * 5
    seen = []

    def two_one(B, cap):
        seen.append(B)
        return [2, 1]
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(two_one))
    del calls[:]
    chunked, kc = run()
    monkeypatch.undo()
    assert seen == [3] and calls == [3] * 5                              # still ONE data term per sub-step, over the whole batch
    assert torch.equal(chunked, whole) and np.array_equal(kc, kw)
    assert not np.array_equal(kw, M.blind_field_init(5, (2, 2), "gaussian", 1.0).astype(np.float32).astype(np.float64))


def test_a_fixed_field_chain_is_field_blurs_and_poisson_and_tiling_are_refused(pkg, monkeypatch, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    x_T, y, noise, _ = chain_inputs(1, 3, 10)
    nd = noise.to(DEV)
    kw = dict(model=model36, x_start=x_T.to(DEV), measurement=y.to(DEV), record=False, save_root=None, pretrain_model="imagenet",
              rgb_guidance=True, sample_pattern=PATTERN)
    fixed = field_cond(pkg, learn=False, **{k: v for k, v in CHAIN_OKW.items() if k != "learn"})
    plain = CM.PosteriorSampling(M.get_operator("field_blur", device=DEV, kernels=M.blind_field_init(5, (2, 2), "gaussian", 1.0), normalize=False),
                                 M.get_noise("gaussian", sigma=0.0), scale="0.3")
    _no_generic(monkeypatch, sampler)
    a = sampler.p_sample_loop(measurement_cond_fn=fixed.conditioning, noise_fn=lambda k, shape: nd[k], index_range=(9, 5), **kw)
    b = sampler.p_sample_loop(measurement_cond_fn=plain.conditioning, noise_fn=lambda k, shape: nd[k], index_range=(9, 5), **kw)
    monkeypatch.undo()
    assert torch.equal(a, b)
    poisson = CM.PosteriorSampling(M.get_operator("blind_field_blur", device=DEV, **CHAIN_OKW), M.get_noise("poisson", rate=1.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="blind_field_blur.*poisson"):
        sampler.p_sample_loop(measurement_cond_fn=poisson.conditioning, **kw)
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(measurement_cond_fn=field_cond(pkg, **CHAIN_OKW).conditioning, tiling=dict(tile=16, stride=8), **kw)


# ------------------------------------------------------------------------------------------------------------ 6: the driver
def test_restore_image_learns_a_field_resets_it_per_global_iteration_and_writes_the_mosaic(pkg, monkeypatch, model48, tmp_path):
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    resets = []
    orig = M.BlindFieldOperator.reset
    monkeypatch.setattr(M.BlindFieldOperator, "reset", lambda self: (resets.append(self.kernels()), orig(self))[1])
    g = torch.Generator().manual_seed(41)
    ref = (torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV)
    truth = dict(name="field_blur", model="radial_defocus", kernel_size=5, sigma_center=0.5, sigma_corner=1.5, grid=[2, 2])
    cfg = {"measurement": {"operator": dict(name="blind_field_blur", simulate_with=truth, **CHAIN_OKW),
                           "noise": {"name": "gaussian", "sigma": 0.0}},
           "conditioning": {"method": "ps", "params": dict(scale="0.3")},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="4"),
           "sample_pattern": dict(PATTERN, global_N=2), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": True}
    res = sampling.restore_image(model48, ref, cfg, noise_seed=7, index_range=(3, 1))
    assert len(res) == 2 and len(resets) == 2
    init = M.blind_field_init(5, (2, 2), "gaussian", 1.0).astype(np.float32).astype(np.float64)
    assert np.array_equal(resets[0], init) and not np.array_equal(resets[1], init)       # the second reset found a learnt field
    blurred = M.get_operator(device=DEV, **truth).forward(ref).cpu()
    for r in res:
        k = r["kernel"]
        assert k.dtype == torch.float32 and k.shape == (2, 2, 5, 5) and float(k.min()) >= 0.0
        assert float((k.double().sum(dim=(2, 3)) - 1.0).abs().max()) <= 1e-6
        assert torch.equal(r["measurement"], blurred) and bool(torch.isfinite(r["sample"]).all())
    assert torch.equal(res[0]["kernel"], res[1]["kernel"]) and torch.equal(res[0]["sample"], res[1]["sample"])   # same seed, same start
    assert not np.array_equal(res[0]["kernel"].double().numpy(), init)
    paths = sampling.save_outputs(res[-1], ref.cpu(), str(tmp_path), "photo", save_grids=False)
    assert paths["kernel"].endswith("photo_kernel.png") and os.path.exists(paths["kernel"])
    from PIL import Image
    pic = np.asarray(Image.open(paths["kernel"]))
    assert pic.ndim == 2 and pic.shape[0] == pic.shape[1] and pic.max() == 255
    with pytest.raises(ValueError, match="blind_field_blur: `simulate: True` needs"):
        bad = dict(cfg, measurement=dict(cfg["measurement"], operator=dict(name="blind_field_blur", **CHAIN_OKW)))
        sampling.restore_image(model48, ref, bad, noise_seed=7)
