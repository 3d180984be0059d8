"""Spatially varying blur on the GPU: osm_psf_field_apply (include/osmosis_psffield.h), forward and adjoint,
 - bit for bit against its fp32 restatement: one osm_psf_apply per node, the four corner outputs gathered per pixel and combined by
   torch fp32 elementwise operations in the header's order (forward); the sum over the nodes, ascending, of osm_psf_apply(adjoint) on
   hat_n (.) v formed in torch fp32 (adjoint);
 - against the float64 oracle of tests/psffield_oracle.py on the same fp32 inputs under the header's bound (ratio <= 1, printed);
then `osmosis::psf_field_apply`, the 'ps' data term through `field_blur`, the fused sampler loop against `_generic_loop`, and the driver.
The reference has no such operator.  Every output is NaN-filled first; C in {3, 4} strides; zero planes.

Bars: the header's bounds (derived there); the data term and the chains at exactly the bars tests/test_psf_gpu.py holds `psf_blur`
to (its constants are imported, not restated).

Measured on one MI355X (the PSFFIELD lines this file prints): worst |err| / bound 0.134 forward, 0.050 adjoint; identical nodes 0.385
of 8 u |c|; the data term's loss <= 1.3e-7 relative, gradient <= 4.5e-7; fused vs generic 2.7e-7 ... 7.2e-7."""
import os

import numpy as np
import pytest
import torch

import psffield_oracle as O
from test_psf_gpu import (CHAIN_CASES, GOLD, H0, MEASURED_RGB, PATTERN, W0, _no_generic, _replay_p_sample_draws, chain_inputs, make_sampler,  # noqa: F401
                          model36, model48, pkg)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U24 = 2.0 ** -24


def _dense(gh, gw, kh, kw, seed):
    return np.random.default_rng(seed).standard_normal((gh, gw, kh, kw))


def _asym(gh, gw, seed):
    k = _dense(gh, gw, 3, 7, seed)                                  # a different asymmetric 3 x 7 PSF per node, each with its own holes
    rng = np.random.default_rng(seed + 1)
    for jy in range(gh):
        for jx in range(gw):
            k[jy, jx].reshape(-1)[rng.choice(21, size=4, replace=False)] = 0.0
    return k


def _motion(gh, gw, k=9):
    from osmosis_diffusion_code_amd.guided_diffusion.measurements import motion_kernel
    return np.stack([np.stack([motion_kernel(k, 0.5, seed=jy * gw + jx) for jx in range(gw)]) for jy in range(gh)])


# case -> (H, W, the node kernels [gh,gw,kh,kw])
CASES = {"a.one_cell": (36, 34, lambda: _dense(2, 2, 5, 5, 1)),             # one cell; ragged tiles on both axes
         "b.cells_per_tile": (40, 72, lambda: _asym(3, 4, 2)),              # several cells per tile; kh != kw; a union with zeros
         "c.mirrors": (8, 12, lambda: _dense(2, 3, 9, 9, 3)),               # both mirrors reach; cells narrower than the reach
         "d.interior": (70, 66, lambda: _motion(5, 5)),                     # an interior tile; nine-node tiles
         "e.all_nodes": (36, 34, lambda: _dense(5, 5, 5, 5, 4))}            # cells of about 8 px: every node in one tile
CHAIN_FIELD = lambda: _motion(2, 3, 5)                                       # noqa: E731  (the chains: a 2 x 3 field of k = 5 kernels on 16 x 24)


def make_op(M, case, B=1):
    H, W, ks = CASES[case]
    return M.get_operator("field_blur", device=DEV, batch_size=B, kernels=ks(), normalize=False), H, W


def chain_op(M, B=1):
    return M.get_operator("field_blur", device=DEV, batch_size=B, kernels=CHAIN_FIELD())


def apply_field(op, x, C_out, adjoint, R=None):
    """osm_psf_field_apply on the colour planes of x [B,C_in,H,W] into a NaN-filled [B,C_out,H,W] (planes beyond 2: zero_planes)."""
    from osmosis_diffusion_code_amd import ops
    B, C_in, H, W = x.shape
    Ry, Rx = op.radius() if R is None else R
    out = torch.full((B, C_out, H, W), float("nan"), device=DEV)
    ops.psf_field_apply(x, out, *op.taps(DEV), op.field_tables(H, W, DEV), Ry, Rx, B, 3, C_in * H * W, C_out * H * W, H, W, adjoint=adjoint,
                        zero_planes=C_out - 3)
    return out


def node_apply(op, x, jy, jx, adjoint):
    """osm_psf_apply with the weights of node (jy, jx) over the shared tap list, on the colour planes of x [B,C,H,W] -> [B,3,H,W]."""
    from osmosis_diffusion_code_amd import ops
    B, C, H, W = x.shape
    dy, dx, w = op.taps(DEV)
    out = torch.full((B, 3, H, W), float("nan"), device=DEV)
    ops.psf_apply(x, out, dy, dx, w[jy, jx].contiguous(), *op.radius(), B, 3, C * H * W, 3 * H * W, H, W, adjoint=adjoint)
    return out


def restated_forward(op, x):
    """The header's forward in fp32: c_kl from osm_psf_apply per node, then a = 1 - fx, b = 1 - fy, top = a c00 + fx c01,
    bot = a c10 + fx c11, out = b top + fy bot -- one torch elementwise operation (one rounding) per product and per sum."""
    B, C, H, W = x.shape
    gh, gw = op.grid
    iy0, fy, ix0, fx = op.field_tables(H, W, DEV)
    conv = torch.stack([torch.stack([node_apply(op, x, jy, jx, False) for jx in range(gw)]) for jy in range(gh)])   # [gh,gw,B,3,H,W]
    cy, cx = iy0.long()[:, None].expand(H, W), ix0.long()[None, :].expand(H, W)
    ii, jj = torch.arange(H, device=DEV)[:, None].expand(H, W), torch.arange(W, device=DEV)[None, :].expand(H, W)

    def corner(k, l):
        return conv[cy + k, cx + l, :, :, ii, jj].permute(2, 3, 0, 1).contiguous()                                  # [H,W,B,3] -> [B,3,H,W]
    a, b = 1.0 - fx, (1.0 - fy)[:, None]
    top = a * corner(0, 0) + fx * corner(0, 1)
    bot = a * corner(1, 0) + fx * corner(1, 1)
    return b * top + fy[:, None] * bot


def hats32(op, H, W):
    """(haty fp32 [gh,H], hatx fp32 [gw,W]) on the device, as the header forms them: a = 1 - fx where ix0 = jx, fx where ix0 = jx - 1."""
    gh, gw = op.grid
    iy0, fy, ix0, fx = op.field_tables(H, W, DEV)

    def axis(i0, f, g):
        j = torch.arange(g, device=DEV)[:, None]
        zero = torch.zeros((), device=DEV)
        return torch.where(i0[None, :] == j, (1.0 - f)[None, :], torch.where(i0[None, :] == j - 1, f[None, :], zero))
    return axis(iy0, fy, gh), axis(ix0, fx, gw)


def restated_adjoint(op, v):
    """s = A_first; s = s + A_n for the other nodes in ascending row-major order, A_n = osm_psf_apply(adjoint) on fl(hat_n v)."""
    B, C, H, W = v.shape
    gh, gw = op.grid
    hy, hx = hats32(op, H, W)
    s = None
    for jy in range(gh):
        for jx in range(gw):
            hat = hy[jy][:, None] * hx[jx][None, :]
            An = node_apply(op, (hat * v[:, 0:3]).contiguous(), jy, jx, True)
            s = An if s is None else s + An
    return s


_REF = {}


def reference(M, case):
    """Inputs and the float64 results of a case, computed once: x [2,4,H,W], v [2,3,H,W] fp32; A x, A^T v and the two bounds."""
    if case not in _REF:
        op, H, W = make_op(M, case)
        g = torch.Generator().manual_seed(11)
        x, v = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
        dy, dx, w = op.host_taps()
        K = O.kernels_of_taps(dy, dx, w, *op.radius())
        x64, v64 = x[:, 0:3].double(), v.double()
        bf, ba = O.bounds(x64, v64, K, len(dy))
        _REF[case] = dict(op=op, H=H, W=W, x=x, v=v, Ax=O.forward_sum(x64, K), Atv=O.adjoint_vjp(v64, K), bf=bf, ba=ba)
    return _REF[case]


def check(got, want, bound, what):
    assert bool(torch.isfinite(got).all()), f"{what}: an output element was not written"
    err = (got[:, 0:3].double() - want).abs()
    ratio = float((err / bound.clamp_min(1e-300)).max())
    print(f"PSFFIELD {what}: worst |err| / bound {ratio:.3f} (max |err| {float(err.max()):.2e})")
    assert ratio <= 1.0, (what, ratio)
    if got.shape[1] > 3:
        assert float(got[:, 3:].abs().max()) == 0.0 and not bool(torch.signbit(got[:, 3:]).any())      # the zero planes: exactly +0


# ------------------------------------------------------------------------------------------------------------ 1: the kernel
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", list(CASES))
def test_forward_and_adjoint_bits_and_float64(pkg, case, C):
    _, _, M, _ = pkg
    ref = reference(M, case)
    op = ref["op"]
    x, v = ref["x"][:, 0:C].contiguous(), ref["v"]
    xd, vd = x.to(DEV), v.to(DEV)
    Ax_d = apply_field(op, xd, 3, False)                        # reads the colour planes of [B,C,HW]
    Atv_d = apply_field(op, vd, C, True)                        # writes [B,C,HW], the depth plane as +0
    # bit for bit the fp32 restatement
    assert torch.equal(Ax_d, restated_forward(op, xd)), f"{case}: forward bits"
    assert torch.equal(Atv_d[:, 0:3], restated_adjoint(op, vd)), f"{case}: adjoint bits"
    Ax, Atv = Ax_d.cpu(), Atv_d.cpu()
    check(Ax, ref["Ax"], ref["bf"], f"{case} C={C} forward")
    check(Atv, ref["Atv"], ref["ba"], f"{case} C={C} adjoint")
    # <A x, v> = <x, A^T v>, in float64 from the kernel's fp32 outputs, under the bound the two element bounds give
    x64, v64 = x[:, 0:3].double(), v.double()
    lhs, rhs = float((Ax.double() * v64).sum()), float((x64 * Atv[:, 0:3].double()).sum())
    allow = float((ref["bf"] * v64.abs()).sum() + (ref["ba"] * x64.abs()).sum())
    print(f"PSFFIELD {case} C={C} adjoint identity: |<Ax,v> - <x,Atv>| / bound {abs(lhs - rhs) / allow:.3f}")
    assert abs(lhs - rhs) <= allow
    # a repeat, and a B = 2 call is two B = 1 calls
    assert torch.equal(apply_field(op, xd, 3, False), Ax_d) and torch.equal(apply_field(op, vd, C, True), Atv_d)
    for b in range(2):
        assert torch.equal(apply_field(op, xd[b:b + 1].contiguous(), 3, False)[0], Ax_d[b]), b
        assert torch.equal(apply_field(op, vd[b:b + 1].contiguous(), C, True)[0], Atv_d[b]), b


def test_unstaged_and_staged_windows_give_the_same_bits(pkg):
    """Case (f): the taps of (b) (reach 1 x 3) at the stated radii 4 (staged), 32 (the last staged size: 96 x 97), 33 (the first
    unstaged: 98 x 99) and 39 = H - 1: the same values in the same order, the same bits -- each of them the natural radius's."""
    _, _, M, _ = pkg
    ref = reference(M, "b.cells_per_tile")
    op = ref["op"]
    assert op.radius() == (1, 3) and (32 + 64) * ((32 + 64) | 1) <= 96 * 97 < (32 + 66) * ((32 + 66) | 1)
    xd, vd = ref["x"].to(DEV), ref["v"].to(DEV)
    for adjoint, src in ((False, xd), (True, vd)):
        base = apply_field(op, src, 4, adjoint)
        for R in (4, 32, 33, 39):
            assert torch.equal(apply_field(op, src, 4, adjoint, R=(R, R)), base), (adjoint, R)
        assert torch.equal(apply_field(op, src, 4, adjoint, R=(39, 4)), base) and torch.equal(apply_field(op, src, 4, adjoint, R=(4, 39)), base)


def test_a_field_of_identical_nodes_is_osm_psf_apply_within_the_combines_roundings(pkg):
    """|out - c| <= 8 u |c| per element, c = osm_psf_apply's value: six roundings of the combine, one each in a and b."""
    _, _, M, _ = pkg
    k = np.random.default_rng(5).standard_normal((5, 7))
    H, W = 40, 72
    field = M.get_operator("field_blur", device=DEV, kernels=np.broadcast_to(k, (3, 4, 5, 7)).copy(), normalize=False)
    g = torch.Generator().manual_seed(13)
    x = torch.randn(2, 3, H, W, generator=g).to(DEV)
    c = node_apply(field, x, 0, 0, False)
    single = M.get_operator("psf_blur", device=DEV, kernel=k, normalize=False)
    assert torch.equal(c, single.forward(x))                     # (node (0, 0)'s launch IS psf_blur's)
    out = apply_field(field, x, 3, False)
    ratio = float(((out.double() - c.double()).abs() / (8 * U24 * c.double().abs()).clamp_min(1e-300)).max())
    print(f"PSFFIELD identical nodes: worst |out - c| / (8 u |c|) {ratio:.3f}")
    assert ratio <= 1.0


def test_bad_arguments_return_a_status_and_launch_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib, ops
    _, _, M, _ = pkg
    op, H, W = make_op(M, "b.cells_per_tile")
    dy, dx, w = op.taps(DEV)
    tabs = op.field_tables(H, W, DEV)
    x = torch.randn(1, 3, H, W, device=DEV)
    out = torch.full((1, 3, H, W), float("nan"), device=DEV)
    lib, p = _lib.load(), _lib.ptr
    good = [p(x), p(out), p(dy), p(dx), p(w), w.shape[2], 1, 3, 3, 4, *(p(t) for t in tabs), 1, 3, 3 * H * W, 3 * H * W, H, W, 0, 0, None]
    # a null pointer (x, a tap array, a table), T < 1, R >= the image side, a grid of 1 / 33 / more nodes than pixels, a short stride, a bad flag
    for pos, val in ((0, None), (2, None), (10, None), (13, None), (5, 0), (6, H), (7, W), (8, 1), (9, 33), (8, H + 1), (16, 3 * H * W - 1),
                     (17, 3 * H * W - 1), (14, 0), (20, 2), (21, -1)):
        args = list(good)
        args[pos] = val
        assert lib.osm_psf_field_apply(*args) == -1 and lib.osm_last_error().decode().startswith("osm_psf_field_apply"), pos
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    with pytest.raises(_lib.OsmosisHipError, match="smaller"):
        ops.psf_field_apply(x, out, dy, dx, w, tabs, 1, 3, 2, 3, 3 * H * W, 3 * H * W, H, W)
    with pytest.raises(_lib.OsmosisHipError, match="table"):
        ops.psf_field_apply(x, out, dy, dx, w, op.field_tables(H, W + 1, DEV), 1, 3, 1, 3, 3 * H * W, 3 * H * W, H, W)
    with pytest.raises(_lib.OsmosisHipError, match="gh,gw,T"):
        ops.psf_field_apply(x, out, dy, dx, w[0, 0].contiguous(), tabs, 1, 3, 1, 3, 3 * H * W, 3 * H * W, H, W)
    with pytest.raises(_lib.OsmosisHipError, match="Ry"):
        ops.psf_field_apply(x, out, dy, dx, w, tabs, H, 3, 1, 3, 3 * H * W, 3 * H * W, H, W)
    assert lib.osm_psf_field_apply(*good) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all())


def test_recorded_launches_replay_and_capture(pkg):
    """The Recorder records the call like any other; replayed, and captured into a graph (the stream is the last
    argument), it writes the same bits."""
    from osmosis_diffusion_code_amd import _lib
    _, _, M, _ = pkg
    ref = reference(M, "a.one_cell")
    op, xd = ref["op"], ref["x"].to(DEV)
    with _lib.Recorder() as rec:
        first = apply_field(op, xd, 4, False)
        out = first.clone()
    assert len(rec) == 1 and rec.calls[0][0].__name__ == "osm_psf_field_apply"
    first.fill_(float("nan"))
    rec.replay()
    assert torch.equal(first, out)
    first.fill_(float("nan"))
    graph = rec.to_graph()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(first, out)


# ------------------------------------------------------------------------------------------------------------ 2: the operator
def test_opcheck_and_autograd_of_psf_field_apply(pkg):
    _, _, M, _ = pkg
    for case in ("b.cells_per_tile", "c.mirrors"):
        op, H, W = make_op(M, case)
        t, tabs, (Ry, Rx) = op.taps(DEV), op.field_tables(H, W, DEV), op.radius()
        g = torch.Generator().manual_seed(12)
        x = torch.randn(2, 3, H, W, generator=g).to(DEV)
        fn = torch.ops.osmosis.psf_field_apply.default
        torch.library.opcheck(fn, (x, *t, *tabs, Ry, Rx, False))
        torch.library.opcheck(fn, (x.clone().requires_grad_(True), *t, *tabs, Ry, Rx, False))
        torch.library.opcheck(fn, (x.clone().requires_grad_(True), *t, *tabs, Ry, Rx, True))
        xr = x.clone().requires_grad_(True)
        y = op.forward(xr)
        assert y.shape == (2, 3, H, W) and torch.equal(y.detach(), apply_field(op, x, 3, False))
        cot = torch.randn(2, 3, H, W, generator=g).to(DEV)
        gx, = torch.autograd.grad(y, xr, cot)
        assert torch.equal(gx, op.transpose(cot)) and torch.equal(gx, apply_field(op, cot, 3, True))      # the adjoint launch, bit for bit
        cr = cot.clone().requires_grad_(True)
        gc, = torch.autograd.grad(op.transpose(cr), cr, x)                                               # ... whose backward is the forward
        assert torch.equal(gc, y.detach())
    with pytest.raises(ValueError, match="reflection"):
        M.get_operator("field_blur", device=DEV, model="radial_defocus").forward(torch.zeros(1, 3, 12, 24, device=DEV))
    with pytest.raises(ValueError, match="node grid"):
        M.get_operator("field_blur", device=DEV, model="radial_defocus", kernel_size=3).forward(torch.zeros(1, 3, 4, 24, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 3: the data term
@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("case", ["b.cells_per_tile", "c.mirrors"])
def test_ps_data_term_through_a_field_vs_float64_autograd(pkg, case, masked, C):
    """loss[b] = ||M (y - A x0[b, 0:3])|| and its x0-gradient against float64 autograd through the oracle on the CPU, at the bars
    tests/test_psf_gpu.py holds `psf_blur` to: loss 2e-6 relative, gradient 2e-7 + 1e-5 max |want|; the depth channel's gradient
    exactly 0; a fully masked image has loss 0 and gradient 0."""
    _, _, M, CM = pkg
    B = 3
    op, H, W = make_op(M, case, B)
    g = torch.Generator().manual_seed(21)
    x0 = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    cond = CM.get_conditioning_method("ps", op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
    mask = torch.ones(B, 3, H, W)
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g)
        mask[1] = (torch.rand(1, 1, H, W, generator=g) > 0.4).float()
        mask[2] = 0.0                                                           # image 2: masked out entirely
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    gk, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV))
    gk, loss = gk.cpu().double(), loss.cpu().double()
    assert gk.shape == (B, C, H, W) and bool(torch.isfinite(gk).all()) and bool(torch.isfinite(loss).all())
    dy, dx, w = op.host_taps()
    K = O.kernels_of_taps(dy, dx, w, *op.radius())
    x64 = x0.double().requires_grad_(True)
    r = mask.double() * (y.double() - O.forward_sum(x64[:, 0:3], K))
    L = (r ** 2).sum(dim=(1, 2, 3)).sqrt()
    live = range(2) if masked else range(B)
    want, = torch.autograd.grad(sum(L[b] for b in live), x64)
    L = L.detach()
    for b in live:
        el, eg = abs(float(loss[b]) - float(L[b])) / float(L[b]), float((gk[b, 0:3] - want[b, 0:3]).abs().max())
        print(f"PSFFIELDTERM {case} masked={masked} C={C} image {b}: loss rel {el:.2e}, grad abs {eg:.2e} (max |want| {float(want[b, 0:3].abs().max()):.2e})")
        assert el <= 2e-6, (b, float(loss[b]), float(L[b]))
        assert eg <= 2e-7 + 1e-5 * float(want[b, 0:3].abs().max()), (b, eg)
    if C == 4:
        assert float(gk[:, 3].abs().max()) == 0.0
    if masked:
        assert float(loss[2]) == 0.0 and float(gk[2].abs().max()) == 0.0


# ------------------------------------------------------------------------------------------------------------ 4: the chains
def ps_cond(pkg, B=1, noiser=None, third_party=False):
    _, _, M, CM = pkg
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    return cls(chain_op(M, B), noiser or M.get_noise("gaussian", sigma=0.0), scale="0.3")


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_field_blur_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """The fused loop against `_generic_loop` (autograd through `operator.forward` = osmosis::psf_field_apply and the HIP UNet) on the
    same injected draws: tiny 3 -> 6 and 4 -> 8 networks, 16 x 24, 10 indices, a 2 x 3 field of k = 5 kernels; DDPM, DDIM +
    clip_denoised, local_M = 2, mean-only, masked under the identity chains' bars of tests/test_rgb_gpu.py (the ones
    tests/test_psf_gpu.py reuses), 4 -> 8 under 1e-4."""
    _, gd, M, CM = pkg
    sname, skw, branch, pat_kw, net, masked, ref_tag = CHAIN_CASES[tag]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    pat = dict(PATTERN, **pat_kw)
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, sampler.num_timesteps))
    x_T, y, noise, mask = chain_inputs(1, C, n)
    rg = branch == "rg"
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=rg,
              sample_pattern=pat, measurement_mask=mask if masked else None)
    cond = ps_cond(pkg)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = ps_cond(pkg, third_party=C == 4)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, rg, pat, tuple(x_T.shape)) is None
    if rg:
        _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    e = float((f.cpu() - g.detach().cpu()).abs().max())
    moved = float(max(r["grad"].abs().max() for r in trace))
    print(f"PSFFIELDCHAIN {tag}: fused vs generic {e:.3e} (bar {bar:.3e}); largest guidance gradient {moved:.2e}")
    assert moved > 0.0
    assert e <= bar


def test_field_blur_stays_fused_poisson_goes_generic_and_tiling_is_refused(pkg, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    x_T, y, noise, _ = chain_inputs(1, 3, 10)
    cond = ps_cond(pkg)
    assert sampler._fast_path_ok(model36, cond.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is cond
    poisson = ps_cond(pkg, noiser=M.get_noise("poisson", rate=1.0))
    assert sampler._fast_path_ok(model36, poisson.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is None
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              tiling=dict(tile=16, stride=8))


def test_batch_of_three_walked_in_chunks_equals_one_pass(pkg, monkeypatch, model36):
    """B = 3 with a mask: the one-pass chain and a [2, 1] walk agree bit for bit (the field is shared: a chunk needs no rows of it)."""
    _, gd, M, CM = pkg
    x_T, y, noise, mask = chain_inputs(3, 3, 10, seed=32)

    def run():
        sampler = make_sampler(gd)
        _no_generic(monkeypatch, sampler)
        cond = ps_cond(pkg, 3)
        return sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                     save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                     noise_fn=lambda k, shape: noise[k], measurement_mask=mask, index_range=(9, 5))
    whole = run()
    assert bool(torch.isfinite(whole).all())
    seen = []

    def two_one(B, cap):
        seen.append(B)
        return [2, 1]
    monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(two_one))
    chunked = run()
    monkeypatch.undo()
    assert seen == [3] and torch.equal(chunked, whole)


# ------------------------------------------------------------------------------------------------------------ 5: the driver
def test_restore_image_carries_the_field_and_writes_its_mosaic(pkg, monkeypatch, model36, tmp_path):
    """`restore_image` with `field_blur` on a 3-index sub-chain: y = noiser(A ref) as for `psf_blur`, the result carries `kernel`
    [gh,gw,k,k], `save_outputs` writes `<name>_kernel.png` as the gh x gw mosaic."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(41)
    ref = (torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV)
    okw = dict(name="field_blur", model="roll_shake", kernel_size=5, angle_deg=20.0, grid=[2, 3], image_size=[H0, W0])
    cfg = {"measurement": {"operator": okw, "noise": {"name": "gaussian", "sigma": 0.0}},
           "conditioning": {"method": "ps", "params": dict(scale="0.3")},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="4"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "imagenet"},
           "manual_seed": 0, "rgb_guidance": True}
    res = sampling.restore_image(model36, ref, cfg, noise_seed=7, index_range=(3, 1))[-1]
    op = M.get_operator(device=DEV, **okw)
    blurred = op.forward(ref).cpu()
    assert res["sample"].shape == (1, 3, H0, W0) and bool(torch.isfinite(res["sample"]).all())
    assert torch.equal(res["measurement"], blurred) and not torch.equal(blurred, ref.cpu())
    k = res["kernel"]
    assert k.dtype == torch.float32 and k.shape == (2, 3, 5, 5) and torch.equal(k, torch.from_numpy(op.kernels()).float())
    paths = sampling.save_outputs(res, ref.cpu(), str(tmp_path), "photo", save_grids=False)
    assert paths["kernel"].endswith("photo_kernel.png") and os.path.exists(paths["kernel"])
    from PIL import Image
    pic = np.asarray(Image.open(paths["kernel"]))
    z = 128 // 15
    assert pic.shape == (2 * 5 * z, 3 * 5 * z) and pic.max() == 255
    with pytest.raises(ValueError, match="simulate"):       # the measurement itself must have the network's grid, as for `psf_blur`
        sampling.restore_image(model36, ref, dict(cfg, measurement=dict(cfg["measurement"], operator=dict(okw, simulate=False))), noise_seed=7)
