"""PSF weight sets on the GPU (include/osmosis_psfset.h: one point-spread function per image and / or per colour plane):
osm_psf_apply_s and osm_psf_tap_step_s against the float64 oracle of tests/psfset_oracle.py and bit for bit against their single-set
siblings, the data term `loss_grad_x0` with per-image / per-channel learnt PSFs, the recovery problem where ONE kernel cannot fit,
the fused sampler loop (ungrouped walk) against `_generic_loop` and the oracle's chain, and `restore_images`.

Bars.  Kernel: tests/test_psf_gpu.py's derived bound per element, (N + 2) 2^-24 sum |w| |x| with N = T (forward) or 9 T (adjoint).
Step: 1 fp32 ulp (the final division's rounding), as tests/test_blind_gpu.py.  Data term: the identity term's bars (loss 2e-6
relative, gradient 2e-7 + 1e-5 max |want|).  Learnt sets: `kernel_bar`'s rule, 5 x the distance between the float64 oracle and the
same oracle with its image side in float32.  Chains: the fused-vs-generic bars of tests/test_rgb_gpu.py; against the oracle's driver
10 x the oracle's own drift under a 1e-6 perturbation of x_T (image and kernels each by their own drift)."""
import os

import numpy as np
import pytest
import torch

import blind_oracle as BO
import psfset_oracle as PO
from oracle import diffusion_ref as D
from oracle import unet_ref as U

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
U24 = 2.0 ** -24
TINY_KW = dict(image_size=256, num_channels=32, num_res_blocks=1, channel_mult="1,2,2", attention_resolutions="128,64",
               num_head_channels=16, num_heads=4, learn_sigma=True, use_scale_shift_norm=True, resblock_updown=True,
               pretrain_model="osmosis")
RGB_KW = dict(TINY_KW, pretrain_model="imagenet")
H0, W0 = 16, 24
PATTERN = dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=1, s_start=1, s_end=0, n_iter=20,
               start_guidance=1, stop_guidance=0)
# tests/test_rgb_gpu.py MEASURED of the identity 'ps' chains, as tests/test_blind_gpu.py copies them
MEASURED_RGB = {"rg.ddpm.c36": 5.960e-07, "rg.ddim.c36": 7.153e-07}
MODES = {"per_image": (True, False), "per_channel": (False, True), "both": (True, True)}
FLAGS = [(False, False), (True, False), (False, True), (True, True)]


@pytest.fixture(scope="module")
def pkg():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from osmosis_diffusion_code_amd.guided_diffusion import condition_methods, gaussian_diffusion, measurements, unet
    return unet, gaussian_diffusion, measurements, condition_methods


def dev(a):
    return (torch.from_numpy(a) if isinstance(a, np.ndarray) else a).to(DEV)


# ------------------------------------------------------------------------------------------------------------ 1: osm_psf_apply_s
# case -> (H, W, k, union): dense k x k supports; `union`: every set lacks taps another has (weight 0.0 there), and nobody has row 0
APPLY_CASES = {"tiles9": (36, 34, 9, False),             # two ragged tiles per axis
               "both_mirrors": (8, 6, 5, False),         # smaller than a tile, both mirrors reach
               "wide9": (40, 72, 9, False),
               "union9": (36, 34, 9, True)}
_APPLY = {}


def apply_reference(case):
    """Inputs, the fp32 kernels K [2,3,k,k] and the tap list of a case, once; `products(nb, nc)` adds the float64 results."""
    if case not in _APPLY:
        H, W, k, union = APPLY_CASES[case]
        g = torch.Generator().manual_seed(11)
        x, v = torch.randn(2, 4, H, W, generator=g), torch.randn(2, 3, H, W, generator=g)
        K = np.random.default_rng(7).standard_normal((2, 3, k, k)).astype(np.float32)
        if union:
            K[:, :, 0, :] = 0.0
            for b in range(2):
                for p in range(3):
                    K[b, p, 1 + b + p, :] = 0.0             # a row this set lacks and the others have
            K[1, 2] = 0.0
            K[1, 2, 6, 1] = 1.5                             # a lone off-centre tap
        iy, ix = np.nonzero((K != 0).any(axis=(0, 1)))
        _APPLY[case] = dict(H=H, W=W, k=k, x=x, v=v, K=K, dy=(iy - k // 2).astype(np.int32), dx=(ix - k // 2).astype(np.int32),
                            w=np.ascontiguousarray(K[:, :, iy, ix]), prod={})
    return _APPLY[case]


def products(ref, nb, nc):
    if (nb, nc) not in ref["prod"]:
        with PO.one_thread():
            K = torch.from_numpy(ref["K"][:nb, :nc].astype(np.float64))
            x64, v64 = ref["x"][:, 0:3].double(), ref["v"].double()

            def vjp(v, kern):
                z = torch.zeros_like(v).requires_grad_(True)
                return torch.autograd.grad(PO.conv_sets(z, kern), z, v)[0]
            ref["prod"][(nb, nc)] = dict(Ax=PO.conv_sets(x64, K), Atv=vjp(v64, K), mag_f=PO.conv_sets(x64.abs(), K.abs()),
                                         mag_a=vjp(v64.abs(), K.abs()))
    return ref["prod"][(nb, nc)]


def apply_s(ref, src, w, C_out, adjoint, R=None):
    """osm_psf_apply_s on the colour planes of src [B,C_in,H,W] into a NaN-filled [B,C_out,H,W]."""
    from osmosis_diffusion_code_amd import ops
    B, C_in, H, W = src.shape
    Ry, Rx = (ref["k"] // 2, ref["k"] // 2) if R is None else R
    out = torch.full((B, C_out, H, W), float("nan"), device=DEV)
    ops.psf_apply_s(src, out, dev(ref["dy"]), dev(ref["dx"]), w, Ry, Rx, B, 3, C_in * H * W, C_out * H * W, H, W, adjoint=adjoint,
                    zero_planes=C_out - 3)
    return out


def apply_one_plane(ref, plane, wset, adjoint):
    """osm_psf_apply on one plane [H,W] alone with one set [T]."""
    from osmosis_diffusion_code_amd import ops
    H, W = plane.shape
    out = torch.full((1, 1, H, W), float("nan"), device=DEV)
    ops.psf_apply(plane.reshape(1, 1, H, W).contiguous(), out, dev(ref["dy"]), dev(ref["dx"]), wset.contiguous(), ref["k"] // 2, ref["k"] // 2,
                  1, 1, H * W, H * W, H, W, adjoint=adjoint)
    return out[0, 0]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("case", list(APPLY_CASES))
def test_apply_s_vs_float64_and_bit_for_bit_vs_osm_psf_apply(pkg, case, C):
    from osmosis_diffusion_code_amd import ops
    ref = apply_reference(case)
    H, W, T = ref["H"], ref["W"], len(ref["dy"])
    xd, vd = dev(ref["x"][:, 0:C].contiguous()), dev(ref["v"])
    wall = dev(ref["w"])
    if case == "union9":
        assert T < 81 and bool((ref["w"] == 0).any(axis=2).all())            # every set lacks a tap of the union
    for nb, nc in ((1, 1), (2, 1), (1, 3), (2, 3)):
        w = wall[:nb, :nc].contiguous()
        pr = products(ref, nb, nc)
        for adjoint, src, want, mag, N, Cout in ((False, xd, pr["Ax"], pr["mag_f"], T, 3), (True, vd, pr["Atv"], pr["mag_a"], 9 * T, C)):
            got = apply_s(ref, src, w, Cout, adjoint)
            assert bool(torch.isfinite(got).all()), "an output element was not written"
            err = (got[:, 0:3].cpu().double() - want).abs()
            ratio = float((err / ((N + 2) * U24 * mag).clamp_min(1e-300)).max())
            print(f"PSFSET apply {case} C={C} sets=({nb},{nc}) adjoint={adjoint}: worst |err| / bound {ratio:.3f} (max |err| {float(err.max()):.2e})")
            assert ratio <= 1.0, (case, nb, nc, adjoint, ratio)
            if Cout > 3:
                assert float(got[:, 3:].abs().max()) == 0.0 and not bool(torch.signbit(got[:, 3:]).any())
            # every plane is osm_psf_apply on that plane alone with that set, bit for bit
            for b in range(2):
                for p in range(3):
                    one = apply_one_plane(ref, src[b, p], w[b if nb > 1 else 0, p if nc > 1 else 0], adjoint)
                    assert torch.equal(got[b, p], one), (case, nb, nc, adjoint, b, p)
            # a stated radius beyond the LDS window (the unstaged path) gives the staged result's bits
            if H > 33 and W > 33:
                assert torch.equal(apply_s(ref, src, w, Cout, adjoint, R=(33, 33)), got), (case, nb, nc, adjoint)
            if (nb, nc) == (1, 1):                  # strides (0, 0): osm_psf_apply itself
                plain = torch.full_like(got, float("nan"))
                ops.psf_apply(src, plain, dev(ref["dy"]), dev(ref["dx"]), w[0, 0].contiguous(), ref["k"] // 2, ref["k"] // 2, 2, 3,
                              src.shape[1] * H * W, Cout * H * W, H, W, adjoint=adjoint, zero_planes=Cout - 3)
                assert torch.equal(got, plain), (case, adjoint)


def test_apply_s_refuses_bad_strides_and_launches_nothing(pkg):
    from osmosis_diffusion_code_amd import _lib
    ref = apply_reference("both_mirrors")
    H, W, T = ref["H"], ref["W"], len(ref["dy"])
    x, w = dev(ref["x"][:, 0:3].contiguous()), dev(ref["w"])
    dy, dx = dev(ref["dy"]), dev(ref["dx"])
    out = torch.full((2, 3, H, W), float("nan"), device=DEV)
    lib, p = _lib.load(), _lib.ptr
    good = [p(x), p(out), p(dy), p(dx), p(w), T, 2, 2, 2, 3, 3 * H * W, 3 * H * W, H, W, 0, 0, 3 * T, T, None]
    for pos, val in ((16, -1), (17, T - 1), (16, 3 * T - 1), (16, T), (4, None), (5, 0), (6, H)):
        args = list(good)
        args[pos] = val
        assert lib.osm_psf_apply_s(*args) != 0 and lib.osm_last_error().decode().startswith("osm_psf_apply_s:")
    torch.cuda.synchronize()
    assert bool(torch.isnan(out).all())
    assert lib.osm_psf_apply_s(*good) == 0
    torch.cuda.synchronize()
    assert torch.equal(out, apply_s(ref, x, w, 3, False))


def test_opcheck_and_autograd_of_psf_apply_s(pkg):
    _, _, M, _ = pkg
    ref = apply_reference("union9")
    op = M.get_operator("psf_blur", device=DEV, kernel=ref["K"].astype(np.float64), normalize=False, per_image=True, per_channel=True,
                        batch_size=2)
    t, (Ry, Rx) = op.taps(DEV), op.radius()
    assert np.array_equal(op.host_taps()[2], ref["w"]) and tuple(t[2].shape) == (2, 3, len(ref["dy"]))
    x = dev(ref["x"][:, 0:3].contiguous())
    for sets in (t[2], t[2][:1].contiguous(), t[2][:, :1].contiguous()):
        torch.library.opcheck(torch.ops.osmosis.psf_apply_s.default, (x, t[0], t[1], sets, Ry, Rx, False))
        torch.library.opcheck(torch.ops.osmosis.psf_apply_s.default, (x.clone().requires_grad_(True), t[0], t[1], sets, Ry, Rx, False))
        torch.library.opcheck(torch.ops.osmosis.psf_apply_s.default, (x.clone().requires_grad_(True), t[0], t[1], sets, Ry, Rx, True))
    xr = x.clone().requires_grad_(True)
    y = op.forward(xr)
    assert torch.equal(y.detach(), apply_s(ref, x, t[2], 3, False))
    cot = dev(ref["v"])
    gx, = torch.autograd.grad(y, xr, cot)
    assert torch.equal(gx, op.transpose(cot)) and torch.equal(gx, apply_s(ref, cot, t[2], 3, True))     # the adjoint launch, bit for bit
    cr = cot.clone().requires_grad_(True)
    gc, = torch.autograd.grad(op.transpose(cr), cr, x)
    assert torch.equal(gc, y.detach())
    with pytest.raises(ValueError, match="batch of 3"):
        op.forward(torch.zeros(3, 3, 36, 34, device=DEV))


# ------------------------------------------------------------------------------------------------------------ 2: osm_psf_tap_step_s
def _step_case(T, B, nparts, nb, nc, seed):
    rng = np.random.default_rng(seed)
    w = rng.random((nb, nc, T)).astype(np.float32)
    w /= w.sum(axis=2, keepdims=True)
    part = rng.standard_normal((B, nparts, T)).astype(np.float32)
    loss = (rng.random(B) + 0.5).astype(np.float32)
    return w, part, loss


def run_step_s(w, part, loss, ntiles, hw3, eta, l1, per_image, per_channel):
    from osmosis_diffusion_code_amd import ops
    wd = dev(w.copy())
    ops.psf_tap_step_s(wd, dev(part), dev(loss), part.shape[0], 3, ntiles, hw3, eta, l1, per_image=per_image, per_channel=per_channel)
    return wd.cpu().numpy()


def run_step(w, part, loss, hw3, eta, l1):
    from osmosis_diffusion_code_amd import ops
    wd = dev(w.copy())
    ops.psf_tap_step(wd, dev(np.ascontiguousarray(part)), dev(np.ascontiguousarray(loss)), part.shape[0], part.shape[1], hw3, eta, l1)
    return wd.cpu().numpy()


@pytest.mark.parametrize("per_image,per_channel", FLAGS)
@pytest.mark.parametrize("T,B,nparts", [(25, 2, 3), (3721, 2, 12), (4225, 2, 3)])
def test_step_s_vs_the_numpy_step_and_bit_for_bit_vs_osm_psf_tap_step(pkg, T, B, nparts, per_image, per_channel):
    nb, nc, ntiles = (B if per_image else 1), (3 if per_channel else 1), nparts // 3
    w, part, loss = _step_case(T, B, nparts, nb, nc, T)
    hw3, eta = 3 * 36 * 34, 40.0                                       # large enough for the step to reach the clamp
    l1 = 1.0 / (T * eta)                                               # eta l1 = the mean weight: about half the taps clamp
    want, u, S = PO.step_sets(w, part, loss, 3, ntiles, hw3, eta, l1, per_image, per_channel)
    got = run_step_s(w, part, loss, ntiles, hw3, eta, l1, per_image, per_channel)
    assert (S > 0).all() and all((u[i, j] == 0).any() and (u[i, j] > 0).any() for i in range(nb) for j in range(nc))
    ulps = np.abs(got.astype(np.float64) - want.astype(np.float64)) / np.spacing(np.maximum(want, np.float32(1e-30))).astype(np.float64)
    print(f"PSFSET step T={T} B={B} nparts={nparts} flags=({int(per_image)},{int(per_channel)}): worst {ulps.max():.2f} ulp, "
          f"{int((u == 0).sum())} of {u.size} taps clamped")
    assert ulps.max() <= 1.0 and np.all(got[u == 0] == 0.0) and (got >= 0).all()
    assert np.abs(got.astype(np.float64).sum(axis=2) - 1.0).max() <= 1e-6             # every set on its own simplex
    # the bit-equalities of the contract
    if not per_image and not per_channel:
        assert np.array_equal(got[0, 0], run_step(w[0, 0], part, loss, hw3, eta, l1))
    if per_image and not per_channel:
        for b in range(B):
            assert np.array_equal(got[b, 0], run_step(w[b, 0], part[b:b + 1], loss[b:b + 1], hw3, eta, l1)), b
    if per_channel:                                                      # at B = 1: set c is the step on its plane's slice of the partials
        for b in (range(B) if per_image else [0]):
            one = got[b] if per_image else run_step_s(w, part[:1], loss[:1], ntiles, hw3, eta, l1, False, True)[0]
            for c in range(3):
                sl = part[b:b + 1, c * ntiles:(c + 1) * ntiles]
                assert np.array_equal(one[c], run_step(w[b if per_image else 0, c], sl, loss[b:b + 1], hw3, eta, l1)), (b, c)
    # a guard tripped in one set leaves that set's bits alone while the others step
    if per_image:
        bad = loss.copy()
        bad[1] = np.nan
        g2 = run_step_s(w, part, bad, ntiles, hw3, eta, l1, per_image, per_channel)
        assert np.array_equal(g2[1], w[1]) and np.array_equal(g2[0], got[0])
    if per_channel:
        pbad = part.copy()
        pbad[0, 2 * ntiles, 7] = np.inf                                  # plane 2 of image 0
        g3 = run_step_s(w, pbad, loss, ntiles, hw3, eta, l1, per_image, per_channel)
        assert np.array_equal(g3[0, 2], w[0, 2]) and np.array_equal(g3[0, :2], got[0, :2])
        if per_image:
            assert np.array_equal(g3[1], got[1])
    huge = run_step_s(w, part, loss, ntiles, hw3, 0.1, 1e9, per_image, per_channel)      # every u clamped to 0, in every set
    assert np.array_equal(huge, w)


# ------------------------------------------------------------------------------------------------------------ 3: the data term
def blind_cond(pkg, B=1, per_image=False, per_channel=False, **okw):
    _, _, M, CM = pkg
    kw = dict(kernel_size=9, n_iter=3, eta=0.5, init_sigma=1.5)
    kw.update(okw)
    return CM.PosteriorSampling(M.get_operator("blind_blur", device=DEV, batch_size=B, per_image=per_image, per_channel=per_channel, **kw),
                                M.get_noise("gaussian", sigma=0.0), scale="0.3")


def term_inputs(B, C, H, W, masked, seed=21):
    g = torch.Generator().manual_seed(seed)
    x0 = torch.rand(B, C, H, W, generator=g) * 1.8 - 0.9
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    mask = None
    if masked:
        mask = torch.rand(B, 3, H, W, generator=g)
        mask[1] = (torch.rand(1, 1, H, W, generator=g) > 0.4).float()
    return x0, y, mask


def kernel_bar(x0, y, mask, w0, k, n_iter, eta, l1=0.0):
    """(float64 oracle result, 5 x its distance to the float32 evaluation of the same oracle, that distance): tests/test_blind_gpu.py's rule."""
    r64 = PO.inner_loop_sets(x0, y, mask, w0, k, k, n_iter, eta, l1)
    r32 = PO.inner_loop_sets(x0, y, mask, w0, k, k, n_iter, eta, l1, dtype=torch.float32)
    d = float(np.abs(r64["w"].astype(np.float64) - r32["w"].astype(np.float64)).max())
    return r64, 5.0 * d, d


def sets3(w):
    """The live / host weights as [nb,nc,T] whatever the operator's sets are."""
    return w.reshape((1, 1) + tuple(w.shape)) if w.ndim == 1 else w


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("mode", list(MODES))
def test_data_term_with_three_inner_iterations_vs_the_oracle(pkg, monkeypatch, mode, masked, C):
    """B = 2 at 36 x 34, k = 9, n_iter = 3: loss and x0-gradient at the identity term's bars, every set after three steps under
    `kernel_bar`; the C call, the single launches and a repeat from reset() bit for bit; with one PSF per image the B = 2 call is two
    B = 1 calls."""
    per_image, per_channel = MODES[mode]
    B, H, W = 2, 36, 34
    x0, y, mask = term_inputs(B, C, H, W, masked)
    cond = blind_cond(pkg, B, per_image, per_channel)
    op = cond.operator
    if masked:
        cond.set_measurement_mask(mask, batch=B, device=DEV)
    w0 = op.host_taps()[2]
    assert w0.shape == (2 if per_image else 1, 3 if per_channel else 1, 81)
    g, loss = cond.loss_grad_x0(dev(x0), dev(y))
    g, loss, w = g.clone(), loss.clone(), op.taps(DEV)[2].clone()
    ref, bar, d = kernel_bar(x0, y, mask, w0, 9, 3, 0.5)
    for b in range(B):
        el = abs(float(loss[b]) - float(ref["loss"][b])) / float(ref["loss"][b])
        eg = float((g[b, 0:3].cpu().double() - ref["g"][b, 0:3]).abs().max())
        assert el <= 2e-6 and eg <= 2e-7 + 1e-5 * float(ref["g"][b, 0:3].abs().max()), (b, el, eg)
    if C == 4:
        assert float(g[:, 3].abs().max()) == 0.0
    ew = np.abs(w.cpu().numpy().astype(np.float64) - ref["w"].astype(np.float64)).max(axis=2)
    moved = np.abs(ref["w"] - w0).max(axis=2)
    print(f"PSFSET term {mode} masked={masked} C={C}: worst set vs float64 oracle {ew.max():.3e}; oracle float64 vs float32 {d:.3e} "
          f"(bar {bar:.3e}); the sets moved {moved.min():.2e} .. {moved.max():.2e}")
    assert (moved > 1e-4).all() and (ew <= bar).all()                    # every set, each under the bar
    assert np.array_equal(op.kernels().reshape(w0.shape), w.cpu().numpy().astype(np.float64))
    assert len({w[i, j].cpu().numpy().tobytes() for i in range(w.shape[0]) for j in range(w.shape[1])}) == w.shape[0] * w.shape[1]
    # a repeat from reset(): the same bits, in the same tensors
    live = op.taps(DEV)[2]
    op.reset()
    assert np.array_equal(live.cpu().numpy(), w0)
    g2, loss2 = cond.loss_grad_x0(dev(x0), dev(y))
    assert op.taps(DEV)[2] is live and torch.equal(g2, g) and torch.equal(loss2, loss) and torch.equal(live, w)
    # the single launches
    op.reset()
    monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1")
    g3, loss3 = cond.loss_grad_x0(dev(x0), dev(y))
    monkeypatch.undo()
    assert torch.equal(g3, g) and torch.equal(loss3, loss) and torch.equal(live, w)
    # a chunked walk: rows (0, 1) then (1, 2) of the open batch step their own rows -- the same bits again
    if per_image:
        op.reset()
        cond.open_batch(B, (H, W), (H, W), torch.device(DEV))
        gc, lc = torch.empty_like(g), torch.empty_like(loss)
        for b in range(B):
            cond.loss_grad_x0(dev(x0[b:b + 1]), dev(y[b:b + 1]), g_out=gc[b:b + 1], loss_out=lc[b:b + 1], rows=(b, b + 1))
        assert torch.equal(gc, g) and torch.equal(lc, loss) and torch.equal(live, w)
        # ... and two B = 1 runs of an operator of its own (one set per image: today's shared entry point, osm_ps_blind_optimize)
        for b in range(B):
            one = blind_cond(pkg, 1, False, per_channel)
            if masked:
                one.set_measurement_mask(mask[b:b + 1], batch=1, device=DEV)
            g1, l1 = one.loss_grad_x0(dev(x0[b:b + 1]), dev(y[b:b + 1]))
            assert one.operator.weight_sets == (1, 3 if per_channel else 1)
            assert torch.equal(g1[0], g[b]) and torch.equal(l1[0], loss[b]) and torch.equal(sets3(one.operator.taps(DEV)[2])[0], w[b]), b


def test_a_fully_masked_image_leaves_its_own_set_untouched_and_the_others_bits_alone(pkg):
    B, H, W = 2, 36, 34
    x0, y, mask = term_inputs(B, 3, H, W, True)
    full = blind_cond(pkg, B, True, False)
    full.set_measurement_mask(mask, batch=B, device=DEV)
    gf, lf = full.loss_grad_x0(dev(x0), dev(y))
    gf, wf = gf.clone(), full.operator.taps(DEV)[2].clone()
    dead = mask.clone()
    dead[1] = 0.0
    cond = blind_cond(pkg, B, True, False)
    cond.set_measurement_mask(dead, batch=B, device=DEV)
    g, loss = cond.loss_grad_x0(dev(x0), dev(y))
    w = cond.operator.taps(DEV)[2]
    assert float(loss[1]) == 0.0 and float(g[1].abs().max()) == 0.0
    assert np.array_equal(w[1].cpu().numpy(), cond.operator.host_taps()[2][1])          # its own set: the init, bit for bit
    assert torch.equal(w[0], wf[0]) and torch.equal(g[0], gf[0]) and float(loss[0]) == float(lf[0])
    assert not torch.equal(wf[1], w[1])


def test_fixed_per_image_psf_takes_the_weight_rows_of_a_chunk(pkg):
    """The three-launch route of a fixed PSF with one kernel per image: rows=(r0, r1) reads the weight rows [r0:r1]."""
    _, _, M, CM = pkg
    B, H, W = 3, 36, 34
    x0, y, mask = term_inputs(B, 4, H, W, True, seed=22)
    k = np.stack([M.motion_kernel(9, 0.5, s) for s in (3, 5, 8)])
    cond = CM.PosteriorSampling(M.get_operator("psf_blur", device=DEV, kernel=k, per_image=True, batch_size=B),
                                M.get_noise("gaussian", sigma=0.0), scale="0.3")
    cond.set_measurement_mask(mask, batch=B, device=DEV)
    g, loss = cond.loss_grad_x0(dev(x0), dev(y))
    g, loss = g.clone(), loss.clone()
    gc, lc = torch.empty_like(g), torch.empty_like(loss)
    cond.open_batch(B, (H, W), (H, W), torch.device(DEV))
    for r0, r1 in ((0, 2), (2, 3)):
        cond.loss_grad_x0(dev(x0[r0:r1]), dev(y[r0:r1]), g_out=gc[r0:r1], loss_out=lc[r0:r1], rows=(r0, r1))
    assert torch.equal(gc, g) and torch.equal(lc, loss)
    for b in range(B):                                                   # image b alone through a one-kernel psf_blur: the same bits
        one = CM.PosteriorSampling(M.get_operator("psf_blur", device=DEV, kernel=k[b]), M.get_noise("gaussian", sigma=0.0), scale="0.3")
        one.set_measurement_mask(mask[b:b + 1], batch=1, device=DEV)
        g1, l1 = one.loss_grad_x0(dev(x0[b:b + 1]), dev(y[b:b + 1]))
        ref = BO.loss_and_r(BO.conv_reflect(x0[b:b + 1, 0:3].double(), torch.from_numpy(k[b].astype(np.float32).astype(np.float64))),
                            y[b:b + 1].double(), mask[b:b + 1].double())[0]
        assert abs(float(l1[0]) - float(ref[0])) <= 2e-6 * float(ref[0])
        # the union tap list carries zeros where kernel b has no tap: an fma with w = 0 adds +-0, the sum is unchanged
        assert torch.allclose(g1[0], g[b], rtol=0, atol=0) and float(l1[0]) == float(loss[b]), b


def test_opcheck_of_ps_blind_loss_grad_s(pkg):
    x0, y, mask = term_inputs(2, 4, 20, 27, True)
    cond = blind_cond(pkg, 2, True, True, kernel_size=5, n_iter=2)
    dy, dx, w = cond.operator.taps(DEV)
    args = (dev(x0), dev(y), dev(mask), dy, dx, w.clone(), 2, 2, 2, 0.5, 0.0)
    torch.library.opcheck(torch.ops.osmosis.ps_blind_loss_grad_s.default, args)
    torch.library.opcheck(torch.ops.osmosis.ps_blind_loss_grad_s.default, args[:2] + (None,) + args[3:])
    torch.library.opcheck(torch.ops.osmosis.ps_blind_loss_grad_s.default, args[:5] + (w[:1].clone(),) + args[6:])
    wl = w.clone()
    loss, g = torch.ops.osmosis.ps_blind_loss_grad_s(dev(x0), dev(y), dev(mask), dy, dx, wl, 2, 2, 2, 0.5, 0.0)
    cond.set_measurement_mask(mask, batch=2, device=DEV)
    g2, loss2 = cond.loss_grad_x0(dev(x0), dev(y))
    assert torch.equal(g, g2) and torch.equal(loss, loss2) and torch.equal(wl, w) and not torch.equal(wl, dev(cond.operator.host_taps()[2]))


# ------------------------------------------------------------------------------------------------------------ 4: recovery
def _loss_at(pkg, x, y, K):
    """The data term's loss AT the kernels K float64 [nb,nc,k,k], through the fixed-PSF route."""
    _, _, M, CM = pkg
    nb, nc = K.shape[:2]
    kern = K[(slice(None) if nb > 1 else 0), (slice(None) if nc > 1 else 0)]
    op = M.get_operator("psf_blur", device=DEV, kernel=kern, normalize=False, per_image=nb > 1, per_channel=nc > 1, batch_size=x.shape[0])
    probe = CM.PosteriorSampling(op, M.get_noise("gaussian", sigma=0.0), scale="0.3")
    return probe.loss_grad_x0(dev(x.float()), dev(y.float()))[1].cpu().double().numpy()


@pytest.mark.parametrize("mode", ["per_image", "per_channel"])
def test_recovery_through_loss_grad_x0(pkg, mode):
    """tests/test_psfset_cpu.py's recovery problem through the kernels: every set's l1 distance to its true kernel <= 0.5 x the
    init's, every image's loss <= 0.25 x the first, the final sets against the float64 oracle under `kernel_bar`; and (per image)
    ONE kernel fitted to the same batch keeps both losses >= 0.5 x the first."""
    per_image, per_channel = MODES[mode]
    x, y, kstar, w0 = PO.recovery_problem_sets(per_image, per_channel)
    B = x.shape[0]
    one = blind_cond(pkg, B, per_image, per_channel, kernel_size=7, n_iter=1, eta=1.0)
    first = one.loss_grad_x0(dev(x.float()), dev(y.float()))[1].cpu().double().numpy()
    cond = blind_cond(pkg, B, per_image, per_channel, kernel_size=7, n_iter=200, eta=1.0)
    cond.loss_grad_x0(dev(x.float()), dev(y.float()))
    K = cond.operator.kernels()
    final = _loss_at(pkg, x, y, K)
    ref, bar, d = kernel_bar(x.float(), y.float(), None, w0, 7, 200, 1.0)
    ew = float(np.abs(K.reshape(w0.shape) - ref["w"].astype(np.float64)).max())
    for b in range(K.shape[0]):
        for c in range(K.shape[1]):
            d0 = np.abs(w0[b, c].astype(np.float64) - kstar[b, c].reshape(-1)).sum()
            d1 = np.abs(K[b, c] - kstar[b, c]).sum()
            print(f"PSFSETRECOVERY gpu {mode} set ({b},{c}): l1 distance {d0:.3f} -> {d1:.3f} ({d1 / d0:.3f})")
            assert d1 <= 0.5 * d0, (b, c)
            assert abs(K[b, c].sum() - 1.0) <= 1e-6 and (K[b, c] >= 0).all()
    print(f"PSFSETRECOVERY gpu {mode}: loss {first} -> {final} ({final / first}); sets vs float64 oracle {ew:.3e}; oracle float64 vs "
          f"float32 {d:.3e} (bar {bar:.3e})")
    assert (final <= 0.25 * first).all()
    assert ew <= bar
    if per_image:
        shared = blind_cond(pkg, B, False, False, kernel_size=7, n_iter=200, eta=1.0)
        shared.loss_grad_x0(dev(x.float()), dev(y.float()))
        sfinal = _loss_at(pkg, x, y, shared.operator.kernels())
        print(f"PSFSETRECOVERY gpu shared: loss ratios {sfinal / first}")
        assert (sfinal >= 0.5 * first).all()                             # one kernel cannot explain two shakes


# ------------------------------------------------------------------------------------------------------------ 5: the chains
def make_model(unet, kw):
    cfg = U.UNetConfig.from_create_model_kwargs(**kw)
    m = unet.create_model(**kw)
    m.load_state_dict(U.seeded_state_dict(cfg, 1234), strict=True)
    m = m.to(DEV).eval()
    m.conv_mode = "f32"
    return m


@pytest.fixture(scope="module")
def model36(pkg):
    return make_model(pkg[0], RGB_KW)


@pytest.fixture(scope="module")
def model48(pkg):
    return make_model(pkg[0], TINY_KW)


def make_sampler(gd, name="ddpm", **kw):
    args = dict(use_timesteps=range(0, 100, 10), betas=gd.get_named_beta_schedule("linear", 1000), model_mean_type="epsilon",
                model_var_type="learned_range", dynamic_threshold=False, clip_denoised=False, rescale_timesteps=False)
    args.update(kw)
    return gd.get_sampler(name)(**args)


def _no_generic(monkeypatch, sampler):
    def no_generic(*a, **k):
        raise AssertionError("the chain fell back to the generic loop")
    monkeypatch.setattr(type(sampler), "_generic_loop", no_generic)


def _replay_p_sample_draws(monkeypatch, noise):
    state, orig = {"k": 0}, torch.randn_like

    def replay(t, **kw):
        k = state["k"]
        state["k"] += 1
        return noise[k // 2].clone() if k % 2 == 0 else orig(t, **kw)
    monkeypatch.setattr(torch, "randn_like", replay)


CHAIN_OKW = dict(kernel_size=5, n_iter=2, eta=0.5, init_sigma=1.0)
SEEDS = [3, 5, 8]


def chain_inputs(B, C, n, seed=31):
    """x_T, the measurement y_b = A(motion_kernel(5, 0.5, SEEDS[b])) ref_b -- every image through its own shake --, the step noise."""
    from osmosis_diffusion_code_amd.guided_diffusion.measurements import motion_kernel
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H0, W0, generator=g)
    ref = torch.rand(B, 3, H0, W0, generator=g, dtype=torch.float64) * 1.6 - 0.8
    K = torch.from_numpy(np.stack([motion_kernel(5, 0.5, s) for s in SEEDS[:B]])[:, None])
    y = PO.conv_sets(ref, K).float()
    noise = torch.randn(n, B, C, H0, W0, generator=g)
    return x_T, y, noise


def chain_cond(pkg, kind, B=2, third_party=False, per_image=True):
    _, _, M, CM = pkg
    cls = type("ThirdPartyPS", (CM.PosteriorSampling,), {}) if third_party else CM.PosteriorSampling
    if kind == "blind":
        op = M.get_operator("blind_blur", device=DEV, batch_size=B, per_image=per_image, **CHAIN_OKW)
    else:
        op = M.get_operator("motion_blur", device=DEV, batch_size=B, kernel_size=5, seed=SEEDS[:B])
        if third_party:
            # `grad_and_value` keeps the reference's batch-global norm (one image there); `loss_grad_x0` defines the loss PER IMAGE.  The
            # autograd form of that definition: the sum of the images' norms (the images are independent through the network)
            def per_image_norms(self, x_prev, x_0_hat, measurement, **kwargs):
                diff = measurement - self.operator.forward(x_0_hat[:, 0:3])
                loss = torch.linalg.vector_norm(diff, dim=(1, 2, 3)).sum()
                return torch.autograd.grad(outputs=loss, inputs=x_prev)[0], loss
            cls = type("PerImagePS", (CM.PosteriorSampling,), {"grad_and_value": per_image_norms})
    return cls(op, M.get_noise("gaussian", sigma=0.0), scale="0.3")


_ORACLE = {}


def oracle_chain():
    """The oracle's DDPM chain on the tiny 3 -> 6 network with one learnt PSF per image (B = 2), once: the final image and kernels,
    their drift under a 1e-6 perturbation of x_T, and the kernels' distance to the same chain with the data term in float32."""
    if not _ORACLE:
        cfg = U.UNetConfig.from_create_model_kwargs(**RGB_KW)
        sd = U.seeded_state_dict(cfg, 1234)
        tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
        x_T, y, noise = chain_inputs(2, 3, 10)
        from osmosis_diffusion_code_amd.guided_diffusion.measurements import blind_init_kernel
        w0 = np.ascontiguousarray(np.broadcast_to(blind_init_kernel(5, "gaussian", 1.0).reshape(-1).astype(np.float32), (2, 1, 25)))

        def net(x, t):
            return U.unet_forward(sd, cfg, x, t)

        def run(x_start):
            return PO.ps_chain_sets(net, tb, x_start, y, list(noise), w0, 5, 5, 2, 0.5, 0.0, 0.3)
        img, w = run(x_T)
        bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
        pimg, pw = run(x_T + bump)
        orig = PO.inner_loop_sets
        try:
            PO.inner_loop_sets = lambda *a, **k: orig(*a, **dict(k, dtype=torch.float32))
            _, w32 = run(x_T)
        finally:
            PO.inner_loop_sets = orig
        _ORACLE.update(img=img, w=w, w0=w0, tb=tb, drift=float((pimg - img).abs().max()),
                       d_kernel=float(np.abs(w.astype(np.float64) - w32.astype(np.float64)).max()),
                       d_kernel_drift=float(np.abs(w.astype(np.float64) - pw.astype(np.float64)).max()))
    return _ORACLE


# case -> (operator, sampler, sampler kwargs, network, the tests/test_rgb_gpu.py chain whose bar applies)
CHAIN_CASES = {"ddpm": ("blind", "ddpm", {}, "c36", "rg.ddpm.c36"),
               "ddim.clip": ("blind", "ddim", dict(clip_denoised=True), "c36", "rg.ddim.c36"),
               "ddpm.c48": ("blind", "ddpm", {}, "c48", None),
               "fixed.motion": ("motion", "ddpm", {}, "c36", "rg.ddpm.c36")}


@pytest.mark.parametrize("tag", list(CHAIN_CASES))
def test_fused_per_image_chain_vs_the_generic_loop(pkg, monkeypatch, model36, model48, tag):
    """B = 2, one PSF per image (learnt, or a fixed `motion_blur(seed=[...])`): the fused loop against `_generic_loop` on the same
    injected draws at tests/test_rgb_gpu.py's fused-vs-generic bars (1e-4 for 4 -> 8), the two routes' final kernels under 5 x the
    oracle chain's float64 / float32 kernel distance."""
    _, gd, M, CM = pkg
    kind, sname, skw, net, ref_tag = CHAIN_CASES[tag]
    C, model, pretrain = (3, model36, "imagenet") if net == "c36" else (4, model48, "osmosis")
    if ref_tag is None:
        bar = 1e-4
    else:
        gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
        bar = min(5.0 * MEASURED_RGB[ref_tag], 10.0 * float(gold[f"{ref_tag}.drift_1e-6"]))
    kbar = 5.0 * oracle_chain()["d_kernel"]
    sampler = make_sampler(gd, sname, **skw)
    n = sum(a for _, _, a in gd.pcgs_schedule(PATTERN, sampler.num_timesteps))
    x_T, y, noise = (dev(t) for t in chain_inputs(2, C, n))
    kw = dict(model=model, x_start=x_T, measurement=y, record=False, save_root=None, pretrain_model=pretrain, rgb_guidance=True,
              sample_pattern=PATTERN)
    cond = chain_cond(pkg, kind)
    assert cond.operator.weight_sets == (2, 1) and not getattr(cond.operator, "couples_batch", False)
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, PATTERN, tuple(x_T.shape)) is cond
    _no_generic(monkeypatch, sampler)
    trace = []
    f = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: noise[k], trace=trace, **kw)
    monkeypatch.undo()
    kf = cond.operator.kernels()
    assert len(trace) == n and f.shape == x_T.shape and bool(torch.isfinite(f).all())
    if C == 3:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
    cond = chain_cond(pkg, kind, third_party=C == 4 or kind == "motion")
    assert sampler._fast_path_ok(model, cond.conditioning, pretrain, True, PATTERN, tuple(x_T.shape)) is None
    _replay_p_sample_draws(monkeypatch, noise)
    g = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **kw)
    monkeypatch.undo()
    kg = cond.operator.kernels()
    e, ek = float((f.cpu() - g.detach().cpu()).abs().max()), float(np.abs(kf - kg).max())
    moved = float(max(r["grad"].abs().max() for r in trace))
    print(f"PSFSETCHAIN {tag}: fused vs generic image {e:.3e} (bar {bar:.3e}), kernels {ek:.3e} (bar {kbar:.3e}); largest guidance "
          f"gradient {moved:.2e}")
    assert moved > 0.0 and e <= bar
    if kind == "blind":
        init = M.blind_init_kernel(5, "gaussian", 1.0).astype(np.float32).astype(np.float64)
        assert all(float(np.abs(kf[b, 0] - init).max()) > 1e-4 for b in range(2)) and not np.array_equal(kf[0], kf[1])
        assert ek <= kbar and np.abs(kf.sum(axis=(2, 3)) - 1.0).max() < 1e-6 and (kf >= 0).all()
    else:
        assert ek == 0.0


def test_fused_per_image_chain_vs_the_oracle_chain(pkg, monkeypatch, model36):
    _, gd, M, CM = pkg
    o = oracle_chain()
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(o["tb"].timestep_map)
    x_T, y, noise = chain_inputs(2, 3, 10)
    nd = dev(noise)
    cond = chain_cond(pkg, "blind")
    _no_generic(monkeypatch, sampler)
    f = sampler.p_sample_loop(model=model36, x_start=dev(x_T), measurement=dev(y), measurement_cond_fn=cond.conditioning, record=False,
                              save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k])
    assert o["drift"] <= 1e-4, o["drift"]
    bar, kbar = max(2e-5, 10.0 * o["drift"]), 10.0 * o["d_kernel_drift"]     # tests/test_blind_gpu.py's rule; the kernels by THEIR drift
    e = float((f.cpu() - o["img"]).abs().max())
    ek = float(np.abs(cond.operator.kernels().reshape(2, 1, 25) - o["w"].astype(np.float64)).max())
    print(f"PSFSETCHAIN oracle: image {e:.3e} (oracle drift_1e-6 {o['drift']:.2e}, bar {bar:.2e}); kernels {ek:.3e} (oracle float64 vs "
          f"float32 {o['d_kernel']:.3e}, under the perturbation {o['d_kernel_drift']:.3e}, bar {kbar:.3e})")
    assert e <= bar and ek <= kbar


def _counted_chain(pkg, monkeypatch, model36, per_image, chunks):
    """A B = 3 blind chain over indices 9 .. 5, walked as `chunks` (None: one pass).  Returns (image, kernels, the data term's calls as
    (images, rows), the engine forwards as batch sizes, which C entry points the data term used)."""
    from osmosis_diffusion_code_amd import engine, ops
    _, gd, M, CM = pkg
    x_T, y, noise = (dev(t) for t in chain_inputs(3, 3, 10, seed=32))
    data, fwd, entry = [], [], set()
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    cond = chain_cond(pkg, "blind", B=3, per_image=per_image)
    orig = cond.loss_grad_x0

    def counted(x0, *a, **k):
        data.append((x0.shape[0], k.get("rows")))
        return orig(x0, *a, **k)
    cond.loss_grad_x0 = counted
    run_forward = engine.UNetEngine.run_forward
    monkeypatch.setattr(engine.UNetEngine, "run_forward", lambda self: (fwd.append(self.B), run_forward(self))[1])
    for name in ("ps_blind_optimize", "ps_blind_optimize_s"):
        fn = getattr(ops, name)
        monkeypatch.setattr(ops, name, lambda *a, _fn=fn, _n=name, **k: (entry.add(_n), _fn(*a, **k))[1])
    if chunks is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B, cap: list(chunks)))
    img = sampler.p_sample_loop(model=model36, x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, record=False,
                                save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN,
                                noise_fn=lambda k, shape: noise[k], index_range=(9, 5))
    monkeypatch.undo()
    return img, cond.operator.kernels(), data, fwd, entry


def test_per_image_batch_of_three_walked_as_two_and_one_is_the_one_pass_chain(pkg, monkeypatch, model36):
    """One PSF per image leaves the images independent: the UNGROUPED walk -- per chunk one forward, one `loss_grad_x0(rows=)`, one
    backward, no re-forward -- and image and kernels equal the one-pass chain bit for bit."""
    whole, kw, data, fwd, entry = _counted_chain(pkg, monkeypatch, model36, True, None)
    assert bool(torch.isfinite(whole).all()) and data == [(3, (0, 3))] * 5 and fwd == [3] * 5 and entry == {"ps_blind_optimize_s"}
    chunked, kc, data, fwd, entry = _counted_chain(pkg, monkeypatch, model36, True, [2, 1])
    assert data == [(2, (0, 2)), (1, (2, 3))] * 5                        # once per chunk, with rows=
    assert fwd == [2, 1] * 5                                             # the network's forward once per chunk per sub-step
    assert torch.equal(chunked, whole) and np.array_equal(kc, kw)
    assert kw.shape == (3, 1, 5, 5) and len({kw[b].tobytes() for b in range(3)}) == 3


def test_shared_psf_keeps_the_grouped_walk_and_the_single_set_entry_point(pkg, monkeypatch, model36):
    """`per_image=False` is what it was: ONE data term over the batch through osm_ps_blind_optimize, a re-forward per chunk, and the
    chunked chain equal to the one-pass chain bit for bit."""
    whole, kw, data, fwd, entry = _counted_chain(pkg, monkeypatch, model36, False, None)
    assert data == [(3, (0, 3))] * 5 and fwd == [3] * 5 and entry == {"ps_blind_optimize"} and kw.shape == (1, 1, 5, 5)
    chunked, kc, data, fwd, entry = _counted_chain(pkg, monkeypatch, model36, False, [2, 1])
    assert data == [(3, (0, 3))] * 5 and fwd == [2, 1, 2, 1] * 5 and entry == {"ps_blind_optimize"}
    assert torch.equal(chunked, whole) and np.array_equal(kc, kw)


def test_refusals_before_any_launch_on_the_loop(pkg, model36):
    _, gd, M, CM = pkg
    sampler = make_sampler(gd)
    x_T, y, _ = (dev(t) for t in chain_inputs(2, 3, 10))
    kw = dict(model=model36, record=False, save_root=None, pretrain_model="imagenet", rgb_guidance=True, sample_pattern=PATTERN)
    cond = chain_cond(pkg, "blind", B=3)
    with pytest.raises(ValueError, match="per_image"):                   # a batch that is not nb
        sampler.p_sample_loop(x_start=x_T, measurement=y, measurement_cond_fn=cond.conditioning, **kw)
    assert np.array_equal(cond.operator.kernels()[0, 0], M.blind_init_kernel(5, "gaussian", 1.0).astype(np.float32).astype(np.float64))
    poisson = CM.PosteriorSampling(M.get_operator("blind_blur", device=DEV, batch_size=2, per_image=True, **CHAIN_OKW),
                                   M.get_noise("poisson", rate=1.0), scale="0.3")
    with pytest.raises(NotImplementedError, match="poisson"):
        sampler.p_sample_loop(x_start=x_T, measurement=y, measurement_cond_fn=poisson.conditioning, **kw)
    with pytest.raises(NotImplementedError, match="ps"):
        sampler.p_sample_loop(x_start=x_T, measurement=y, measurement_cond_fn=chain_cond(pkg, "blind").conditioning,
                              tiling=dict(tile=16, stride=8), **kw)
    with pytest.raises(NotImplementedError, match="robust"):
        sampler.p_sample_loop(x_start=x_T, measurement=y, measurement_cond_fn=chain_cond(pkg, "blind").conditioning,
                              robust=dict(loss="tukey"), **kw)


# ------------------------------------------------------------------------------------------------------------ 6: the driver
def test_restore_images_learns_one_kernel_per_image_and_writes_each(pkg, monkeypatch, model36, tmp_path):
    """`restore_images(batch_size=2)` with `blind_blur: {per_image: True}` over two photos with different shakes (`simulate_with:
    {name: motion_blur, seed: [3, 5]}`), 3-index sub-chains on the tiny 3 -> 6 network."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, M, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(41)
    images = [(torch.rand(1, 3, H0, W0, generator=g) * 1.6 - 0.8).to(DEV) for _ in range(2)]
    cfg = {"measurement": {"operator": dict(name="blind_blur", per_image=True,
                                            simulate_with=dict(name="motion_blur", kernel_size=5, intensity=0.5, seed=[3, 5]), **CHAIN_OKW),
                           "noise": {"name": "gaussian", "sigma": 0.0}},
           "conditioning": {"method": "ps", "params": dict(scale="0.3")},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="4"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": None}, "unet_model": {"pretrain_model": "imagenet"},
           "manual_seed": 0, "rgb_guidance": True}
    kw = dict(device=DEV, noise_seed=7, index_range=(3, 1))
    both = sampling.restore_images(model36, images, cfg, batch_size=2, **kw)
    single = sampling.restore_images(model36, images, cfg, batch_size=1, **kw)
    bumped = sampling.restore_images(model36, images, cfg, batch_size=1, x_scale=1.0 + 1e-6, **kw)      # x_T + 1e-6 x_T: a 1e-6 N(0, 1) bump
    assert cfg["measurement"]["operator"]["simulate_with"]["seed"] == [3, 5]                            # the caller's config stays
    init = M.blind_init_kernel(5, "gaussian", 1.0).astype(np.float32).astype(np.float64)
    for b in range(2):
        r, s = both[b], single[b]
        k = r["kernel"]
        assert k.dtype == torch.float32 and k.shape == (5, 5) and abs(float(k.double().sum()) - 1.0) <= 1e-6 and float(k.min()) >= 0.0
        assert float(np.abs(k.double().numpy() - init).max()) > 1e-4
        blurred = M.get_operator("motion_blur", device=DEV, kernel_size=5, intensity=0.5, seed=[3, 5][b]).forward(images[b]).cpu()
        assert torch.equal(r["measurement"], blurred) and torch.equal(s["measurement"], blurred)
        e = float((r["sample"] - s["sample"]).abs().max())
        ek = float((k.double() - s["kernel"].double()).abs().max())
        drift = float((bumped[b]["kernel"].double() - s["kernel"].double()).abs().max())
        print(f"PSFSETDRIVER image {b}: batch vs single sample {e:.3e} (bar 2e-5), kernel {ek:.3e}; the single run's kernel drift under a "
              f"1e-6 perturbation of x_T {drift:.3e} (bar {10 * drift:.3e})")
        assert e < 2e-5                                                  # tests/test_configs_gpu.py's batch-vs-single bar
        assert ek <= 10.0 * drift
        paths = sampling.save_outputs(r, images[b].cpu(), str(tmp_path), f"photo{b}")                  # a 3 -> 6 result: no depth tiles
        assert paths["kernel"].endswith(f"photo{b}_kernel.png") and os.path.exists(paths["kernel"]) and "depth_raw" not in paths
        assert sorted(paths) == ["grid", "input", "kernel", "rgb"]
    assert not torch.equal(both[0]["kernel"], both[1]["kernel"])
    # one PSF per colour plane: every result carries [3,k,k], written as one RGB picture
    pc = dict(cfg, measurement=dict(cfg["measurement"], operator=dict(cfg["measurement"]["operator"], per_channel=True)))
    res = sampling.restore_images(model36, images, pc, batch_size=2, **kw)
    assert res[0]["kernel"].shape == (3, 5, 5) and not torch.equal(res[0]["kernel"][0], res[0]["kernel"][1])
    paths = sampling.save_outputs(res[1], images[1].cpu(), str(tmp_path / "pc"), "photo")
    from PIL import Image
    assert np.asarray(Image.open(paths["kernel"])).shape == (125, 125, 3)
