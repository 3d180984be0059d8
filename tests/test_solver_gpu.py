"""Few-step solvers (DDIM, DPM-Solver++ 2M) on the HIP path.

Kernel level: osm_solver_update_c / osm_solver_update_rng_c against float64 on the vector, the scalar and the unaligned path, the
details of the contract (history, NaN, aliasing, batches, the in-kernel draw), torch.library.opcheck.
Chain level (the tiny 4 -> 8 and 3 -> 6 networks, 16 x 24, a 10-index chain, injected noise, `_generic_loop` patched to raise): a
DDPM-class sampler with `solver="ddim"` against the DDIM sampler's own fused chain, Osmosis chains against the oracle's loop with the
rule (tests/solver_oracle.py), bit-equalities of chunks / groups / one tile / `solver=None`, fused against `_generic_loop`,
`index_range`, and `restore_image` with the `diffusion: {solver, timestep_spacing}` config."""
import os

import numpy as np
import pytest
import torch

import depthprior_oracle as DO
import solver_oracle as SO
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from test_mask_gpu import (AUX, COND, OPERATORS, PATTERN, RGB_KW, TINY_KW, T, _free_running_bar, _no_generic, _replay_randn_like,
                           _same_bits, make_model, make_sampler, model36, model48, osmosis_cond, pkg)  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
EPS = 2.0 ** -24
GOLD = os.path.join(os.path.dirname(__file__), "golden")
CH, CW = 16, 24
USE = range(0, 100, 10)


# ============================================================================================================ kernel level
def rows_of(kind, eta=0.5):
    """fp32 rows [A, B0, B1, S, noise_on, 0, 0, t] of a 10-index chain: 'first' (B1 = 0), '2m' (B1 != 0), 'ddim' (S != 0)."""
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    s = make_sampler(gd)
    tab = gd.solver_table(s, "ddim", eta) if kind == "ddim" else gd.solver_table(s, "dpmpp_2m")
    i = 9 if kind == "first" else 5
    row = np.zeros(8, dtype=np.float32)
    row[0:4] = tab[i]
    row[4] = row[3] != 0
    assert (row[2] != 0) == (kind == "2m") and (row[3] != 0) == (kind == "ddim")
    return torch.from_numpy(row)


def kernel_inputs(B, C, H, W, seed, offset):
    """x0, x, hist, g, dxu, z [B,C,H,W] on the device; offset 1: every tensor starts one float past a 16-byte boundary."""
    gen = torch.Generator().manual_seed(seed)
    n = B * C * H * W
    out = []
    for k in range(6):
        v = torch.randn(n, generator=gen) * (0.02 if k in (3, 4) else 1.0)
        buf = torch.empty(n + 4, device=DEV)
        t = buf[offset:offset + n]
        t.copy_(v)
        out.append(t.view(B, C, H, W))
        assert t.data_ptr() % 16 == 4 * offset
    return out


def fresh(like, offset):
    buf = torch.full((like.numel() + 4,), float("nan"), device=DEV)
    return buf[offset:offset + like.numel()].view(like.shape)


GEOMETRIES = {"vector_36x34": (36, 34, 0), "scalar_5x7": (5, 7, 0), "unaligned_36x34": (36, 34, 1)}


@pytest.mark.parametrize("geo", list(GEOMETRIES))
@pytest.mark.parametrize("C", [3, 4])
def test_solver_update_vs_float64(pkg, C, geo):
    """B = 2; rows with B1 = 0, B1 != 0 and S != 0; with and without g / dx_unet / clip / noise / grad_out.  Per element
    |x_next - float64| <= 6 x 2^-24 (|A x| + |B0 x0| + |B1 h| + |S z| + |scale gc|): four products and four sums rounded once each,
    every partial sum bounded by the sum of the terms' magnitudes, and grad = fma(c0, g, dx_unet) with one rounding."""
    from osmosis_diffusion_code_amd import ops
    H, W, off = GEOMETRIES[geo]
    B, HW = 2, H * W
    x0, x, hist, g, dxu, z = kernel_inputs(B, C, H, W, 11 + C, off)
    coef = torch.tensor([1.37, -0.9, 0, 0, 0, 0, 1, 0], device=DEV)
    scale = torch.tensor([7.0, 7.0, 7.0, 0.9][:C], device=DEV)
    worst, worst_g, cases = 0.0, 0.0, 0
    for kind in ("first", "2m", "ddim"):
        row = rows_of(kind).to(DEV)
        A, B0, B1, S = (float(v) for v in row[:4].double())
        for guided, with_dxu, clip, with_noise, with_grad in [(True, True, 0.005, True, True), (True, False, -1.0, True, False),
                                                              (False, False, -1.0, True, True), (True, True, -1.0, False, True),
                                                              (True, True, 0.03, False, False)]:
            h = hist.clone()
            xn, go = fresh(x, off), fresh(x, off) if with_grad else None
            ops.solver_update_c(x0, x, h, g if guided else None, dxu if (guided and with_dxu) else None, z if with_noise else None, coef,
                                row, scale if guided else None, clip, xn, go, None, B, C, HW)
            grad = torch.zeros_like(x0, dtype=torch.float64)
            if guided:
                grad = float(coef[0].double()) * g.double() + (dxu.double() if with_dxu else 0.0)
            gc = grad.clamp(-clip, clip) if clip >= 0 else grad
            sg = scale.double().view(1, C, 1, 1) * gc if guided else torch.zeros_like(grad)
            terms = [A * x.double(), B0 * x0.double(), B1 * hist.double(), (S * z.double()) if with_noise else torch.zeros_like(grad)]
            want = terms[0] + terms[1] + terms[2] + terms[3] - sg
            bound = 6.0 * EPS * (sum(t.abs() for t in terms) + sg.abs())
            ratio = float(((xn.double() - want).abs() / bound).max())
            worst, cases = max(worst, ratio), cases + 1
            assert bool(torch.isfinite(xn).all()) and ratio <= 1.0, (C, geo, kind, guided, with_dxu, clip, with_noise, ratio)
            assert torch.equal(h, x0)
            if with_grad:
                gb = EPS * (grad.abs() + 1e-30)
                rg = float(((go.double() - grad).abs() / gb).max())
                worst_g = max(worst_g, rg)
                assert rg <= 1.0 or not guided, (C, geo, kind, rg)
                if not guided:
                    assert float(go.abs().max()) == 0.0
    print(f"SOLVERKERNEL C = {C} {geo}: worst |err| / bound {worst:.3f} over {cases} cases (grad_out: {worst_g:.3f} of one rounding)")


def test_solver_update_details(pkg):
    """hist <- x0; a NaN-filled hist under a B1 = 0 row is never read; a NaN in g reaches x_next at its element only; x_next aliasing
    x; B = 2 against two B = 1 calls; the scalar path gives the vector path's bits."""
    from osmosis_diffusion_code_amd import ops
    B, C, H, W = 2, 4, 36, 34
    HW = H * W
    x0, x, hist, g, dxu, z = kernel_inputs(B, C, H, W, 21, 0)
    coef = torch.tensor([1.37, -0.9, 0, 0, 0, 0, 1, 0], device=DEV)
    scale = torch.tensor([7.0, 7.0, 7.0, 0.9], device=DEV)

    def run(row, hist_in, gg=g, xin=None, out=None, sl=slice(0, B), off=0):
        h = hist_in[sl].clone()
        xi = x[sl] if xin is None else xin
        xn = torch.empty_like(x[sl]) if out is None else out
        go = torch.empty_like(x[sl])
        ops.solver_update_c(x0[sl], xi, h, gg[sl], dxu[sl], z[sl], coef, row.to(DEV), scale, 0.005, xn, go, None, sl.stop - sl.start, C, HW)
        return xn, go, h
    for kind in ("first", "2m", "ddim"):
        row = rows_of(kind)
        want = run(row, hist)
        assert torch.equal(want[2], x0) and bool(torch.isfinite(want[0]).all())
        alias = x.clone()
        got = run(row, hist, xin=alias, out=alias)
        assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], x0), kind
        for b in range(B):
            one = run(row, hist, sl=slice(b, b + 1))
            assert torch.equal(one[0], want[0][b:b + 1]) and torch.equal(one[1], want[1][b:b + 1]) and torch.equal(one[2], x0[b:b + 1])
        # the scalar path (one float off the alignment) gives the same bits
        shifted = [fresh(t, 1) for t in (x0, x, hist, g, dxu, z)]
        for s_, t in zip(shifted, (x0, x, hist, g, dxu, z)):
            s_.copy_(t)
        xn, go = fresh(x, 1), fresh(x, 1)
        ops.solver_update_c(shifted[0], shifted[1], shifted[2], shifted[3], shifted[4], shifted[5], coef, row.to(DEV), scale, 0.005, xn, go,
                            None, B, C, HW)
        assert torch.equal(xn, want[0]) and torch.equal(go, want[1]) and torch.equal(shifted[2], x0), kind
    nan_hist = torch.full_like(hist, float("nan"))
    for kind in ("first", "ddim"):                                       # B1 = 0: hist is not read
        got = run(rows_of(kind), nan_hist)
        assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], run(rows_of(kind), hist)[0]) and torch.equal(got[2], x0)
    assert not bool(torch.isfinite(run(rows_of("2m"), nan_hist)[0]).any())   # (B1 != 0 reads it)
    gn = g.clone()
    gn[1, 2, 7, 9] = float("nan")
    got, want = run(rows_of("2m"), hist, gg=gn), run(rows_of("2m"), hist)
    bad = torch.isnan(got[0])
    assert int(bad.sum()) == 1 and bool(bad[1, 2, 7, 9]) and torch.equal(got[0][~bad], want[0][~bad])
    assert bool(torch.isnan(got[1][1, 2, 7, 9])) and int(torch.isnan(got[1]).sum()) == 1


@pytest.mark.parametrize("C", [3, 4])
def test_in_kernel_noise_is_randn_sub_and_the_tensor_form(pkg, C):
    """osm_solver_update_rng_c: noise_out is bit-equal to osm_randn_sub at the same (seed, step, sub, image), x_next / grad_out / hist
    bit-equal to osm_solver_update_c fed that noise; a row with S = 0 draws nothing (noise_out = 0)."""
    from osmosis_diffusion_code_amd import ops
    B, H, W = 2, 36, 34
    HW = H * W
    x0, x, hist, g, dxu, _ = kernel_inputs(B, C, H, W, 31, 0)
    coef = torch.tensor([1.37, -0.9, 0, 0, 0, 0, 1, 0], device=DEV)
    scale = torch.tensor([7.0, 7.0, 7.0, 0.9][:C], device=DEV)
    step = torch.tensor([6], device=DEV, dtype=torch.int32)
    for kind, seed, sub, img0, stride in (("ddim", 1234, 0, 0, 1), ("ddim", 2 ** 40 + 17, 3, 5, 1), ("ddim", 99, 0, 2, 0), ("2m", 7, 0, 0, 1)):
        row = rows_of(kind).to(DEV)
        a = [torch.empty_like(x) for _ in range(3)]
        ha = hist.clone()
        ops.solver_update_rng_c(x0, x, ha, g, dxu, coef, row, scale, 0.005, a[0], a[1], a[2], B, C, HW, seed, step, step_offset=1,
                                sub=sub, img0=img0, img_stride=stride)
        zz = torch.empty(B, C * HW, device=DEV)
        ops.randn_sub(zz, B, C * HW, seed, step_const=7, sub=sub, img0=img0, img_stride=stride)
        want_z = zz.view(B, C, H, W) if kind == "ddim" else torch.zeros_like(x)
        assert torch.equal(a[2], want_z), (kind, seed, sub)
        if stride == 0:
            assert torch.equal(a[2][0], a[2][1])
        b = [torch.empty_like(x) for _ in range(3)]
        hb = hist.clone()
        ops.solver_update_c(x0, x, hb, g, dxu, want_z.contiguous(), coef, row, scale, 0.005, b[0], b[1], b[2], B, C, HW)
        for u, v in zip(a, b):
            assert torch.equal(u, v), (kind, seed, sub)
        assert torch.equal(ha, x0) and torch.equal(hb, x0)


def test_opcheck_of_the_solver_operator(pkg):
    from osmosis_diffusion_code_amd import ops
    B, C, H, W = 2, 4, 12, 10
    x0, x, hist, g, dxu, z = (t.clone() for t in kernel_inputs(B, C, H, W, 41, 0))
    coef = torch.tensor([1.37, -0.9, 0, 0, 0, 0, 1, 0], device=DEV)
    scale = torch.tensor([7.0, 7.0, 7.0, 0.9], device=DEV)
    row = rows_of("2m").to(DEV)
    xn, h = torch.empty_like(x), hist.clone()
    grad = torch.ops.osmosis.solver_update(x0, x, h, g, dxu, z, coef, row, scale, 0.005, xn)
    want, go, hw_ = torch.empty_like(x), torch.empty_like(x), hist.clone()
    ops.solver_update_c(x0, x, hw_, g, dxu, z, coef, row, scale, 0.005, want, go, None, B, C, H * W)
    assert torch.equal(xn, want) and torch.equal(grad, go) and torch.equal(h, x0)
    torch.library.opcheck(torch.ops.osmosis.solver_update.default, (x0, x, hist.clone(), g, dxu, z, coef, row, scale, 0.005, torch.empty_like(x)))
    torch.library.opcheck(torch.ops.osmosis.solver_update.default,
                          (x0, x, hist.clone(), None, None, None, coef, rows_of("ddim").to(DEV), scale, -1.0, torch.empty_like(x)))


# ============================================================================================================ chain level
def solver_sampler(gd, solver=None, eta=0.0, name="ddpm", **kw):
    extra = {} if solver is None else dict(solver=solver, solver_eta=eta)
    return make_sampler(gd, name, **extra, **kw)


def chain_inputs(B, C, seed, hw=(CH, CW), n=T):
    H, W = hw
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, C, H, W, generator=g)
    y = torch.rand(B, 3, H, W, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, C, H, W, generator=g)
    mask = torch.rand(B, 3, H, W, generator=g) * (torch.rand(B, 1, H, W, generator=g) > 0.3).float()
    yy, xx = torch.meshgrid(torch.linspace(0, 1, H), torch.linspace(0, 1, W), indexing="ij")
    z = torch.stack([1.0 + 2.5 * (0.3 * b + yy) + 1.5 * torch.exp(-((xx - 0.5) ** 2 + (yy - 0.4) ** 2) / 0.05) for b in range(B)])[:, None]
    m = (torch.rand(B, 1, H, W, generator=g) > 0.25).float() * (0.2 + 0.8 * torch.rand(B, 1, H, W, generator=g))
    z = torch.where(m > 0, z, torch.zeros_like(z))
    return x_T, y, noise, mask, z.contiguous(), m.contiguous()


def ref_setup(kw=TINY_KW):
    cfg = U.UNetConfig.from_create_model_kwargs(**kw)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), USE)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    return cfg, sd, tb


# The Osmosis chains against the oracle: (operator, rule, eta, mask, depth prior, tiled, first index).  Every one is a fixed CPU
# quantity whose oracle drift under a 1e-6 perturbation of x_T stays below 1e-4 (checked on the CPU when the seeds were chosen and
# asserted below), so none is skipped to teacher forcing.
OSMOSIS_CHAINS = {
    "revised+dpmpp_2m": ("underwater_physical_revised", "dpmpp_2m", 0.0, False, False, False, T - 1, 401),
    "haze+ddim_eta0.5": ("haze_physical", "ddim", 0.5, False, False, False, T - 1, 402),
    "revised+dpmpp_2m+mask+depth": ("underwater_physical_revised", "dpmpp_2m", 0.0, True, True, False, T - 1, 403),
    "tiled24x36+dpmpp_2m": ("underwater_physical_revised", "dpmpp_2m", 0.0, False, False, True, T - 1, 404),
    "revised+dpmpp_2m+index_range(4,0)": ("underwater_physical_revised", "dpmpp_2m", 0.0, False, False, False, 4, 405),
}
PRIOR = dict(weight=2.0, align="affine", loss="norm")


def oracle_osmosis_chain(case, bump=None):
    """The oracle's loop with the rule for one of OSMOSIS_CHAINS (B = 1).  Returns (trace, inputs)."""
    from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd
    from test_tiled_gpu import CANVAS, TILING, tiled_oracle_model
    opname, rule, eta, masked, prior, tiled, first, seed = OSMOSIS_CHAINS[case]
    cfg, sd, tb = ref_setup()
    x_T, y, noise, mask, z, m = chain_inputs(1, 4, seed, CANVAS if tiled else (CH, CW))
    if first != T - 1:
        x_T = 0.2 * x_T                     # a chain entered at a low-noise index starts from a state of that scale
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    rg = DO.make_guidance(opname, dict(okw, depth_type="gamma", value="1.4,1.4,1"), None, *x_T.shape[-2:], mask if masked else None, 20, AUX,
                          COND["loss_function"], COND["loss_weight"], dict(PRIOR, z=z, m=m) if prior else None, scale=COND["scale"],
                          gradient_clip=COND["gradient_clip"])
    net = lambda x, t: U.unet_forward(sd, cfg, x, t)  # noqa: E731
    if tiled:
        origins, wy, wx, inv = gd.tile_grid(*CANVAS, TILING["tile"], TILING["stride"], "hann")
        net = tiled_oracle_model(sd, cfg, origins, wy, wx, inv, *TILING["tile"])
    trace = []
    SO.osmosis_loop(net, tb, x_T if bump is None else x_T + bump, y, rg, PATTERN, [noise[k] for k in range(T)], rule, eta, first=first,
                    trace=trace)
    return trace, (x_T, y, noise, mask if masked else None, z, m)


def oracle_drift(case):
    ref, inputs = oracle_osmosis_chain(case)
    bump = 1e-6 * torch.randn(inputs[0].shape, generator=torch.Generator().manual_seed(99))
    pert, _ = oracle_osmosis_chain(case, bump)
    return ref, inputs, float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())


@pytest.mark.parametrize("case", list(OSMOSIS_CHAINS))
def test_fused_osmosis_chain_with_a_solver_vs_the_oracle(pkg, monkeypatch, model48, case):
    """The project's chain protocol (tests/test_mask_gpu.py): free-running, final image and pred_xstart under 10 x the oracle's own
    drift under a 1e-6 perturbation of x_T (floor 2e-5), loss 20 x that, phi 2e-6.  `index_range=(4, 0)` starts the oracle at index
    4 with empty history; the tiled case runs the 24 x 36 canvas as six 16 x 16 tiles against the oracle's tiled wrapper."""
    from test_tiled_gpu import TILING
    _, gd, _, _ = pkg
    opname, rule, eta, masked, prior, tiled, first, _ = OSMOSIS_CHAINS[case]
    ref, (x_T, y, noise, mask, z, m), drift = oracle_drift(case)
    assert drift <= 1e-4, f"{case}: oracle drift {drift:.2e} (the case was chosen to stay free-running)"
    bar = _free_running_bar(drift)
    sampler = solver_sampler(gd, rule, eta)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)
    cond = osmosis_cond(pkg, opname, PATTERN)
    kw = {}
    if prior:
        kw["depth_prior"] = dict(PRIOR, z=z, confidence=m)
    if tiled:
        kw["tiling"] = dict(TILING, window="hann")
    if first != T - 1:
        kw["index_range"] = (first, 0)
    trace = []
    sampler.p_sample_loop(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False,
                          save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                          noise_fn=lambda k, shape: nd[k], trace=trace, measurement_mask=mask, **kw)
    assert len(trace) == len(ref) == first + 1
    a, b, slots = trace[-1], ref[-1], cond.operator._slots()
    f_img, f_x0 = float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max())
    want = float(np.asarray(b["loss"]).reshape(-1)[0])
    f_loss = abs(float(a["loss"][0]) - want) / want
    f_phi = max(float((a["phi"][0, off:off + n].cpu() - b["phi"][name].reshape(-1)[:n]).abs().max()) for name, (off, n) in slots.items())
    msg = (f"SOLVERCHAIN {case}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
           f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}")
    print(msg)
    assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
    if rule == "ddim":                       # the injected noise entered: S != 0 above index 0
        assert float((trace[0]["x_out"].cpu() - ref[0]["x_out"]).abs().max()) < bar and eta > 0


# ------------------------------------------------------------------------------------------------------------ ps
MEASURED_RGB = {"rg.ddim.c36": 7.153e-07}      # tests/test_rgb_gpu.py MEASURED


def ps_cond(pkg, B=1):
    _, _, M, CM = pkg
    return CM.get_conditioning_method("ps", M.get_operator("noise", device=DEV, batch_size=B), M.get_noise("gaussian", sigma=0.0), scale="0.3")


def ps_bar():
    gold = np.load(os.path.join(GOLD, "loop_rgb.npz"))
    return min(5.0 * MEASURED_RGB["rg.ddim.c36"], 10.0 * float(gold["rg.ddim.c36.drift_1e-6"]))


def run_ps(pkg, monkeypatch, model, sampler, x_T, y, noise, fused=True, **kw):
    args = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), record=False, save_root=None, pretrain_model="imagenet",
                rgb_guidance=True, sample_pattern=PATTERN, **kw)
    cond = ps_cond(pkg, x_T.shape[0])
    nd = noise.to(DEV)
    if fused:
        _no_generic(monkeypatch, sampler)
        out = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, noise_fn=lambda k, shape: nd[k], **args)
    else:
        monkeypatch.setenv("OSM_FUSED_RGB", "0")
        assert sampler._fast_path_ok(model, cond.conditioning, "imagenet", True, PATTERN, tuple(x_T.shape)) is None
        _replay_randn_like(monkeypatch, nd, 3)
        out = sampler.p_sample_loop(measurement_cond_fn=cond.conditioning, **args)
    monkeypatch.undo()
    return out.detach()


@pytest.mark.parametrize("clip", [False, True], ids=["plain", "clip_denoised"])
def test_ps_ddpm_class_with_the_ddim_solver_equals_the_ddim_samplers_fused_chain(pkg, monkeypatch, model36, clip):
    """The kernels already pinned to the real reference: the `ddim` sampler's fused chain (osm_ddim_update_c) against a DDPM-class
    sampler with `solver="ddim"` (osm_solver_update_c) on the same inputs.  Bar: the one tests/test_rgb_gpu.py holds that DDIM chain
    to against `_generic_loop`, min(5 x measured, 10 x its recorded drift_1e-6)."""
    _, gd, _, _ = pkg
    x_T, y, noise = chain_inputs(1, 3, 411)[:3]
    want = run_ps(pkg, monkeypatch, model36, make_sampler(gd, "ddim", clip_denoised=clip), x_T, y, noise)
    got = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, "ddim", clip_denoised=clip), x_T, y, noise)
    also = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, "ddim", name="ddim", clip_denoised=clip), x_T, y, noise)
    e = float((got - want).abs().max())
    print(f"SOLVERPS ddim clip_denoised {clip}: solver vs the ddim sampler's fused chain {e:.3e} (bar {ps_bar():.3e})")
    assert bool(torch.isfinite(got).all()) and e <= ps_bar()
    assert torch.equal(also, got)                # (a solver replaces the class's own rule, whichever class)
    ancestral = run_ps(pkg, monkeypatch, model36, make_sampler(gd, "ddpm", clip_denoised=clip), x_T, y, noise)
    assert float((ancestral - want).abs().max()) > 100 * ps_bar()      # (another rule is far outside the bar)


def test_ps_chain_with_dpmpp_2m_vs_the_oracle(pkg, monkeypatch, model36):
    """A 3 -> 6 `ps` chain with dpmpp_2m against tests/solver_oracle.ps_loop, free-running at 10 x the oracle's own drift."""
    _, gd, _, _ = pkg
    cfg, sd, tb = ref_setup(RGB_KW)
    x_T, y, noise = chain_inputs(1, 3, 412)[:3]
    net = lambda x, t: U.unet_forward(sd, cfg, x, t)  # noqa: E731
    ref = SO.ps_loop(net, tb, x_T, y, 0.3, [noise[k] for k in range(T)], "dpmpp_2m")
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    drift = float((SO.ps_loop(net, tb, x_T + bump, y, 0.3, [noise[k] for k in range(T)], "dpmpp_2m") - ref).abs().max())
    assert drift <= 1e-4, drift
    bar = _free_running_bar(drift)
    got = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, "dpmpp_2m"), x_T, y, noise).cpu()
    e = float((got - ref).abs().max())
    print(f"SOLVERPS dpmpp_2m vs the oracle: {e:.3e} (oracle drift_1e-6 {drift:.2e}, bar {bar:.2e})")
    assert e < bar
    first_order = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, "ddim"), x_T, y, noise).cpu()
    assert float((first_order - ref).abs().max()) > 10 * bar            # (the history term matters at this bar)


# ------------------------------------------------------------------------------------------------------------ bit-equalities
def run_osmosis(pkg, monkeypatch, model, sampler, B, seed, sizes=None, groups=None, tiling=None, fused=True, library=False, hw=(CH, CW)):
    _, gd, M, CM = pkg
    x_T, y, noise, mask, z, m = chain_inputs(B, 4, seed, hw)
    nd = noise.to(DEV)
    if sizes is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: list(sizes)))
    gkw = {} if groups is None else dict(phi_groups=list(groups), phi_reduce="mean")
    operator = M.get_operator("underwater_physical_revised", device=DEV, batch_size=B, **OPERATORS["underwater_physical_revised"], **gkw)
    cond = CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **PATTERN, aux_loss=AUX)
    kw = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False, save_root=None,
              pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN)
    if tiling is not None:
        kw["tiling"] = tiling
    if fused:
        _no_generic(monkeypatch, sampler)
        noise_kw = dict(noise="library", noise_seed=77) if library else dict(noise_fn=lambda k, shape: nd[k])
        out = sampler.p_sample_loop(**noise_kw, **kw)
    else:
        cond.hip_ok = lambda: False
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, PATTERN, tuple(x_T.shape)) is None
        _replay_randn_like(monkeypatch, nd, 4)
        out = sampler.p_sample_loop(**kw)
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("rule,eta", [("dpmpp_2m", 0.0), ("ddim", 0.5)])
def test_chunks_groups_and_one_tile_bit_for_bit(pkg, monkeypatch, model48, rule, eta):
    """A B = 3 chain walked as chunks of [2, 1] is the one-pass chain (every chunk's rows of the history); a shared-water group
    [2, 1] likewise; one tile covering the canvas is the untiled chain.  ddim at eta = 0.5 draws its noise in the kernel here
    (`noise="library"`): the draw belongs to (seed, image, step), not to the walk."""
    _, gd, _, _ = pkg
    lib = rule == "ddim"
    s = lambda: solver_sampler(gd, rule, eta)  # noqa: E731
    whole = run_osmosis(pkg, monkeypatch, model48, s(), 3, 421, [3], library=lib)
    assert bool(torch.isfinite(whole[0]).all())
    _same_bits(run_osmosis(pkg, monkeypatch, model48, s(), 3, 421, [2, 1], library=lib), whole, f"{rule}: one pass vs chunks of [2, 1]")
    grouped = run_osmosis(pkg, monkeypatch, model48, s(), 3, 421, [3], groups=(2, 1), library=lib)
    _same_bits(run_osmosis(pkg, monkeypatch, model48, s(), 3, 421, [2, 1], groups=(2, 1), library=lib), grouped,
               f"{rule} + shared water: one pass vs chunks of [2, 1]")
    assert not torch.equal(grouped[0], whole[0])
    one = run_osmosis(pkg, monkeypatch, model48, s(), 1, 422, library=lib)
    tiled = run_osmosis(pkg, monkeypatch, model48, s(), 1, 422, tiling=dict(tile=(CH, CW), stride=(CH, CW), window="uniform"), library=lib)
    _same_bits(tiled, one, f"{rule}: one 16 x 24 tile vs the untiled fused chain")
    other = run_osmosis(pkg, monkeypatch, model48, make_sampler(gd), 1, 422, library=lib)
    assert not torch.equal(other[0], one[0])                              # (the ancestral chain is another chain)


def test_solver_none_is_the_sampler_built_without_the_keyword(pkg, monkeypatch, model48, model36):
    _, gd, _, _ = pkg
    for library in (False, True):
        a = run_osmosis(pkg, monkeypatch, model48, make_sampler(gd), 2, 423, library=library)
        b = run_osmosis(pkg, monkeypatch, model48, make_sampler(gd, solver=None, solver_eta=0.0), 2, 423, library=library)
        _same_bits(a, b, f"solver=None vs no keyword (library noise {library})")
    x_T, y, noise = chain_inputs(1, 3, 424)[:3]
    for name in ("ddpm", "ddim"):
        assert torch.equal(run_ps(pkg, monkeypatch, model36, make_sampler(gd, name), x_T, y, noise),
                           run_ps(pkg, monkeypatch, model36, make_sampler(gd, name, solver=None), x_T, y, noise)), name


# ------------------------------------------------------------------------------------------------------------ fused vs generic
@pytest.mark.parametrize("rule,eta", [("dpmpp_2m", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_fused_osmosis_chain_with_a_solver_equals_the_generic_loop(pkg, monkeypatch, model48, rule, eta):
    """Both loops with the same injected noise at the neighbouring suites' fused-versus-generic bars (image and pred_xstart 1e-4,
    loss rtol 1e-5, phi 1e-6)."""
    _, gd, _, _ = pkg
    f = run_osmosis(pkg, monkeypatch, model48, solver_sampler(gd, rule, eta), 2, 431)
    g = run_osmosis(pkg, monkeypatch, model48, solver_sampler(gd, rule, eta), 2, 431, fused=False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"SOLVERGENERIC osmosis {rule} eta {eta}: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6 and np.allclose(f[2], g[2], rtol=1e-5)


@pytest.mark.parametrize("rule,eta", [("dpmpp_2m", 0.0), ("ddim", 0.0), ("ddim", 0.5)])
def test_fused_ps_chain_with_a_solver_equals_the_generic_loop(pkg, monkeypatch, model36, rule, eta):
    """The 3 -> 6 `ps` chain, fused against `_generic_loop` (autograd over the HIP UNet), at tests/test_rgb_gpu.py's bar for the pair."""
    _, gd, _, _ = pkg
    x_T, y, noise = chain_inputs(1, 3, 432)[:3]
    f = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, rule, eta), x_T, y, noise)
    g = run_ps(pkg, monkeypatch, model36, solver_sampler(gd, rule, eta), x_T, y, noise, fused=False)
    e = float((f - g).abs().max())
    print(f"SOLVERGENERIC ps {rule} eta {eta}: fused vs generic {e:.3e} (bar {ps_bar():.3e})")
    assert bool(torch.isfinite(f).all()) and e <= ps_bar()


# ------------------------------------------------------------------------------------------------------------ the driver
def test_restore_image_with_a_solver_config(pkg, monkeypatch, model48):
    """`diffusion: {solver: dpmpp_2m, timestep_spacing: logsnr, timestep_respacing: "10"}` on a 3-index sub-chain: it runs fused, the
    results carry `solver` and `steps`, the sampler has the logsnr indices; without the keys the results have neither."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    seen = {}
    orig = gd.create_sampler

    def spy(**kw):
        seen["sampler"] = orig(**kw)
        return seen["sampler"]
    monkeypatch.setattr(sampling, "create_sampler", spy)
    ref = (torch.rand(1, 3, CH, CW, generator=torch.Generator().manual_seed(441)) * 1.2 - 0.6).to(DEV)
    diffusion = dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon", model_var_type="learned_range",
                     dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False, timestep_respacing="10")
    cfg = {"measurement": {"operator": dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised"),
                           "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)}, "diffusion": dict(diffusion, solver="dpmpp_2m", timestep_spacing="logsnr"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    res = sampling.restore_image(model48, ref, cfg, noise_seed=7, index_range=(2, 0), x_scale=0.1)[-1]
    assert res["solver"] == "dpmpp_2m" and res["steps"] == 10 and bool(torch.isfinite(res["sample"]).all())
    assert seen["sampler"].timestep_map == [0, 5, 22, 73, 202, 410, 603, 757, 886, 999] and seen["sampler"].solver == "dpmpp_2m"
    cfg["diffusion"] = diffusion
    plain = sampling.restore_image(model48, ref, cfg, noise_seed=7, index_range=(2, 0), x_scale=0.1)[-1]
    assert "solver" not in plain and "steps" not in plain and seen["sampler"].solver is None
    assert not torch.equal(plain["sample"], res["sample"])
