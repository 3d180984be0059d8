"""The Levenberg-Marquardt phi solver (`optimizer: lm`, osm_phys_desc.optimizer = 9) on the HIP path, through the C ABI.

Kernel level: `loss_grad_x0` against the fp64 oracle (tests/lm_oracle.py) on the cases tests/test_philm_cpu.py vets
(`PARITY_CASES`: every compared decision has a margin >= 1e-3 in the oracle, asserted here again), two consecutive calls, and
bit-equalities (one C call against the single launches, B = 2 against two B = 1 calls, a repeat, freeze_phi against the sgd freeze
call, a fully masked image, a NaN pixel), and the refusals of osm_phys_* before any launch.
Bars: loss and gradient at the plain kernels' bars (3e-5 relative, 3e-5 of max |g| per image).  phi cannot be derived (the 3 x 3
blocks are ill-conditioned at small lambda), so it is measured: a float32 restatement of the oracle (fp32 pixel math, fp32 sums per
1024-pixel block) deviates 1.2e-7 from the fp64 oracle on these cases on the CPU (tests/test_philm_cpu.py, `PHI_FP32_MEASURED`);
the bar is 10 x that, PHI_BAR = 1.2e-6, to cover compiler contraction and expf differences between device and host.

Chain level (the tiny 4 -> 8 network in f32, a 16 x 24 image, a 10-index respaced chain, n_iter = 3, injected noise,
`_generic_loop` patched to raise): fused against the oracle's `p_sample_loop` with `LMGuidance` at the bars
tests/test_physgroup_gpu.py derives (10 x the oracle's own drift under a 1e-6 perturbation of x_T, phi 2e-6), fused against
`_generic_loop`, a B = 3 chain walked [2, 1], one tile covering the canvas."""
import os

import numpy as np
import pytest
import torch

import lm_oracle as L
from oracle import diffusion_ref as D
from oracle import unet_ref as U
from test_mask_gpu import (AUX, COND, OPERATORS, PATTERN, TINY_KW, T, _free_running_bar, _no_generic, _replay_randn_like, _same_bits,
                           chain_inputs, make_sampler, model48, pkg)  # noqa: F401  (fixtures)
from test_philm_cpu import PHI_FP32_MEASURED

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
PHI_BAR = 10.0 * PHI_FP32_MEASURED


def lm_cond(pkg, c, B=None, optimizer="lm"):
    _, _, M, CM = pkg
    kw = {} if c["lm_lambda"] is None else dict(lm_lambda=c["lm_lambda"])
    oper = M.get_operator(c["opname"], device=DEV, batch_size=c["B"] if B is None else B, optimizer=optimizer, **L.case_okw(c), **kw)
    return CM.get_conditioning_method("osmosis", oper, M.get_noise("clean"), loss_function=c["loss_function"], loss_weight=c["loss_weight"],
                                      weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True, gradient_clip="False,0",
                                      n_iter=c["n_iter"], aux_loss=AUX if c["aux"] else None, pattern="pcgs")


def snapshot(cond, g, loss):
    return {"g": g.clone(), "loss": loss.clone(), "phi": cond.operator.phi.clone(), "red": cond._state["red"].clone(),
            "opt": None if cond._opt is None else cond._opt.clone()}


def same(got, want, what, rows=None):
    for name in want:
        a, b = got[name], want[name]
        if a is None and b is None:
            continue
        if name == "red":
            a, b = a.view(-1, 16), b.view(-1, 16)
        if rows is not None:
            a, b = a[rows[0]], b[rows[1]]
        assert torch.equal(a, b) or (torch.equal(a.isnan(), b.isnan()) and torch.equal(a.nan_to_num(), b.nan_to_num())), \
            (what, name, float((a - b).abs().max()))


def run(pkg, c, sl=None, py_loop=False, monkeypatch=None, freeze=False, optimizer="lm", edit=None, calls=None):
    """The case on the device: a snapshot per call.  sl: the images of the batch to run; edit(x0, y, mask) -> the same, changed."""
    B = c["B"] if sl is None else sl.stop - sl.start
    cond = lm_cond(pkg, c, B, optimizer)
    if monkeypatch is not None:
        monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1" if py_loop else "0")
    out = []
    for k in range(c["calls"] if calls is None else calls):
        x0, y, mask = L.case_inputs(c, min(k, c["calls"] - 1))
        if edit is not None:
            x0, y, mask = edit(x0, y, mask)
        if sl is not None:
            x0, y, mask = x0[sl], y[sl], None if mask is None else mask[sl]
        if mask is not None and k == 0:
            cond.set_measurement_mask(mask.float(), batch=B, device=DEV)
        g, loss = cond.loss_grad_x0(x0.float().to(DEV), y.float().to(DEV), freeze_phi=freeze)
        out.append(snapshot(cond, g, loss))
    return out, cond


def check_against_the_oracle(c, got, what):
    want, gd = L.run_case(c)
    margins = L.compared_margins(gd)
    assert min(margins) >= L.MIN_MARGIN, (c["name"], min(margins))
    worst = [0.0, 0.0, 0.0]
    for k, (snap, (sep, g, phi9, state)) in enumerate(zip(got, want)):
        B = c["B"]
        loss = snap["loss"].cpu().numpy().astype(np.float64)
        e_loss = float((np.abs(loss - sep) / np.abs(sep)).max())
        kind = L.KINDS[c["opname"]]
        used = [0, 1, 2, 6, 7, 8] if kind == 1 else ([0, 6, 7, 8] if kind == 2 else list(range(9)))
        e_phi = float(np.abs(snap["phi"].cpu().numpy().astype(np.float64)[:, used] - phi9.astype(np.float64)[:, used]).max())
        gg = snap["g"].cpu().double()
        e_g = max(float((gg[b] - g[b]).abs().max()) / float(g[b].abs().max()) for b in range(B))
        print(f"PHILM {what} {c['name']} call {k}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} (bar {PHI_BAR:.1e}) grad {e_g:.2e} of its max; "
              f"min margin {min(margins):.2e}; decisions {[''.join(str(int(r['accept'])) for r in rs) for rs in gd.records]}")
        worst = [max(a, b) for a, b in zip(worst, (e_loss, e_phi, e_g))]
        # the decisions are the oracle's: lambda and the retry flag of the state row are what its state machine left
        opt = snap["opt"].cpu().numpy()
        assert np.array_equal(opt[:, L.LAMBDA], state[:, L.LAMBDA]) and np.array_equal(opt[:, L.RETRY], state[:, L.RETRY]), \
            (c["name"], k, opt[:, L.LAMBDA], state[:, L.LAMBDA])
        assert bool(torch.isfinite(snap["phi"]).all())
    assert worst[0] <= 3e-5 and worst[2] <= 3e-5, (c["name"], worst)
    assert worst[1] <= PHI_BAR, (c["name"], worst)


# ------------------------------------------------------------------------------------------------------------ 1: against the oracle
@pytest.mark.parametrize("c", L.PARITY_CASES, ids=[c["name"] for c in L.PARITY_CASES])
def test_lm_loss_grad_x0_vs_the_oracle(pkg, c):
    got, cond = run(pkg, c)
    nblk = (c["H"] * c["W"] + 1023) // 1024
    assert cond._state["desc"].optimizer == 9 and cond._state["part"].numel() == c["B"] * nblk * 32
    check_against_the_oracle(c, got, "vs oracle")
    if c["eta"].get("phi_b_eta") == 0.0:        # frozen slots keep their bits
        assert torch.equal(got[0]["phi"][:, 3:6], lm_cond(pkg, c).operator.phi[:, 3:6])


def test_two_consecutive_calls_vs_the_oracle(pkg):
    """lambda and the base carry over; the second call's x0 has moved, and its second step is rejected at the close."""
    got, _ = run(pkg, L.TWO_CALLS)
    check_against_the_oracle(L.TWO_CALLS, got, "two calls")


# ------------------------------------------------------------------------------------------------------------ 2: bit-equalities
def _case(name):
    return next(c for c in L.PARITY_CASES + [L.TWO_CALLS] if c["name"] == name)


@pytest.mark.parametrize("name", ["revised.reject_path", "revised.two_calls.mask", "haze.norm.depth.mask.aux"])
def test_one_call_is_the_single_launches_and_a_repeat_repeats(pkg, monkeypatch, name):
    c = _case(name)
    want, _ = run(pkg, c, monkeypatch=monkeypatch, calls=2)
    single, _ = run(pkg, c, monkeypatch=monkeypatch, py_loop=True, calls=2)
    again, _ = run(pkg, c, monkeypatch=monkeypatch, calls=2)
    for k in range(2):
        same(single[k], want[k], (name, "single launches", k))
        same(again[k], want[k], (name, "repeat", k))
    assert not torch.equal(want[0]["phi"], lm_cond(pkg, c).operator.phi)


@pytest.mark.parametrize("name", ["revised.norm.depth.aux", "uw.mse.none.mask", "revised.reject_path"])
def test_a_batch_of_two_is_two_single_calls(pkg, name):
    c = _case(name)
    both, _ = run(pkg, c)
    assert not torch.equal(both[0]["phi"][0], both[0]["phi"][1])
    for b in range(2):
        one, _ = run(pkg, c, sl=slice(b, b + 1))
        same(both[0], one[0], (name, f"image {b}"), rows=(slice(b, b + 1), slice(0, 1)))


@pytest.mark.parametrize("name", ["revised.norm.depth.aux", "uw.mse.none.mask"])
def test_freeze_phi_is_the_sgd_freeze_call(pkg, name):
    c = _case(name)
    got, cond = run(pkg, c, freeze=True)
    want, _ = run(pkg, c, freeze=True, optimizer="sgd")
    for k in ("g", "loss", "phi", "red"):
        assert torch.equal(got[0][k], want[0][k]), (name, k)
    fresh = lm_cond(pkg, c)
    assert torch.equal(got[0]["phi"], fresh.operator.phi)
    lam = 1.0 if c["lm_lambda"] is None else c["lm_lambda"]
    seeded = torch.zeros(c["B"], 20)
    seeded[:, L.LAMBDA] = lam
    assert torch.equal(got[0]["opt"].cpu(), seeded)                 # the state: the seeded lambda, nothing else


def test_a_fully_masked_image(pkg):
    """Image 1 masked out: loss 0, its phi and state rows untouched; image 0 is its own B = 1 run."""
    c = _case("haze.norm.depth.mask.aux")

    def blank(x0, y, mask):
        mask = mask.clone()
        mask[1] = 0.0
        return x0, y, mask
    got, _ = run(pkg, c, edit=blank)
    fresh = lm_cond(pkg, c)
    assert float(got[0]["loss"][1]) == 0.0 and torch.equal(got[0]["phi"][1], fresh.operator.phi[1])
    seeded = torch.zeros(20)
    seeded[L.LAMBDA] = c["lm_lambda"]
    assert torch.equal(got[0]["opt"][1].cpu(), seeded)
    assert bool(torch.isfinite(got[0]["g"]).all())
    one, _ = run(pkg, c, sl=slice(0, 1), edit=blank)
    same(got[0], one[0], "image 0", rows=(slice(0, 1), slice(0, 1)))
    assert not torch.equal(got[0]["phi"][0], fresh.operator.phi[0])


def test_a_nan_pixel_leaves_phi_finite_and_unchanged(pkg):
    """An x0 with one NaN pixel in image 1 (an ordinary input): its S is not finite, which counts as a reject with no base -- no
    step; phi stays what it was.  Image 0 is its own B = 1 run."""
    c = _case("revised.norm.depth.aux")

    def poke(x0, y, mask):
        x0 = x0.clone()
        x0[1, 1, 5, 7] = float("nan")
        return x0, y, mask
    got, _ = run(pkg, c, edit=poke)
    fresh = lm_cond(pkg, c)
    assert torch.equal(got[0]["phi"][1], fresh.operator.phi[1]) and bool(torch.isfinite(got[0]["phi"]).all())
    assert bool(torch.isnan(got[0]["loss"][1]))
    one, _ = run(pkg, c, sl=slice(0, 1), edit=poke)
    same(got[0], one[0], "image 0", rows=(slice(0, 1), slice(0, 1)))


# ------------------------------------------------------------------------------------------------------------ 3: refusals of the C ABI
def test_the_entry_points_refuse_before_any_launch(pkg):
    from osmosis_diffusion_code_amd import ops
    from osmosis_diffusion_code_amd._lib import OsmosisHipError, PhysDesc
    c = _case("revised.norm.depth.aux")
    cond = lm_cond(pkg, c)
    B, HW = c["B"], c["H"] * c["W"]
    x0, y, _ = L.case_inputs(c)
    x0, y = x0.float().to(DEV).contiguous(), y.float().to(DEV).contiguous()
    st = cond._prepare(B, HW, x0.device)
    d, part, red, loss, g = st["desc"], st["part"], st["red"], st["loss"], st["g"]
    phi, opt = cond.operator.phi, cond._opt
    phi0, opt0 = phi.clone(), opt.clone()
    f32 = dict(device=DEV, dtype=torch.float32)
    with pytest.raises(OsmosisHipError, match="opt_state"):
        ops.phys_optimize(d, x0, y, phi, part, red, loss, g, 4, False, None)
    with pytest.raises(OsmosisHipError, match="do_update"):
        ops.phys_finalize(d, part, red, phi, 4, loss, opt)
    with pytest.raises(OsmosisHipError, match=r"lm.*grouped"):
        ops.phys_optimize_g(d, ops.group_desc((1, 1), "mean"), x0, y, None, phi, part, red, loss, g, 4, False, opt)
    with pytest.raises(OsmosisHipError, match=r"lm.*grouped"):
        ops.phys_finalize_g(d, ops.group_desc((1, 1), "mean"), part, red, phi, 1, loss, opt)
    with pytest.raises(OsmosisHipError, match=r"lm.*composed"):
        ops.phys_reduce_lin(d, x0, phi, torch.zeros(B, 3, HW, **f32), part)
    with pytest.raises(OsmosisHipError, match=r"lm.*composed"):
        ops.phys_finalize_lin(d, HW, part, torch.zeros(B * 2, **f32), red, phi, 1, loss, opt)
    d3 = PhysDesc.from_buffer_copy(d)
    d3.kind, d3.weight_type, d3.gamma_avrg, d3.gamma_val = 3, 0, 0.0, 0.0
    with pytest.raises(OsmosisHipError, match=r"lm.*kind 3"):
        ops.phys_optimize(d3, x0, y, phi, part, red, loss, g, 1, True, opt)
    with pytest.raises(ValueError, match="32"):
        ops.phys_reduce(d, x0, y, phi, torch.empty(B * 2 * 16, **f32))
    torch.cuda.synchronize()
    assert torch.equal(phi, phi0) and torch.equal(opt, opt0)


# ============================================================================================================ chain level
CH, CW = 16, 24
LM_PATTERN = dict(PATTERN, n_iter=3)
CHAINS = {"revised": ("underwater_physical_revised", False, 91), "haze+mask": ("haze_physical", True, 91)}


def chain_okw(opname):
    return dict(OPERATORS[opname], optimizer="lm")


def chain_cond(pkg, opname, B=1):
    _, _, M, CM = pkg
    operator = M.get_operator(opname, device=DEV, batch_size=B, **chain_okw(opname))
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **LM_PATTERN, aux_loss=AUX)


def _oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask):
    okw = {k: v for k, v in OPERATORS[opname].items() if k.startswith("phi") and not k.endswith("flag")}
    rg = L.make_guidance(opname, dict(okw, depth_type="gamma", value="1.4,1.4,1"), 3, B=x_T.shape[0], mask=mask, aux=AUX,
                         loss_function=COND["loss_function"], loss_weight=COND["loss_weight"], scale=COND["scale"],
                         gradient_clip=COND["gradient_clip"])
    trace = []
    D.p_sample_loop(lambda x, t: U.unet_forward(sd, cfg, x, t), tb, x_T, y, rg, LM_PATTERN, [noise[k] for k in range(T)], trace)
    return trace


@pytest.mark.parametrize("case", list(CHAINS))
def test_fused_lm_chain_vs_the_oracle(pkg, monkeypatch, model48, case):
    """The fused chain against the oracle's loop with the LM guidance, same weights, x_T, measurement and noise, free-running.  Bars
    as tests/test_physgroup_gpu.py derives them: 10 x the oracle's own drift on this chain under a 1e-6 perturbation of x_T
    (`_free_running_bar`), loss 20 x that, phi 2e-6."""
    _, gd, _, _ = pkg
    opname, masked, seed = CHAINS[case]
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    x_T, y, noise, mask = chain_inputs(1, 4, seed)
    mask = mask if masked else None
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ref = _oracle_chain(opname, cfg, sd, tb, x_T, y, noise, mask)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert = _oracle_chain(opname, cfg, sd, tb, x_T + bump, y, noise, mask)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    assert bar is not None, f"{case}: the oracle's own drift {drift:.2e} > 1e-3"
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(tb.timestep_map)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)
    cond = chain_cond(pkg, opname)
    trace = []
    kw = {} if mask is None else {"measurement_mask": mask}
    sampler.p_sample_loop(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False,
                          save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=LM_PATTERN,
                          noise_fn=lambda k, shape: nd[k], trace=trace, **kw)
    assert len(trace) == T and cond._state["desc"].optimizer == 9
    slots = cond.operator._slots()

    def errs(a, b):
        e_phi = max(float((a["phi"][0, off:off + m].cpu() - b["phi"][n].reshape(-1)[:m]).abs().max()) for n, (off, m) in slots.items())
        want = float(np.asarray(b["loss"]).reshape(-1)[0])
        return (float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max()),
                abs(float(a["loss"][0]) - want) / want, e_phi)
    e_img, e_x0, e_loss, e_phi = (max(v) for v in zip(*(errs(a, b) for a, b in zip(trace, ref))))
    f_img, f_x0, f_loss, f_phi = errs(trace[-1], ref[-1])
    msg = (f"PHILMCHAIN {case}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
           f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}; worst over the chain: x_out {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
           f"phi {e_phi:.2e}")
    print(msg)
    assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg


def _chain(pkg, monkeypatch, model, B, sizes=None, tiling=None, fused=True, seed=95, masked=True):
    _, gd, _, _ = pkg
    x_T, y, noise, mask = chain_inputs(B, 4, seed)
    nd = noise.to(DEV)
    sampler = make_sampler(gd)
    if sizes is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B_, cap: list(sizes)))
    cond = chain_cond(pkg, "underwater_physical_revised", B)
    kw = dict(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False, save_root=None,
              pretrain_model="osmosis", rgb_guidance=False, sample_pattern=LM_PATTERN)
    if masked:
        kw["measurement_mask"] = mask
    if tiling is not None:
        kw["tiling"] = tiling
    if fused:
        _no_generic(monkeypatch, sampler)
        out = sampler.p_sample_loop(noise_fn=lambda k, shape: nd[k], **kw)
    else:
        cond.hip_ok = lambda: False             # the conditioner declines the fused loop; its step (the LM kernels) stays
        assert sampler._fast_path_ok(model, cond.conditioning, "osmosis", False, LM_PATTERN, tuple(x_T.shape)) is None
        _replay_randn_like(monkeypatch, nd, 4)
        out = sampler.p_sample_loop(**kw)
    monkeypatch.undo()
    assert cond._state["desc"].optimizer == 9
    return out


def test_fused_lm_chain_equals_the_generic_loop(pkg, monkeypatch, model48):
    """Both loops with the same mask and injected noise, at the bars tests/test_mask_gpu.py holds the sgd pairs to (image and
    pred_xstart 1e-4, loss rtol 1e-5, phi 1e-6)."""
    f, g = _chain(pkg, monkeypatch, model48, 1), _chain(pkg, monkeypatch, model48, 1, fused=False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"PHILMGENERIC: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6
    assert np.allclose(f[2], g[2], rtol=1e-5)


def test_chunks_and_one_tile_bit_for_bit(pkg, monkeypatch, model48):
    """A B = 3 chain walked as chunks of [2, 1] is the one-pass chain (every chunk takes its rows of phi and of the solver's state);
    one tile covering the canvas is the untiled chain."""
    whole = _chain(pkg, monkeypatch, model48, 3, [3])
    assert bool(torch.isfinite(whole[0]).all())
    _same_bits(_chain(pkg, monkeypatch, model48, 3, [2, 1]), whole, "lm: one pass vs chunks of [2, 1]")
    one = _chain(pkg, monkeypatch, model48, 1, masked=False)
    tiled = _chain(pkg, monkeypatch, model48, 1, masked=False, tiling=dict(tile=(CH, CW), stride=(CH, CW), window="uniform"))
    _same_bits(tiled, one, "lm: one 16 x 24 tile vs the untiled fused chain")
