"""Shared water parameters across a burst on the HIP path (`phi_groups=` of the physical operators; include/osmosis_physgroup.h).

Kernel level: `loss_grad_x0` of a grouped operator against the oracle of a group (tests/physgroup_oracle.py), bit-equalities
(all-singleton groups against the ungrouped entry points, one C call against the single launches, repeats, two identical images as
one `mean` group, the independence of groups, freeze_phi, an ungrouped batch past the group limit), fully masked members,
torch.library.opcheck.
Chain level (the tiny 4 -> 8 network in f32, a 16 x 24 image, a 10-index respaced chain, injected noise, `_generic_loop` patched to
raise): B = 3 as groups [2, 1] against the oracle's own loop driven per group, a group walked in chunks, fused against
`_generic_loop`, `restore_images(shared_water=True)`."""
import os

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as D
from oracle import unet_ref as U
from physgroup_oracle import grouped_inner_loop, make_guidance
from physlin_oracle import DEGRADATIONS
from test_mask_gpu import (AUX, COND, OPERATORS, OPS, PATTERN, TINY_KW, T, _free_running_bar, _no_generic,
                           _replay_randn_like, _same_bits, etas, make_masks, make_sampler, model48, pkg)  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ETA = {"adam": 2e-3, "adadelta": 5e-2, "asgd": 2e-5}        # (else 1e-3; adadelta / asgd as tests/test_mask_gpu.py scales them)


def eta_of(optimizer):
    return ETA.get(optimizer, 1e-3)


def inputs(B, H, W, h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x0 = (0.6 * torch.randn(B, 4, H, W, generator=g)).clamp(-1.0, 1.0)      # depth >= -1: the gamma bases stay positive
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    return x0, y


def gcond(pkg, opname, B, groups, reduce="mean", optimizer="sgd", n_iter=5, aux=None, loss_function="norm", loss_weight="depth", deg=None,
          eta=None):
    _, _, M, CM = pkg
    okw = OPS[opname]
    kw = {} if groups is None else dict(phi_groups=list(groups), phi_reduce=reduce)
    oper = M.get_operator(opname, device=DEV, batch_size=B, optimizer=optimizer, degradation=deg, **okw,
                          **etas(okw, eta_of(optimizer) if eta is None else eta), **kw)
    return CM.get_conditioning_method("osmosis", oper, M.get_noise("clean"), loss_function=loss_function, loss_weight=loss_weight,
                                      weight_function="gamma,1.4,1.4,1", scale="7,7,7,0.9", gradient_x_prev=True,
                                      gradient_clip="False,0", n_iter=n_iter, aux_loss=aux, pattern="pcgs")


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
        assert torch.equal(a, b), (what, name, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------------ 1: against the oracle
# (name, B, image grid, groups, degradation): two reduce workgroups with a ragged tail; nblk = 5, the second round of the four-lane
# partial walk; more members than the finalize workgroup has waves, and no multiple of them; the composed route
SHAPES = [("b5_36x34_2+3", 5, (36, 34), (2, 3), None), ("b5_36x34_1+3+1", 5, (36, 34), (1, 3, 1), None),
          ("b3_74x58_3", 3, (74, 58), (3,), None), ("b9_8x12_9", 9, (8, 12), (9,), None),
          ("b3_36x34_blur_2+1", 3, (36, 34), (2, 1), "gaussian_blur"), ("b3_74x58_sr2box_2+1", 3, (74, 58), (2, 1), "sr2_box")]
# (operator, loss, weight, auxiliary losses, mask, reduce, optimizer): cycled, three per shape -- every operator, loss, weight, mask
# kind, reduce and optimizer code appears
CONFIGS = [("underwater_physical_revised", "norm", "depth", True, None, "mean", "sgd"),
           ("underwater_physical", "mse", "none", False, "uniform", "sum", "adam"),
           ("haze_physical", "norm", "none", True, "binary", "mean", "adamw"),
           ("underwater_physical_revised", "mse", "depth", False, "b1hw", "sum", "adamax"),
           ("underwater_physical", "norm", "depth", True, None, "sum", "rmsprop"),
           ("haze_physical", "mse", "depth", True, "uniform", "mean", "adagrad"),
           ("underwater_physical_revised", "norm", "none", False, "binary", "mean", "adadelta"),
           ("underwater_physical", "norm", "depth", True, "uniform", "mean", "asgd"),
           ("haze_physical", "norm", "depth", False, None, "sum", "rprop"),
           ("underwater_physical_revised", "norm", "depth", True, "uniform", "mean", "adam"),
           ("haze_physical", "mse", "none", True, None, "mean", "sgd"),
           ("underwater_physical", "mse", "depth", False, "binary", "sum", "sgd")]


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_grouped_loss_grad_x0_vs_the_oracle_of_each_group(pkg, shape):
    """Loss per image, phi after 5 inner iterations and dL/dx0 against autograd through the oracle of every group.  Bars: the ones
    tests/test_guidance_gpu.py / test_mask_gpu.py / test_physlin_gpu.py hold the per-image kernels to -- loss 3e-5 relative, phi
    3e-6 (5e-6 for the stateful optimizers), gradient 3e-5 of its largest entry per image; the cross-member sum is fp64."""
    name, B, (H, W), groups, degname = shape
    i = [s[0] for s in SHAPES].index(name)
    for k in range(3):
        cfg = CONFIGS[(3 * i + k) % len(CONFIGS)]
        opname, lf, lw, aux, mkind, reduce, optimizer = cfg
        aux = AUX if aux else None
        deg = None if degname is None else DEGRADATIONS[degname]
        cond = gcond(pkg, opname, B, groups, reduce, optimizer, 5, aux, lf, lw, deg)
        h, w = cond.operator.out_shape(H, W)
        x0, y = inputs(B, H, W, h, w, 100 + 3 * i + k)
        mask = None if mkind is None else make_masks(mkind, B, h, w, 1000 + 3 * i + k)
        if mask is not None:
            cond.set_measurement_mask(mask, batch=B, device=DEV)
        g, sep = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=False)
        g, sep, got_phi = g.cpu(), sep.cpu().numpy().astype(np.float64), {n: v.cpu() for n, v in cond.operator.variables().items()}
        okw = dict(OPS[opname], **etas(OPS[opname], eta_of(optimizer)))
        want_sep, want_phi, want_g = grouped_inner_loop(groups, opname, okw, cond.operator.degradation, x0.double(), y.double(),
                                                        None if mask is None else mask.double(), 5, optimizer, aux, lf, lw, reduce)
        e_loss = float((np.abs(sep - want_sep) / np.abs(want_sep)).max())
        e_phi = max(float((got_phi[n].double() - want_phi[n].double()).abs().max()) for n in want_phi)
        e_g = max(float((g[b].double() - want_g[b]).abs().max()) / float(want_g[b].abs().max()) for b in range(B))
        print(f"PHYSGROUP {name} {cfg}: loss(rel) {e_loss:.2e} phi {e_phi:.2e} grad {e_g:.2e} of its max")
        for lo, hi in zip(cond.operator.group_offsets[:-1], cond.operator.group_offsets[1:]):
            assert all(torch.equal(cond.operator.phi[lo], cond.operator.phi[b]) for b in range(lo, hi)), (name, cfg, lo, hi)
        assert e_loss <= 3e-5, (name, cfg, e_loss)
        assert e_phi <= (3e-6 if optimizer == "sgd" else 5e-6), (name, cfg, e_phi)
        assert e_g <= 3e-5, (name, cfg, e_g)


# ------------------------------------------------------------------------------------------------------------ 2: bit-equalities
# plain, masked, composed through a separable operator with the weight plane (P = 4), composed through a PSF without (P = 3)
ROUTES = {"plain": (None, None, "depth"), "masked": (None, "uniform", "depth"), "blur_P4": ("gaussian_blur", None, "depth"),
          "psf_P3_masked": ("psf_blur", "binary", "none")}
HW0 = (36, 34)


def route_run(pkg, route, groups, reduce="mean", optimizer="sgd", B=3, sl=None, py_loop=False, calls=1, seed=400, n_iter=5, freeze=False,
              monkeypatch=None, edit=None, eta=None, mask_edit=None, grid=HW0):
    degname, mkind, lw = ROUTES[route]
    H, W = grid
    cond = gcond(pkg, "underwater_physical_revised", B if sl is None else sl.stop - sl.start, groups, reduce, optimizer, n_iter, AUX, "norm",
                 lw, None if degname is None else DEGRADATIONS[degname], eta=eta)
    h, w = cond.operator.out_shape(H, W)
    x0, y = inputs(B, H, W, h, w, seed)
    mask = None if mkind is None else make_masks(mkind, B, h, w, seed + 1)
    if edit is not None:
        x0, y = edit(x0, y)
    if mask_edit is not None:
        mask = mask_edit(mask)
    if sl is not None:
        x0, y, mask = x0[sl], y[sl], None if mask is None else mask[sl]
    if mask is not None:
        cond.set_measurement_mask(mask, batch=x0.shape[0], device=DEV)
    if monkeypatch is not None:
        monkeypatch.setenv("OSM_PHYS_PY_LOOP", "1" if py_loop else "0")
    out = []
    for _ in range(calls):
        g, loss = cond.loss_grad_x0(x0.to(DEV), y.to(DEV), freeze_phi=freeze)
        out.append(snapshot(cond, g, loss))
    return out


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("route", list(ROUTES))
def test_singleton_groups_are_the_ungrouped_entry_points_bit_for_bit(pkg, route, optimizer):
    """Groups [1, 1, 1]: phi, loss, g, red and the optimizer state equal osm_phys_optimize / _m / _lin for both `reduce` values,
    after one call of 5 inner iterations and after a second one (adam's state carried on)."""
    want = route_run(pkg, route, None, optimizer=optimizer, calls=2)
    assert all(bool(torch.isfinite(t).all()) for t in want[1].values() if t is not None)
    for reduce in ("mean", "sum"):
        got = route_run(pkg, route, (1, 1, 1), reduce, optimizer, calls=2)
        same(got[0], want[0], (route, optimizer, reduce, "first call"))
        same(got[1], want[1], (route, optimizer, reduce, "second call"))


@pytest.mark.parametrize("route", list(ROUTES))
def test_one_call_is_the_single_launches_and_a_repeat_repeats(pkg, monkeypatch, route):
    """osm_phys_optimize(_lin)_g against OSM_PHYS_PY_LOOP=1 (reduce / osm_phys_finalize(_lin)_g / grad, one Python call each), groups
    [2, 1], adam, two calls; and the same call again gives the same bits."""
    want = route_run(pkg, route, (2, 1), "mean", "adam", calls=2, monkeypatch=monkeypatch)
    same(route_run(pkg, route, (2, 1), "mean", "adam", calls=2, monkeypatch=monkeypatch, py_loop=True)[1], want[1], (route, "single launches"))
    same(route_run(pkg, route, (2, 1), "mean", "adam", calls=2, monkeypatch=monkeypatch)[1], want[1], (route, "repeat"))
    assert not torch.equal(want[1]["phi"][0], want[1]["phi"][2]) and torch.equal(want[1]["phi"][0], want[1]["phi"][1])


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
@pytest.mark.parametrize("route", ["plain", "blur_P4"])
def test_two_identical_images_as_one_mean_group_are_the_single_image_run(pkg, route, optimizer):
    """(a + a) / 2 is exact in fp64: both rows of the pair equal the B = 1 ungrouped run on phi, loss, g, red and the state."""
    one = route_run(pkg, route, None, optimizer=optimizer, B=2, sl=slice(0, 1))[0]
    two = route_run(pkg, route, (2,), "mean", optimizer, B=2, edit=lambda x0, y: (x0[0:1].repeat(2, 1, 1, 1), y[0:1].repeat(2, 1, 1, 1)))[0]
    for b in range(2):
        same(two, one, (route, optimizer, f"row {b}"), rows=(slice(b, b + 1), slice(0, 1)))


def test_a_group_does_not_depend_on_the_other_groups(pkg):
    """B = 5 as [2, 3]: another image 0 leaves phi, loss, g, red and the state of the rows 2 .. 4 bit-identical (and moves the rows 0, 1)."""
    for route, optimizer in (("masked", "adam"), ("blur_P4", "sgd")):
        a = route_run(pkg, route, (2, 3), "mean", optimizer, B=5)[0]

        def other(x0, y):
            x0, y = x0.clone(), y.clone()
            x0[0], y[0] = -x0[0].flip(-1), y[0].flip(-2)
            return x0, y
        b = route_run(pkg, route, (2, 3), "mean", optimizer, B=5, edit=other)[0]
        same(b, a, (route, "rows 2..4"), rows=(slice(2, 5), slice(2, 5)))
        assert not torch.equal(a["phi"][1], b["phi"][1]) and torch.equal(b["phi"][0], b["phi"][1])


@pytest.mark.parametrize("route", ["plain", "masked", "blur_P4"])
def test_freeze_phi_is_the_ungrouped_call(pkg, route):
    want = route_run(pkg, route, None, optimizer="adam", freeze=True)[0]
    got = route_run(pkg, route, (2, 1), "sum", "adam", freeze=True)[0]
    same(got, want, (route, "freeze_phi"))
    assert torch.equal(got["phi"], gcond(pkg, "underwater_physical_revised", 3, None).operator.phi)


# B = 65: one image more than a group table holds (OSM_MAX_GROUPS = 64).  36 x 36 = 1296 pixels: two reduce workgroups, the second
# one partial, and no multiple of the gradient kernel's 256.
PAST_LIMIT = dict(B=65, grid=(36, 36), n_iter=3)


@pytest.mark.parametrize("route", ["plain", "masked", "blur_P4"])
def test_ungrouped_finalize_past_the_group_limit(pkg, route):
    """The per-image finalize shares its body with the grouped one but takes no group table: a batch of 65 runs (adam, 3 inner
    iterations, auxiliary losses), and phi, loss, g, red and the optimizer rows of images 0, 63 and 64 equal their own B = 1 runs
    bit for bit."""
    got = route_run(pkg, route, None, optimizer="adam", **PAST_LIMIT)[0]
    assert all(bool(torch.isfinite(t).all()) for t in got.values())
    for b in (0, 63, 64):
        one = route_run(pkg, route, None, optimizer="adam", sl=slice(b, b + 1), **PAST_LIMIT)[0]
        same(got, one, (route, f"image {b}"), rows=(slice(b, b + 1), slice(0, 1)))


def test_a_full_group_table_entry_beside_a_singleton(pkg):
    """The same batch as groups [64, 1] under `mean`: the singleton's rows equal the ungrouped B = 1 run of image 64 bit for bit (a
    group's sum starts from its first member), and the 64 members of the other group hold one phi row and one optimizer row."""
    got = route_run(pkg, "plain", (64, 1), "mean", "adam", **PAST_LIMIT)[0]
    one = route_run(pkg, "plain", None, optimizer="adam", sl=slice(64, 65), **PAST_LIMIT)[0]
    same(got, one, "the singleton", rows=(slice(64, 65), slice(0, 1)))
    for name in ("phi", "opt"):
        assert bool((got[name][0:64] == got[name][0:1]).all()), name
    assert not torch.equal(got["phi"][0], got["phi"][64]) and bool(torch.isfinite(got["phi"]).all())


# ------------------------------------------------------------------------------------------------------------ 3: masks
@pytest.mark.parametrize("route", ["masked", "psf_P3_masked"])
@pytest.mark.parametrize("reduce", ["mean", "sum"])
def test_one_member_of_a_pair_fully_masked(pkg, route, reduce):
    """Norm loss, a group of two whose member 1 is masked out: its loss is 0 and its g the auxiliary terms alone; phi steps with
    member 0's gradient -- bit-equal to member 0's own B = 1 run under `sum`, and under `mean` (the gradient halved: exact in
    binary) to that run with eta halved; both rows carry it."""
    def blank(mask):
        mask = mask.clone()
        mask[1] = 0.0
        return mask
    pair = route_run(pkg, route, (2,), reduce, "sgd", B=2, mask_edit=blank)[0]
    eta = eta_of("sgd") * (0.5 if reduce == "mean" else 1.0)
    one = route_run(pkg, route, None, optimizer="sgd", B=2, sl=slice(0, 1), eta=eta)[0]
    assert all(bool(torch.isfinite(t).all()) for t in pair.values() if t is not None)
    assert float(pair["loss"][1]) == 0.0
    assert torch.equal(pair["phi"][0], one["phi"][0]) and torch.equal(pair["phi"][1], one["phi"][0])
    assert torch.equal(pair["loss"][0], one["loss"][0]) and torch.equal(pair["g"][0], one["g"][0])
    H, W = HW0
    x0, _ = inputs(2, H, W, H, W, 400)                  # (route_run's x0: drawn before y, whatever the measurement's grid)
    xa = x0[1:2].clone().requires_grad_(True)
    (ga,) = torch.autograd.grad(D.aux_loss(xa, AUX), xa)
    assert float((pair["g"][1:2].cpu() - ga).abs().max()) < 3e-5 * float(ga.abs().max()) + 1e-9 and float(pair["g"][1, 3].abs().max()) == 0.0


@pytest.mark.parametrize("optimizer", ["sgd", "adam"])
def test_a_group_whose_members_are_all_masked_takes_no_step(pkg, optimizer):
    """[2, 1] with both members of the pair masked out: their phi rows and state rows are untouched (adam's step counter too), their
    losses 0; the third image steps as its own B = 1 run does."""
    def blank(mask):
        mask = mask.clone()
        mask[0:2] = 0.0
        return mask
    for route in ("masked", "psf_P3_masked"):
        got = route_run(pkg, route, (2, 1), "mean", optimizer, mask_edit=blank)[0]
        phi0 = gcond(pkg, "underwater_physical_revised", 3, None).operator.phi
        assert torch.equal(got["phi"][0:2], phi0[0:2]) and float(got["loss"][0:2].abs().max()) == 0.0
        assert not torch.equal(got["phi"][2], phi0[2])
        if got["opt"] is not None:
            assert float(got["opt"][0:2].abs().max()) == 0.0 and float(got["opt"][2].abs().max()) > 0
        one = route_run(pkg, route, None, optimizer=optimizer, sl=slice(2, 3))[0]
        same(got, one, (route, optimizer, "the third image"), rows=(slice(2, 3), slice(0, 1)))


# ------------------------------------------------------------------------------------------------------------ 4: torch.library
def test_opcheck_of_phys_loss_grad_g(pkg):
    from osmosis_diffusion_code_amd import torch_ops
    H, W = 12, 20
    cond = gcond(pkg, "underwater_physical_revised", 3, (2, 1), "mean", aux=AUX, n_iter=3)
    x0, y = (t.to(DEV) for t in inputs(3, H, W, H, W, 700))
    mask = make_masks("b1hw", 3, H, W, 701).to(DEV)
    icfg, fcfg = torch_ops.phys_config(cond._prepare(3, H * W, x0.device)["desc"])
    phi = cond.operator.phi.clone()
    args = (x0, y, mask, phi, icfg, fcfg, 3, False, [2, 1], "mean")
    loss, g, phi_new = torch.ops.osmosis.phys_loss_grad_g(*args)
    cond.set_measurement_mask(mask.cpu(), batch=3, device=DEV)
    g2, loss2 = cond.loss_grad_x0(x0, y, freeze_phi=False)
    assert torch.equal(loss, loss2) and torch.equal(g, g2) and torch.equal(phi_new, cond.operator.phi)
    assert torch.equal(phi_new[0], phi_new[1]) and not torch.equal(phi_new[0], phi_new[2])
    assert torch.equal(phi, gcond(pkg, "underwater_physical_revised", 3, None).operator.phi)          # functional: phi untouched
    # singleton groups are osmosis::phys_loss_grad, no mask
    l1, g1, p1 = torch.ops.osmosis.phys_loss_grad_g(x0, y, None, phi, icfg, fcfg, 3, False, [1, 1, 1], "sum")
    l0, g0, p0 = torch.ops.osmosis.phys_loss_grad(x0, y, phi, icfg, fcfg, 3, False)
    assert torch.equal(l1, l0) and torch.equal(g1, g0) and torch.equal(p1, p0)
    with pytest.raises(Exception, match="group_sizes"):
        torch.ops.osmosis.phys_loss_grad_g(x0, y, None, phi, icfg, fcfg, 3, False, [2, 2], "mean")
    torch.library.opcheck(torch.ops.osmosis.phys_loss_grad_g.default, args)
    torch.library.opcheck(torch.ops.osmosis.phys_loss_grad_g.default, (x0, y, None, phi, icfg, fcfg, 1, True, [3], "sum"))


# ============================================================================================================ chain level
CH, CW = 16, 24
GROUPS = (2, 1)
CHAINS = {
    "revised+sgd": ("underwater_physical_revised", "sgd", None, False),
    "haze+adam": ("haze_physical", "adam", None, False),
    "revised+sgd+mask": ("underwater_physical_revised", "sgd", None, True),
    "revised+sgd+gaussian_blur5": ("underwater_physical_revised", "sgd", dict(name="gaussian_blur", kernel_size=5, intensity=1.0), False),
}


def chain_inputs(B, h, w, seed, masked, n=T):
    g = torch.Generator().manual_seed(seed)
    x_T = 0.5 * torch.randn(B, 4, CH, CW, generator=g)
    y = torch.rand(B, 3, h, w, generator=g) * 1.6 - 0.8
    noise = torch.randn(n, B, 4, CH, CW, generator=g)
    mask = None
    if masked:
        mask = torch.rand(B, 3, h, w, generator=g) * (torch.rand(B, 1, h, w, generator=g) > 0.3).float()
        mask[:, :, 2:4, 3:7] = 0.0
    return x_T, y, noise, mask


def chain_okw(opname, optimizer):
    okw = dict(OPERATORS[opname], optimizer=optimizer)
    if optimizer == "adam":             # (adam's step is eta itself: a step size that keeps phi physical over 10 x 20 steps)
        okw.update({k: "1e-4" for k in okw if k.endswith("_eta")})
    return okw


def chain_cond(pkg, opname, optimizer, deg, groups, B=3, reduce="mean", pattern=PATTERN):
    _, _, M, CM = pkg
    kw = {} if groups is None else dict(phi_groups=list(groups), phi_reduce=reduce)
    operator = M.get_operator(opname, device=DEV, batch_size=B, degradation=deg, **chain_okw(opname, optimizer), **kw)
    return CM.get_conditioning_method("osmosis", operator, M.get_noise("clean"), **COND, **pattern, aux_loss=AUX)


def _oracle_group_chain(opname, optimizer, deg_op, cfg, sd, tb, x_T, y, noise, mask):
    """The oracle's p_sample_loop once per group, with the group's guidance; the traces concatenated over the batch."""
    okw = {k: v for k, v in chain_okw(opname, optimizer).items() if k.startswith("phi") and not k.endswith("flag")}
    traces, lo = [], 0
    for n in GROUPS:
        sl = slice(lo, lo + n)
        rg = make_guidance(opname, dict(okw, depth_type="gamma", value="1.4,1.4,1"), deg_op, CH, CW, None if mask is None else mask[sl], 20,
                           optimizer, AUX, COND["loss_function"], COND["loss_weight"], "mean", scale=COND["scale"],
                           gradient_clip=COND["gradient_clip"])
        trace = []
        D.p_sample_loop(lambda x, t: U.unet_forward(sd, cfg, x, t), tb, x_T[sl], y[sl], rg, PATTERN, [noise[k][sl] for k in range(T)], trace)
        traces.append(trace)
        lo += n
    merged = []
    for k in range(T):
        recs = [t[k] for t in traces]
        merged.append({"x_in": torch.cat([r["x_in"] for r in recs]), "x_out": torch.cat([r["x_out"] for r in recs]),
                       "x0": torch.cat([r["x0"] for r in recs]), "loss": np.concatenate([np.asarray(r["loss"]).reshape(-1) for r in recs]),
                       "phi": {name: torch.cat([r["phi"][name] for r in recs]) for name in recs[0]["phi"]}})
    return merged


@pytest.mark.parametrize("case", list(CHAINS))
def test_fused_grouped_chain_vs_the_oracle_driven_per_group(pkg, monkeypatch, model48, case):
    """B = 3 as groups [2, 1], free-running against the oracle's loop per group with the same weights, x_T, measurement and noise.
    Bars as tests/test_mask_gpu.py / test_physlin_gpu.py build theirs: from the oracle's own drift on this chain under a 1e-6
    perturbation of x_T (`_free_running_bar`: 10 x the drift, loss 20 x that, phi 2e-6); where the oracle cannot reproduce itself to
    1e-3, teacher-forced per index from the oracle's x_in and phi at the north-star 1e-3.  The phi rows of a group are equal at every
    recorded step."""
    _, gd, M, _ = pkg
    opname, optimizer, deg, masked = CHAINS[case]
    cfg = U.UNetConfig.from_create_model_kwargs(**TINY_KW)
    sd = U.seeded_state_dict(cfg, 1234)
    tb = D.Tables(D.named_beta_schedule("linear", 1000), range(0, 100, 10))
    deg_op = None if deg is None else M.build_degradation(deg, "cpu")
    h, w = (CH, CW) if deg_op is None else deg_op.out_shape(CH, CW)
    x_T, y, noise, mask = chain_inputs(3, h, w, 291, masked)
    torch.set_num_threads(max(1, min(8, os.cpu_count() or 1)))
    ref = _oracle_group_chain(opname, optimizer, deg_op, cfg, sd, tb, x_T, y, noise, mask)
    bump = 1e-6 * torch.randn(x_T.shape, generator=torch.Generator().manual_seed(99))
    pert = _oracle_group_chain(opname, optimizer, deg_op, cfg, sd, tb, x_T + bump, y, noise, mask)
    drift = float((pert[-1]["x_out"] - ref[-1]["x_out"]).abs().max())
    bar = _free_running_bar(drift)
    sampler = make_sampler(gd)
    assert sampler.timestep_map == list(tb.timestep_map)
    _no_generic(monkeypatch, sampler)
    nd = noise.to(DEV)

    def hip(x_start, index_range=None, phi0=None, k0=0):
        cond = chain_cond(pkg, opname, optimizer, deg, GROUPS)
        if phi0 is not None:
            for name, (off, m) in cond.operator._slots().items():
                cond.operator.phi[:, off:off + m] = phi0[name].reshape(3, -1)[:, :m].to(DEV)
        trace = []
        kw = {} if index_range is None else {"index_range": index_range}
        if mask is not None:
            kw["measurement_mask"] = mask
        sampler.p_sample_loop(model=model48, x_start=x_start.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                              record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                              noise_fn=lambda k, shape: nd[k0 + k], trace=trace, **kw)
        return trace, cond

    def errs(a, b, slots):
        e_phi = max(float((a["phi"][:, off:off + m].cpu() - b["phi"][n].reshape(3, -1)[:, :m]).abs().max()) for n, (off, m) in slots.items())
        want = np.asarray(b["loss"], dtype=np.float64)
        return (float((a["x_out"].cpu() - b["x_out"]).abs().max()), float((a["x0"].cpu() - b["x0"]).abs().max()),
                float((np.abs(a["loss"].cpu().numpy() - want) / want).max()), e_phi)

    def rows_equal(trace):
        for rec in trace:
            assert torch.equal(rec["phi"][0], rec["phi"][1]), (case, rec["idx"])
    if bar is not None:
        trace, cond = hip(x_T)
        assert len(trace) == T
        rows_equal(trace)
        assert not torch.equal(trace[-1]["phi"][0], trace[-1]["phi"][2])
        slots = cond.operator._slots()
        e_img, e_x0, e_loss, e_phi = (max(v) for v in zip(*(errs(a, b, slots) for a, b in zip(trace, ref))))
        f_img, f_x0, f_loss, f_phi = errs(trace[-1], ref[-1], slots)
        msg = (f"PHYSGROUPCHAIN {case}: free-running, oracle drift_1e-6 {drift:.2e}, bar {bar:.2e}: final image {f_img:.2e} x0 {f_x0:.2e} "
               f"loss(rel) {f_loss:.2e} phi {f_phi:.2e}; worst over the chain: x_out {e_img:.2e} x0 {e_x0:.2e} loss(rel) {e_loss:.2e} "
               f"phi {e_phi:.2e}")
        print(msg)
        assert f_img < bar and f_x0 < bar and f_loss < 20.0 * bar and f_phi < 2e-6, msg
        return
    # (teacher forcing hands over x_in and phi per index; a stateful optimizer's moments cannot be handed over)
    assert optimizer == "sgd", f"{case}: the oracle's drift {drift:.2e} > 1e-3 leaves only teacher forcing, which cannot carry adam's state"
    worst = [0.0, 0.0, 0.0, 0.0]
    for k in range(T):
        idx = T - 1 - k
        trace, cond = hip(ref[k]["x_in"], (idx, idx), None if k == 0 else ref[k - 1]["phi"], k0=k)
        rows_equal(trace)
        worst = [max(w_, e) for w_, e in zip(worst, errs(trace[0], ref[k], cond.operator._slots()))]
    msg = (f"PHYSGROUPCHAIN {case}: oracle drift_1e-6 {drift:.2e} > 1e-3, teacher-forced per index: x_out {worst[0]:.2e} x0 {worst[1]:.2e} "
           f"loss(rel) {worst[2]:.2e} phi {worst[3]:.2e}")
    print(msg)
    assert worst[0] < 1e-3 and worst[1] < 1e-3 and worst[2] < 2e-5 and worst[3] < 2e-6, msg


def _chain(pkg, monkeypatch, model, groups, sizes=None, optimizer="sgd", deg=None, masked=True, seed=292, reduce="mean"):
    _, gd, M, _ = pkg
    h, w = (CH, CW) if deg is None else M.build_degradation(deg, "cpu").out_shape(CH, CW)
    x_T, y, noise, mask = chain_inputs(3, h, w, seed, masked)
    nd = noise.to(DEV)
    sampler = make_sampler(gd)
    _no_generic(monkeypatch, sampler)
    if sizes is not None:
        monkeypatch.setattr(gd.GaussianDiffusion, "chunk_sizes", staticmethod(lambda B, cap: list(sizes)))
    cond = chain_cond(pkg, "underwater_physical_revised", optimizer, deg, groups, reduce=reduce)
    kw = {} if mask is None else {"measurement_mask": mask}
    out = sampler.p_sample_loop(model=model, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning,
                                record=False, save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=PATTERN,
                                noise_fn=lambda k, shape: nd[k], **kw)
    monkeypatch.undo()
    return out


@pytest.mark.parametrize("optimizer,deg", [("sgd", None), ("adam", dict(name="super_resolution", scale_factor=2, method="box"))])
def test_one_group_walked_in_chunks_is_the_one_pass_chain(pkg, monkeypatch, model48, optimizer, deg):
    """One group of three in one engine pass against the same chain walked as chunks of [2, 1] images (every chunk's forward, ONE
    data term over the batch, every chunk's forward again before its backward): bit for bit, with per-image masks."""
    whole = _chain(pkg, monkeypatch, model48, (3,), [3], optimizer, deg)
    chunked = _chain(pkg, monkeypatch, model48, (3,), [2, 1], optimizer, deg)
    assert bool(torch.isfinite(whole[0]).all())
    _same_bits(whole, chunked, "one group: one pass vs chunks of [2, 1]")
    for n, v in whole[1].items():
        assert torch.equal(v[0], v[1]) and torch.equal(v[0], v[2]), n
    # and the grouping matters: per-image phi gives another chain
    free = _chain(pkg, monkeypatch, model48, None, [3], optimizer, deg)
    assert not torch.equal(free[0], whole[0])
    # singleton groups through the two-phase step are the ungrouped chain, in one pass and in chunks
    _same_bits(_chain(pkg, monkeypatch, model48, (1, 1, 1), [3], optimizer, deg), free, "groups [1, 1, 1] vs ungrouped")
    _same_bits(_chain(pkg, monkeypatch, model48, (1, 1, 1), [2, 1], optimizer, deg, reduce="sum"), free, "groups [1, 1, 1] in chunks vs ungrouped")


def test_a_chunk_of_a_grouped_batch_is_refused_on_the_device(pkg):
    cond = chain_cond(pkg, "underwater_physical_revised", "sgd", None, (2, 1))
    x0, y = (t.to(DEV) for t in inputs(3, CH, CW, CH, CW, 5))
    cond.open_batch(3, (CH, CW), (CH, CW), DEV)
    with pytest.raises(ValueError, match="water group spans chunks"):
        cond.loss_grad_x0(x0[0:2], y[0:2], rows=(0, 2))


@pytest.mark.parametrize("case", ["plain", "local_M2", "clip_denoised"])
def test_grouped_fused_chain_equals_the_grouped_generic_loop(pkg, monkeypatch, model48, case):
    """Both loops on B = 3 as [2, 1] with the same mask and the same injected noise, at the bars tests/test_mask_gpu.py holds the
    ungrouped pairs to (image and pred_xstart 1e-4, loss rtol 1e-5, phi 1e-6)."""
    _, gd, _, _ = pkg
    pat = dict(PATTERN, local_M=2, s_start=0.6, s_end=0.2) if case == "local_M2" else PATTERN
    n = sum(a for _, _, a in gd.pcgs_schedule(pat, T))
    x_T, y, noise, mask = chain_inputs(3, CH, CW, 293, True, n)
    noise = noise.to(DEV)

    def run(fused):
        sampler = make_sampler(gd, clip_denoised=case == "clip_denoised")
        cond = chain_cond(pkg, "underwater_physical_revised", "sgd", None, GROUPS, pattern=pat)
        kw = dict(model=model48, x_start=x_T.to(DEV), measurement=y.to(DEV), measurement_cond_fn=cond.conditioning, record=False,
                  save_root=None, pretrain_model="osmosis", rgb_guidance=False, sample_pattern=pat, measurement_mask=mask)
        if fused:
            _no_generic(monkeypatch, sampler)
            out = sampler.p_sample_loop(noise_fn=lambda k, shape: noise[k], **kw)
        else:
            cond.hip_ok = lambda: False             # the conditioner declines the fused loop; its step (the grouped kernels) stays
            assert sampler._fast_path_ok(model48, cond.conditioning, "osmosis", False, pat, tuple(x_T.shape)) is None
            _replay_randn_like(monkeypatch, noise, 4)
            out = sampler.p_sample_loop(**kw)
        monkeypatch.undo()
        return out
    f, g = run(True), run(False)
    e_img, e_x0 = float((f[0].cpu() - g[0].detach().cpu()).abs().max()), float((f[3] - g[3]).abs().max())
    e_phi = max(float((f[1][k].cpu() - g[1][k].detach().cpu()).abs().max()) for k in f[1])
    print(f"PHYSGROUPGENERIC {case}: fused vs generic img {e_img:.2e} x0 {e_x0:.2e} phi {e_phi:.2e} loss {f[2]} / {g[2]}")
    assert e_img < 1e-4 and e_x0 < 1e-4 and e_phi < 1e-6
    assert np.allclose(f[2], g[2], rtol=1e-5)
    for k in f[1]:
        assert torch.equal(f[1][k][0], f[1][k][1]) and torch.equal(g[1][k][0], g[1][k][1])


# ------------------------------------------------------------------------------------------------------------ the driver
def test_restore_images_with_shared_water(pkg, monkeypatch, model48):
    """`restore_images(batch_size=2, shared_water=True)` on the 3-index low-noise sub-chain tests/test_physlin_gpu.py uses for its
    batched driver test: both results carry `water_group` = [0, 1] and the same phi, which is neither image's own (the batch-1
    runs'); a batch of one stays ungrouped; the caller's config is not touched."""
    from osmosis_diffusion_code_amd import sampling
    _, gd, _, _ = pkg
    monkeypatch.setattr(gd.GaussianDiffusion, "_generic_loop", lambda *a, **k: 1 / 0)
    g = torch.Generator().manual_seed(296)
    photos = [(torch.rand(1, 3, 256, 256, generator=g) * 1.2 - 0.6).to(DEV) for _ in range(3)]
    op_cfg = dict(OPERATORS["underwater_physical_revised"], name="underwater_physical_revised")
    op_cfg.update({k: "1e-3" for k in op_cfg if k.endswith("_eta")})
    cfg = {"measurement": {"operator": op_cfg, "noise": {"name": "clean"}},
           "conditioning": {"method": "osmosis", "params": dict(COND)},
           "diffusion": dict(sampler="ddpm", steps=1000, noise_schedule="linear", model_mean_type="epsilon",
                             model_var_type="learned_range", dynamic_threshold=False, clip_denoised=True, rescale_timesteps=False,
                             timestep_respacing="10"),
           "sample_pattern": dict(PATTERN), "aux_loss": {"aux_loss": AUX}, "unet_model": {"pretrain_model": "osmosis"},
           "manual_seed": 0, "rgb_guidance": False}
    sub = dict(index_range=(2, 0), x_scale=0.05)
    shared = sampling.restore_images(model48, photos, cfg, device=DEV, batch_size=2, shared_water=True, noise_seed=7, **sub)
    alone = sampling.restore_images(model48, photos[:2], cfg, device=DEV, batch_size=1, noise_seed=7, **sub)
    assert "phi_groups" not in cfg["measurement"]["operator"]
    assert sorted(shared) == [0, 1, 2] and shared[0]["water_group"] == [0, 1] == shared[1]["water_group"] and shared[2]["water_group"] == [2]
    assert all("water_group" not in r for r in alone.values())
    for name in ("phi_a", "phi_b", "phi_inf"):
        a, b = shared[0]["phi"][name], shared[1]["phi"][name]
        assert torch.equal(a, b) and bool(torch.isfinite(a).all()), name
        assert not torch.equal(a, alone[0]["phi"][name]) and not torch.equal(a, alone[1]["phi"][name]), name
    assert shared[0]["sample"].shape == (1, 4, 256, 256) and not torch.equal(shared[0]["sample"], shared[1]["sample"])
