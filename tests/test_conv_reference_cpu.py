"""The fp64 convolution reference of tests/conv_reference.py can be trusted (no GPU): it agrees with F.conv2d / autograd in
double, its data gradient is the adjoint of its forward, its column sums agree with tests/gn_reference.py, the "ints" cases keep
their preconditions, every randn case's arithmetic model stays within HALF the bar the GPU test applies, and the case lists of
tests/test_conv_gpu.py reach every route of launch() in csrc/igemm.hip."""
import collections

import pytest
import torch
import torch.nn.functional as F

import conv_reference as R
import gn_reference as GN

F64 = torch.float64


@pytest.mark.parametrize("k,half", [(3, False), (1, False), (3, True)])
def test_forward_and_dgrad_agree_with_torch_in_double(k, half):
    c = R.case(2, 5, 7, 8, 6, k, "randn", half)
    x = c.x.to(F64).requires_grad_(True)
    y = F.conv2d(x, c.wref.to(F64), c.bias.to(F64), padding=k // 2)
    ref = R.epilogue_ref(c.y0, c.bias, c.res, c.prior, "all")
    assert torch.allclose(ref, y.detach() + c.res.to(F64) + c.prior.to(F64), rtol=0, atol=1e-13)
    (dx,) = torch.autograd.grad(y, x, c.dy.to(F64))
    assert torch.allclose(c.dx0, dx, rtol=0, atol=1e-13)
    if half:
        assert torch.equal(c.x, c.x.half().float()) and torch.equal(c.wref, c.w.half().float())
    for epi, (hb, hr, ha) in R.EPILOGUES.items():
        want = c.y0 + hb * c.bias.to(F64)[None, :, None, None] + hr * c.res.to(F64) + ha * c.prior.to(F64)
        assert torch.equal(R.epilogue_ref(c.y0, c.bias, c.res, c.prior, epi), want), epi


def test_dgrad_is_the_adjoint_of_forward():
    for k in (1, 3):
        c = R.case(2, 6, 5, 12, 8, k)
        lhs = float((c.y0 * c.dy.to(F64)).sum())
        rhs = float((c.x.to(F64) * c.dx0).sum())
        assert abs(lhs - rhs) <= 1e-12 * max(abs(lhs), 1.0), (k, lhs, rhs)


def test_rows_and_nchw_are_inverse():
    t = torch.arange(2 * 3 * 4 * 5, dtype=torch.float32).reshape(2, 3, 4, 5)
    assert torch.equal(R.nchw(R.rows(t), 2, 4, 5), t)
    assert torch.equal(R.rows(t)[1 * 20 + 2 * 5 + 3], t[1, :, 2, 3])


def test_fused_input_reference_is_group_norm_film_silu_then_padding():
    B, C, H, W, G = 2, 8, 5, 6, 4
    g = torch.Generator().manual_seed(3)
    x = torch.randn(B, C, H, W, generator=g) * 1.3 + 0.2
    gamma, beta, film = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g), 0.3 * torch.randn(B, 2 * C, generator=g)
    w = torch.randn(6, C, 3, 3, generator=g)
    xr = R.rows(x).reshape(B, H * W, C)
    table = GN.table(xr, G, gamma, beta, film)
    a = R.gn_input(x, table, True)
    assert torch.allclose(R.rows(a).reshape(B, H * W, C), GN.forward(xr, G, gamma, beta, film, True), rtol=0, atol=1e-12)
    y = F.group_norm(x.to(F64), G, gamma.to(F64), beta.to(F64), eps=1e-5)
    y = y * (1 + film[:, :C, None, None].to(F64)) + film[:, C:, None, None].to(F64)
    assert torch.allclose(R.conv64(a, w), F.conv2d(F.silu(y), w.to(F64), padding=1), rtol=0, atol=1e-9)   # eps as float32 in GN.stats
    assert torch.equal(R.gn_input(x, table, True, half=True), a.half().to(F64))


def test_column_sums_agree_with_the_group_norm_reference():
    c = R.case(2, 6, 5, 12, 8, 3)
    B, HW, C, G = 2, 30, 8, 4
    y = R.rows(c.y0).reshape(B, HW, C)
    cs = R.colsum_ref(y, 1)
    mean, rstd = GN.cols_combine(cs.reshape(B, 1, 2, C), B, 1, HW, C, G)
    m2, r2 = GN.stats(y, G)
    assert torch.allclose(mean, m2, rtol=0, atol=1e-12) and torch.allclose(rstd, r2, rtol=1e-10, atol=0)
    g = torch.Generator().manual_seed(5)
    xg = torch.randn(B, HW, C, generator=g) * 1.5 + 0.3
    gamma, beta = 1 + 0.1 * torch.randn(C, generator=g), 0.1 * torch.randn(C, generator=g)
    for silu in (True, False):
        cs2 = R.colsum_ref(y, 2, xg, GN.table(xg, G, gamma, beta), silu)
        a, b = GN.cols_combine(cs2.reshape(B, 1, 2, C), B, 1, HW, C, G, mode=1)
        _, m1, m2_ = GN.backward(xg, y, G, gamma, beta, silu=silu)
        assert torch.allclose(a, m1, rtol=1e-10, atol=1e-13) and torch.allclose(b, m2_, rtol=1e-10, atol=1e-13)


def _int_specs():
    return [s for s in R.SPECS if s.values == "ints"]


def test_ints_preconditions_hold_for_every_integer_case():
    """conv(|x|, |w|) + |bias| + |res| + |prior| < 2^24 everywhere (every partial sum in any order is an exact fp32 integer), all
    operands are integers, and for half storage |y_ref| <= 2048 (consecutive integers are halves up to there)."""
    assert len(_int_specs()) >= 40
    for s in _int_specs():
        half = s.arith == "f16"
        c = R.case(s.B, s.H, s.W, s.Cin, s.Cout, s.k, "ints", half)
        xin, bias, res, prior, _ = R.operands(c, s.dgrad)
        w = R.flip_t(c.w) if s.dgrad else c.w
        for t in (xin, w, bias, res, prior):
            assert torch.equal(t, t.round())
        assert torch.equal(c.w, (c.w / 4).round() * 4) and float(c.x.abs().max()) <= 4 and float(c.w.abs().max()) <= 8
        bound = R.conv64(xin.abs(), w.abs()) + bias.abs().to(F64)[None, :, None, None] + res.abs().to(F64) + prior.abs().to(F64)
        assert float(bound.max()) < 2 ** 24, R.spec_id(s)
        ref = R.spec_ref(s)
        assert float(ref.abs().max()) > 0
        if half:
            assert float(ref.abs().max()) <= 2048 and float(R.conv64(xin, w).abs().max()) <= 2048, (R.spec_id(s), float(ref.abs().max()))
            assert torch.equal(c.w, c.wref)
        assert torch.equal(R.store(ref, half), ref)
    for s in R.GEMM_SPECS:
        if s.values == "ints":
            c = R.gemm_case(s.M, s.N, s.K, s.b_kn, s.nb, "ints")
            b = torch.einsum("zmk,znk->zmn", c.A.abs().to(F64), c.Bm.abs().to(F64)) * abs(s.alpha) + 24
            assert float(b.max()) < 2 ** 24
            ref = R.gemm_ref(c, s.alpha, s.epi)
            assert torch.equal(ref, ref.round()) and torch.equal(ref.float().to(F64), ref)


def test_integer_cases_are_exact_in_every_arithmetic_model():
    """the precondition in action: the plane-rounded models (direct and Winograd domain) of integer cases ARE the reference"""
    done = set()
    for s in _int_specs():
        key = (s.arith, s.wino, s.k)
        if key in done or s.Cin * s.H * s.W > 40 * 17 * 19 * 4:
            continue
        done.add(key)
        assert torch.equal(R.spec_model(s), R.spec_ref(s)), R.spec_id(s)
    assert len(done) >= 10


def _randn_keys():
    """one representative per (shape, arithmetic, kernel family, fused input): the model does not depend on views or split-K"""
    seen = {}
    for s in R.SPECS:
        if s.values == "randn":
            seen.setdefault((s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.arith, s.wino, s.gn, s.dgrad, s.epi in ("none", "bias")), s)
    return list(seen.values())


def test_model_error_is_within_half_the_bar_for_every_randn_case():
    worst = collections.defaultdict(float)
    for s in _randn_keys():
        ref, mod = R.spec_ref(s), R.spec_model(s)
        tol = R.bar(s.arith, s.wino, s.gn)
        for b in range(s.B):
            e = float((mod[b] - ref[b]).abs().max() / ref[b].abs().max())
            worst[(s.arith, s.wino, s.gn)] = max(worst[(s.arith, s.wino, s.gn)], e / tol)
            assert e <= 0.5 * tol, (R.spec_id(s), b, e, tol)
    print({k: round(v, 3) for k, v in worst.items()})


def test_scales_cases_keep_their_bar_per_image():
    n = 0
    for s in R.SPECS:
        if s.values == "scales":
            ref, mod = R.spec_ref(s), R.spec_model(s)
            mx = [float(ref[b].abs().max()) for b in range(s.B)]
            assert mx[1] > 1e3 * mx[0] > 0
            for b in range(s.B):
                assert float((mod[b] - ref[b]).abs().max()) <= 0.5 * R.bar(s.arith, s.wino) * mx[b], (R.spec_id(s), b)
            n += 1
    assert n >= 5


def test_every_route_and_combine_is_reached():
    routes, combines, forms = collections.Counter(), collections.Counter(), collections.Counter()
    for s in R.SPECS:
        r = R.spec_reaches(s)
        if "refused" in r:
            continue
        routes[r["route"]] += 1
        combines[r["combine"]] += 1
        forms[(r["route"], r["epilogue"])] += 1
    for s in R.NT2_SPECS:
        r = R.spec_reaches(s, {"OSM_HALO_NT2": "2"})
        routes[r["route"]] += 1
    print(dict(routes), dict(combines), dict(forms))
    for name in R.ROUTES:
        assert routes[name] > 0, name
    for name in R.COMBINES:
        assert combines[name] > 0, name
    assert not [c for c in combines if c.startswith("refused")], combines
    # both epilogue forms of every split-plane kernel that has both
    for route in ("tap9", "tap1", "tap1_hp", "halo16", "halo8"):
        assert forms[(route, "vector")] > 0 and forms[(route, "scalar")] > 0, route
    # each combine with bias + res + accumulate; <1> through Cout % 4 and through ldy % 4; an empty last share on every K loop
    full = collections.Counter(R.spec_reaches(s)["combine"] for s in R.SPECS if s.epi == "all" and s.splitk > 1)
    for name in R.COMBINES:
        assert full[name] > 0, name
    one = [s for s in R.SPECS if R.spec_reaches(s).get("combine") == "reduce<1>"]
    assert any((s.Cin if s.dgrad else s.Cout) % 4 for s in one) and any((s.Cin if s.dgrad else s.Cout) % 4 == 0 for s in one)
    empty = collections.Counter()
    for s in R.SPECS:
        r = R.spec_reaches(s)
        if s.splitk > 1 and r["splitk"] > 1:
            K = s.Cout if s.dgrad else s.Cin
            chunks = (2 * R._cdiv(K, 32) if s.wino else R._cdiv(K, 32) * (1 if r["route"].startswith(("halo", "narrow")) else s.k * s.k))
            per = R._cdiv(chunks, r["splitk"])
            if per * (r["splitk"] - 1) >= chunks:
                empty[r["route"]] += 1
    for route in ("tap9", "tap1", "tap1_hp", "halo16", "halo8", "wino", "wino_hp"):
        assert empty[route] > 0, (route, dict(empty))
    # the switches re-route what they should
    for s in R.HALO0_SPECS:
        assert R.spec_reaches(s, {"OSM_CONV_HALO": "0"})["route"] == "tap9"
    assert {s.arith for s in R.HALO0_SPECS} == {"bf16x3", "bf16x6", "f16"} and len(R.HALO0_SPECS) >= 30
    for s in R.NARROW0_SPECS:
        assert R.spec_reaches(s)["route"] == "narrow" and R.spec_reaches(s, {"OSM_NARROW": "0"})["route"] == "halo16"
    assert len(R.NARROW0_SPECS) >= 20
    g = collections.Counter(R.reaches_gemm(s.M, s.N, s.K, s.b_kn, s.nb[0] * s.nb[1], s.splitk, s.ldc_extra == 0)["combine"]
                            for s in R.GEMM_SPECS)
    assert g["reduce<4>"] and g["reduce<1>"] and g["deep"], g


def test_reaches_refusals_and_forms():
    W = R.WINOGRAD
    assert R.reaches(2, 17, 19, 40, 96, 3, 3 | W, views=dict(y4=False))["refused"].startswith("the Winograd kernel stores")
    assert R.reaches(2, 8, 8, 64, 64, 3, 3 | W)["refused"].startswith("Winograd weight image")
    assert R.reaches(2, 16, 16, 64, 64, 3, 4 | W, gn=True)["refused"].startswith("the f16x3 Winograd image does not")
    assert R.reaches(2, 4, 4, 64, 64, 3, 4)["refused"].startswith("the direct f16x3 image")
    assert R.reaches(1, 10, 10, 64, 64, 1, 4)["refused"].startswith("the direct f16x3 kernel needs H * W")
    assert R.reaches(2, 9, 17, 40, 36, 3, 4, gn=True)["refused"].startswith("the f16x3 image does not")
    assert R.reaches(2, 9, 17, 40, 36, 3, 3, gn=True, env={"OSM_CONV_HALO": "0"})["refused"].startswith("osm_conv2d_nhwc: gn_table")
    assert R.reaches(2, 9, 17, 40, 36, 3, 4, env={"OSM_CONV_HALO": "0"})["refused"].startswith("the direct f16x3 image")
    assert R.reaches(2, 9, 17, 40, 36, 3, 0, colsum=1)["refused"].startswith("column sums are produced")
    assert R.reaches(2, 4, 4, 40, 36, 3, 3, colsum=1)["refused"].startswith("column sums are produced")
    assert R.reaches(2, 4, 4, 40, 70, 3, 3, splitk=2, colsum=1)["combine"].startswith("refused: column sums with split-K")
    assert R.reaches(2, 16, 16, 64, 64, 3, 4 | W)["kernel"] == "conv3_wino8_kernel<2,false,true,true>"
    assert R.reaches(2, 16, 16, 64, 64, 3, 4 | W, splitk=4)["kernel"] == "conv3_wino8_kernel<2,false,true,false>"
    assert R.reaches(2, 16, 16, 72, 64, 3, 4 | W)["kernel"] == "conv3_wino8_kernel<2,false,true,false>"
    assert R.reaches(2, 9, 17, 160, 36, 3, 3, splitk=4)["splitk"] == 4 and R.reaches(2, 9, 17, 160, 36, 3, 3, splitk=9)["splitk"] == 5
    assert R.reaches(1, 8, 8, 288, 36, 3, 3, splitk=8)["combine"] == "deep"
    assert R.reaches(2, 9, 17, 40, 256, 3, 1, family="f16", env={"OSM_HALO_NT2": "2"})["route"] == "halo_nt2"
    assert R.reaches(2, 9, 17, 40, 256, 3, 1, family="f16", views=dict(y4=False), env={"OSM_HALO_NT2": "2"})["route"] == "halo16"
