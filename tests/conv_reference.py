"""fp64 reference of the convolution / GEMM family of csrc/igemm.hip, its arithmetic models, the dispatch written out as a
function, the case lists of tests/test_conv_gpu.py and the checkers (a helper, not a test; imports no GPU code: the runners
take the `ops` module as an argument, as tests/attn_reference.py does).

    y[b][o][h][w] = sum_{c, kh, kw} x[b][c][h + kh - p][w + kw - p] w[o][c][kh][kw]  (+ bias[o]) (+ res) (+ prior y)
    dx = the same with dy for x and wd[c][o][kh][kw] = w[o][c][k-1-kh][k-1-kw]        (the data gradient)

Everything is NCHW here and [B H W][C] ("nhwc rows") where the kernels see it.  tests/test_conv_reference_cpu.py checks the
references against F.conv2d / autograd in double, the column sums against tests/gn_reference.py, the "ints" preconditions, the
arithmetic models against the bars, and that the case lists reach every route."""
import functools
import math
from collections import namedtuple
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gn_reference import SENTINEL, Guarded

F64 = torch.float64
WINOGRAD = 0x10
WFMT = {"f32": 0, "f16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}
HALF_ULP = 2.0 ** -11          # tests/test_fp16_gpu.py (not imported here: that module imports the package)
NAN = float("nan")


# ------------------------------------------------------------------------------------------------ layout
def rows(t):
    """[B][C][H][W] -> [B H W][C]"""
    B, C, H, W = t.shape
    return t.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def nchw(m, B, H, W):
    return m.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def flip_t(w):
    """the data-gradient weights: a convolution of dy with flip_t(w) is the adjoint of the convolution of x with w"""
    return w.transpose(0, 1).flip(2, 3).contiguous()


def conv64(x, w):
    return F.conv2d(x.to(F64), w.to(F64), None, padding=w.shape[-1] // 2)


# ------------------------------------------------------------------------------------------------ cases
def _ints(g, shape, lo, hi, mul=1, keep=1.0):
    t = torch.randint(lo, hi + 1, shape, generator=g).float() * mul
    if keep < 1.0:
        t = t * (torch.rand(shape, generator=g) < keep).float()
    return t


@functools.lru_cache(maxsize=None)
def case(B, H, W, Cin, Cout, k, values="randn", half=False, seed=0):
    """Inputs (fp32 CPU tensors that the storage type holds exactly) and fp64 references of one layer.  Read-only: shared.
    x, w, bias, res, prior: the forward operands; dy, dbias, dres, dprior: the data gradient's (its output has Cin columns);
    wref: the weights the reference uses (half-rounded in the fp16 family); y0 / dx0: the bare convolutions."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * B + 131 * H + 17 * W + 3 * Cin + Cout + 977 * k)
    c = SimpleNamespace(B=B, H=H, W=W, Cin=Cin, Cout=Cout, k=k, values=values, half=half)
    xs, ys = (B, Cin, H, W), (B, Cout, H, W)
    if values == "ints":
        # every product and partial sum an integer below 2^24 (2048 for half storage): exact in every arithmetic and order;
        # x in {-4..4}, w in 4 {-2..2} keep the Winograd transforms integers too.  Half storage: sparser, smaller integers
        keep = min(1.0, 40.0 / (Cin * k * k)) if half else min(1.0, 600.0 / (Cin * k * k))
        xa = 2 if half else 4
        c.x, c.dy = _ints(g, xs, -xa, xa), _ints(g, ys, -xa, xa)
        c.w = _ints(g, (Cout, Cin, k, k), -2, 2, 4, keep)
        c.bias, c.dbias = _ints(g, (Cout,), -8, 8), _ints(g, (Cin,), -8, 8)
        c.res, c.prior = _ints(g, ys, -8, 8), _ints(g, ys, -8, 8)
        c.dres, c.dprior = _ints(g, xs, -8, 8), _ints(g, xs, -8, 8)
    else:
        c.x, c.dy = torch.randn(xs, generator=g), torch.randn(ys, generator=g)
        c.w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
        c.bias, c.dbias = torch.randn(Cout, generator=g), torch.randn(Cin, generator=g)
        c.res, c.prior = torch.randn(ys, generator=g), torch.randn(ys, generator=g)
        c.dres, c.dprior = torch.randn(xs, generator=g), torch.randn(xs, generator=g)
        if values == "scales":           # image b is 10^(4 b - 4) times its neighbour's size; no bias (it has no image)
            s = torch.tensor([10.0 ** (4 * b - 4) for b in range(B)]).reshape(B, 1, 1, 1)
            for n in ("x", "dy", "res", "prior", "dres", "dprior"):
                setattr(c, n, getattr(c, n) * s)
            c.bias, c.dbias = torch.zeros(Cout), torch.zeros(Cin)
        if half:
            for n in ("x", "dy", "res", "prior", "dres", "dprior"):
                setattr(c, n, getattr(c, n).half().float())
    c.wref = c.w.half().float() if half else c.w
    c.y0 = conv64(c.x, c.wref)
    c.dx0 = conv64(c.dy, flip_t(c.wref))
    return c


EPILOGUES = {"none": (0, 0, 0), "bias": (1, 0, 0), "res": (0, 1, 0), "both": (1, 1, 0), "acc": (0, 0, 1), "all": (1, 1, 1)}


def operands(c, dgrad):
    """(input, packed-weight selector, bias, res, prior, bare reference) of the forward or the data-gradient layer"""
    if dgrad:
        return c.dy, c.dbias, c.dres, c.dprior, c.dx0
    return c.x, c.bias, c.res, c.prior, c.y0


def epilogue_ref(base, bias, res, prior, epi):
    hb, hr, ha = EPILOGUES[epi]
    y = base.clone()
    if hb:
        y = y + bias.to(F64)[None, :, None, None]
    if hr:
        y = y + res.to(F64)
    if ha:
        y = y + prior.to(F64)
    return y


# ------------------------------------------------------------------------------------------------ fused GroupNorm input
def gn_table(B, C, seed=0):
    """a [B][4][C] table mean | rstd | g | b of plausible values (the kernels take any table: gn_prep is not under test)"""
    g = torch.Generator().manual_seed(4242 + seed + C)
    return torch.stack([0.1 * torch.randn(B, C, generator=g), 1 + 0.1 * torch.rand(B, C, generator=g),
                        1 + 0.1 * torch.randn(B, C, generator=g), 0.1 * torch.randn(B, C, generator=g)], 1).contiguous()


def gn_input(x, table, silu=True, half=False):
    """act((x - mean) rstd g + b) per image and channel, fp64; the zero padding comes AFTER it (conv64 pads its input).
    half: the DIRECT fp16 kernels (halo-tile) store the transformed input as half before the product; the Winograd kernel
    transforms in fp32 and rounds only V, so its reference takes half=False."""
    t = table.to(F64)
    m, r, ga, be = (t[:, i, :, None, None] for i in range(4))
    z = (x.to(F64) - m) * r * ga + be
    a = z * torch.sigmoid(z) if silu else z
    return a.half().to(F64) if half else a


# ------------------------------------------------------------------------------------------------ column sums
def colsum_ref(y, mode, stat_x=None, table=None, silu=True):
    """[B][2][C] from y [B][HW][C] (fp64).  mode 1: (sum y, sum y^2).  mode 2: y is the gradient w.r.t. act(xh g + b),
    xh = (stat_x - mean) rstd: (sum dxh, sum dxh xh), dxh = y act'(z) g."""
    y = y.to(F64)
    if mode == 1:
        return torch.stack([y.sum(1), (y * y).sum(1)], 1)
    t = table.to(F64)
    m, r, ga, be = (t[:, i:i + 1, :] for i in range(4))
    xh = (stat_x.to(F64) - m) * r
    z = xh * ga + be
    s = torch.sigmoid(z)
    dxh = y * (s * (1 + z * (1 - s)) if silu else 1.0) * ga
    return torch.stack([dxh.sum(1), (dxh * xh).sum(1)], 1)


# ------------------------------------------------------------------------------------------------ arithmetic models
def _planes(t, kind, n):
    """t (fp64, holding fp32 values) as n planes of bf16 or half, each the rounding of what the earlier ones left"""
    out, r = [], t.to(F64)
    for _ in range(n):
        p = r.float().to(torch.bfloat16 if kind == "bf16" else torch.float16).to(F64)
        out.append(p)
        r = r - p
    return out


def _pow2_scale(t, dims):
    """2^e per slice that brings max |t| into [2^13, 2^14) (the f16x3 kernels' scale)"""
    mx = t.abs().amax(dim=dims, keepdim=True).clamp_min(1e-300)
    return torch.exp2(14 - (torch.floor(torch.log2(mx)) + 1))


_G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=F64)
_BT = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=F64)
_AT = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=F64)


def model(arith, x, w, wino=False):
    """fp64 convolution of the operands rounded the way `arith` rounds them, without the product terms it drops: the error the
    arithmetic has by construction (accumulation order and the final store apart).  x [B][C][H][W] (already transformed if a
    GroupNorm is fused), w [O][C][k][k]; the data gradient is model(arith, dy, flip_t(w))."""
    x, w = x.to(F64), w.to(F64)
    if arith == "f32":
        return conv64(x, w)
    B, C, H, W = x.shape
    kind, n = {"f16": ("f16", 1), "bf16x3": ("bf16", 2), "bf16x6": ("bf16", 3), "f16x3": ("f16", 2)}[arith]
    if not wino:
        sx = _pow2_scale(x, (1, 2, 3)) if arith == "f16x3" else 1.0
        sw = _pow2_scale(w, (0, 1, 2, 3)) if arith == "f16x3" else 1.0
        xp, wp = _planes(x * sx, kind, n), _planes(w * sw, kind, n)
        y = sum(conv64(xp[a], wp[b]) for a in range(n) for b in range(n - a))
        return y / sx / sw
    # F(2x2, 3x3): U = G g G^T, V = B^T d B rounded to planes in the transform domain, Y = A^T (sum_c U V) A
    Hp, Wp = H + (H & 1), W + (W & 1)
    xpad = F.pad(x, (1, 1 + Wp - W, 1, 1 + Hp - H))
    d = xpad.unfold(2, 4, 2).unfold(3, 4, 2)                                   # [B][C][th][tw][4][4]
    sx = _pow2_scale(x, (1, 2, 3)).reshape(B, 1, 1, 1, 1, 1) if arith == "f16x3" else 1.0
    V = _BT @ (d * sx) @ _BT.T
    U = _G @ w @ _G.T                                                          # [O][C][4][4]
    su = _pow2_scale(U, (0, 1, 2, 3)) if arith == "f16x3" else 1.0
    Vp, Up = _planes(V, kind, n), _planes(U * su, kind, n)
    Mx = sum(torch.einsum("bctuij,ocij->botuij", Vp[a], Up[b]) for a in range(n) for b in range(n - a))
    Y = _AT @ (Mx / sx / su) @ _AT.T                                           # [B][O][th][tw][2][2]
    Y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, w.shape[0], Hp, Wp)
    return Y[:, :, :H, :W].contiguous()


def store(y, half):
    """the final store: to float, or to half in the fp16 family"""
    return y.half().to(F64) if half else y.float().to(F64)


# ------------------------------------------------------------------------------------------------ bars
def bar(arith, wino=False, gn=False):
    """The project's tolerances (relative to max |ref|).  A fused GroupNorm input has its own bar in the fp32-class arithmetics
    (6e-6) and in the DIRECT f16 kernels (6 HALF_ULP); bf16x3 keeps its (wider) arithmetic bar, which already contains it, and
    f16 Winograd keeps 1.5e-3 with or without a fused input."""
    base = {"f32": 5e-6, "bf16x6": 4e-6, "f16x3": 4e-6, "bf16x3": 3e-4 if wino else 2e-4,
            "f16": 1.5e-3 if wino else 1.5 * HALF_ULP}[arith]
    if gn and not (arith == "f16" and wino):
        base = max(base, 6 * HALF_ULP if arith == "f16" else 6e-6)
    return base


COLSUM_BAR = {1: 1e-5, 2: 2e-5}
GEMM_BAR = 2e-6


# ------------------------------------------------------------------------------------------------ dispatch, from launch()
ROUTES = ("f32", "tap9", "tap1", "tap1_hp", "halo16", "halo8", "narrow", "halo_nt2", "wino", "wino_hp_pipe", "wino_hp")
COMBINES = ("reduce<4>", "reduce<1>", "deep", "stats")


def _cdiv(a, b):
    return (a + b - 1) // b


def wino_shape_ok(H, W, K, N):
    return H >= 16 and W >= 16 and K >= 16 and N >= 64 and N % 32 == 0 and H * W * K * 4 < (1 << 30)


def _combine(sk, colsum, M, N, HW, v4, nbatch=1, sx4=True):
    if sk <= 1:
        return "none"
    if colsum == 2 and not sx4:
        return "refused: column sums with split-K read stat_x / stat_table as 4-element vectors"
    if colsum:
        if not (N % 4 == 0 and v4 and M % 8 == 0 and HW % 8 == 0 and nbatch == 1):
            return "refused: column sums with split-K need"
        return "stats"
    if v4 and nbatch == 1 and sk >= 8 and nbatch * M * N // 4 <= 64 * 1024:
        return "deep"
    return "reduce<4>" if v4 else "reduce<1>"


def reaches(B, H, W, Cin, Cout, k, wfmt, splitk=1, views=None, gn=False, colsum=0, family="f32", env=None):
    """What launch() in csrc/igemm.hip does with a layer: dict(route, kernel, epilogue, combine, splitk, nch, tile), or
    dict(refused=<start of the message>).  views: y4 (ldy % 4 == 0 and y aligned to 4 elements), r4 (no res, or the same for
    res), sx4 (the same for stat_x).  env: the process-wide switches OSM_CONV_HALO, OSM_NARROW, OSM_HALO_NT2.
    If the dispatch changes, this function is updated, not the assertions of the tests."""
    v = dict(y4=True, r4=True, sx4=True)
    v.update(views or {})
    env = env or {}
    halo_on = env.get("OSM_CONV_HALO", "1")[0] != "0"
    narrow_on = env.get("OSM_NARROW", "1")[0] != "0"
    wino, wf = bool(wfmt & WINOGRAD), wfmt & ~WINOGRAD
    N, K, M, HW, taps = Cout, Cin, B * H * W, H * W, k * k
    out4 = v["y4"] and v["r4"]
    nchunks = taps * _cdiv(K, 32)
    sk = max(1, min(splitk, nchunks))
    if (family == "f16") != (wf == 1):
        return dict(refused="fp16 activations go with the fp16 weight image")
    if gn and not (wf != 0 and k == 3 and W >= 8 and H >= 8 and halo_on):
        return dict(refused="osm_conv2d_nhwc: gn_table needs the halo-tile kernel")
    if wino:
        if not (k == 3 and 1 <= wf <= 4 and wino_shape_ok(H, W, K, N)):
            return dict(refused="Winograd weight image")
        if not out4:
            return dict(refused="the Winograd kernel stores 4-element vectors")
        ksteps = 2 * _cdiv(K, 32)
        sk = min(sk, ksteps)
        if colsum == 2 and not v["sx4"]:
            return dict(refused="the Winograd kernel reads stat_x")
        route = "wino"
        if wf == 4:
            if gn:
                return dict(refused="the f16x3 Winograd image does not take a fused GroupNorm input")
            pipe = K % 16 == 0 and _cdiv(ksteps, sk) >= 4
            kernel = f"conv3_wino8_kernel<2,false,true,{'true' if pipe else 'false'}>"
            route = "wino_hp_pipe" if pipe else "wino_hp"
        else:
            kernel = f"conv3_wino8_kernel<{wf},{'true' if gn else 'false'}>"
        comb = _combine(sk, colsum, M, N, HW, True)
        nch = (HW // 8 if (N % 4 == 0 and HW % 8 == 0) else 0) if sk > 1 else _cdiv(H, 16) * _cdiv(W, 16)
        return dict(route=route, kernel=kernel, epilogue="vector", combine=comb, splitk=sk, nch=nch, tile=(16, 16), kind=5)
    halo = wf != 0 and taps == 9 and W >= 8 and H >= 8 and halo_on
    if colsum and (wf == 0 or not (halo or sk > 1)):
        return dict(refused="column sums are produced by the halo-tile kernel or the split-K combine only")
    if halo:
        sk = min(sk, _cdiv(K, 32))
        wide = W >= 16
        narrow = narrow_on and wide and N <= 32 and not colsum
        mtiles = B * _cdiv(H, 8) * (_cdiv(W, 16) if wide else _cdiv(W, 8))
        aligned = sk > 1 or (out4 and (not colsum or colsum == 1 or v["sx4"]))
        route = "narrow" if narrow else ("halo16" if wide else "halo8")
        np_ = {1: 1, 2: 2, 3: 3, 4: 2}[wf]
        if wf == 4 and gn:
            return dict(refused="the f16x3 image does not take a fused GroupNorm input")
        nt2 = False
        if family == "f16":
            mode = int(env.get("OSM_HALO_NT2", "1"))
            nt2 = (mode > 0 and wide and not narrow and N % 256 == 0 and (mode == 2 or mtiles * (N // 256) * sk >= 512) and aligned)
        if nt2:
            route = "halo_nt2"
        kernel = (f"conv3_halo_bf16s_kernel<{np_},{'true' if gn else 'false'},{16 if wide else 8},3,8,"
                  f"{'true' if narrow else 'false'},{2 if nt2 else 1},{'true' if wf == 4 else 'false'}>")
        epi = "scalar" if narrow else ("vector" if (N % 4 == 0 and aligned) else "scalar")
        comb = _combine(sk, colsum, M, N, HW, out4, sx4=v["sx4"])
        nch = (HW // 8 if (N % 4 == 0 and HW % 8 == 0) else 0) if sk > 1 else _cdiv(H, 8) * (_cdiv(W, 16) if wide else _cdiv(W, 8))
        kind = (4 if narrow_on and N <= 32 else 2) if wide else 3
        return dict(route=route, kernel=kernel, epilogue=epi, combine=comb, splitk=sk, nch=nch, tile=(8, 16 if wide else 8),
                    kind=kind)
    nch = (HW // 8 if (N % 4 == 0 and HW % 8 == 0) else 0) if (sk > 1 and wf != 0) else 0
    if wf != 0:
        if wf == 4:
            if taps != 1:
                return dict(refused="the direct f16x3 image (wfmt 4 without OSM_WFMT_WINOGRAD): 3x3 layers need H, W >= 8")
            if HW % 128 != 0:
                return dict(refused="the direct f16x3 kernel needs H * W to be a multiple of 128")
            kernel, route = "igemm_bf16s_kernel<1,2,true>", "tap1_hp"
        else:
            kernel, route = f"igemm_bf16s_kernel<{taps},{wf}>", "tap9" if taps == 9 else "tap1"
        epi = "vector" if (N % 4 == 0 and (sk > 1 or out4)) else "scalar"
        return dict(route=route, kernel=kernel, epilogue=epi, combine=_combine(sk, colsum, M, N, HW, out4, sx4=v["sx4"]), splitk=sk,
                    nch=nch, tile=None, kind=1)
    kernel = "igemm_f32_kernel<9,false>" if taps == 9 else f"igemm_f32_kernel<1,false{',true' if N <= 64 else ''}>"
    return dict(route="f32", kernel=kernel, epilogue="scalar", combine=_combine(sk, 0, M, N, HW, out4), splitk=sk, nch=0,
                tile=None, kind=0)


def reaches_gemm(M, N, K, b_kn, nbatch=1, splitk=1, c4=True):
    """osm_gemm through the same launch(): the exact-fp32 kernel instance and the combine.  c4: N, ldc, ldr, the batch strides of
    C multiples of 4 and C / res 16-byte aligned."""
    sk = max(1, min(splitk, _cdiv(K, 32)))
    kernel = f"igemm_f32_kernel<1,{'true' if b_kn else 'false'}{',true' if N <= 64 else ''}>"
    return dict(kernel=kernel, combine=_combine(sk, 0, M, N, M, c4 and N % 4 == 0, nbatch), splitk=sk)


# ------------------------------------------------------------------------------------------------ specs of the GPU file
Spec = namedtuple("Spec", "B H W Cin Cout k arith wino splitk epi view gn stat values dgrad",
                  defaults=(False, 1, "both", "dense", False, 0, "randn", False))


def spec_id(s):
    return (f"{s.B}x{s.H}x{s.W}-{s.Cin}to{s.Cout}-k{s.k}-{s.arith}{'-wino' if s.wino else ''}-sk{s.splitk}-{s.epi}-{s.view}"
            f"{'-gn' if s.gn else ''}{f'-stat{s.stat}' if s.stat else ''}-{s.values}{'-dgrad' if s.dgrad else ''}")


def spec_wfmt(s):
    return WFMT[s.arith] | (WINOGRAD if s.wino else 0)


def spec_views(s):
    """window layout of a spec: (x c0, x ld extra), (y c0, ldy extra), (res c0, ldr extra), (stat_x c0, ld extra), and the
    alignment facts reaches() wants.  "win": the misaligned windows of the decoder's concat (odd c0, ldy = Cout + 7);
    "awin": the aligned ones (c0 = 32, ld % 4 == 0) for the routes that need vectors; "swin": those with a misaligned stat_x."""
    N = s.Cin if s.dgrad else s.Cout
    if s.view == "dense":
        return SimpleNamespace(x=(0, 0), y=(0, 0), r=(0, 0), sx=(0, -N % 4), facts=dict(y4=N % 4 == 0, r4=N % 4 == 0, sx4=True))
    xw = (4 if (s.Cin + s.Cout) % 8 else 36, 44)
    if s.view == "win":
        return SimpleNamespace(x=xw, y=(3, 7), r=(5, 12), sx=(4, 8), facts=dict(y4=False, r4=False, sx4=True))
    assert N % 4 == 0
    if s.view == "swin":        # aligned y / res, a misaligned stat_x: the halo epilogue's scalar fallback, refused by Winograd
        return SimpleNamespace(x=xw, y=(32, 64), r=(8, 12), sx=(1, 4), facts=dict(y4=True, r4=True, sx4=False))
    return SimpleNamespace(x=xw, y=(32, 64), r=(8, 12), sx=(32, 36), facts=dict(y4=True, r4=True, sx4=True))


def spec_reaches(s, env=None):
    K, N = (s.Cout, s.Cin) if s.dgrad else (s.Cin, s.Cout)
    f = dict(spec_views(s).facts)
    if EPILOGUES[s.epi][1] == 0:
        f["r4"] = True
    return reaches(s.B, s.H, s.W, K, N, s.k, spec_wfmt(s), s.splitk, f, s.gn, s.stat, "f16" if s.arith == "f16" else "f32", env)


def _both(*a, **kw):
    """a spec forward and as the data gradient (same layer: the gradient's output has Cin columns)"""
    s = Spec(*a, **kw)
    return [s, s._replace(dgrad=True)] if s.Cout % 4 == 0 else [s]      # (the gradient's input has Cout channels: multiples of 4)


def _specs():
    S, L = Spec, []
    # ---- igemm_f32_kernel<9>, <1>, <1,.,true>: wfmt 0
    L += _both(2, 5, 7, 4, 3, 3, "f32", view="win") + _both(2, 4, 4, 36, 8, 1, "f32", epi="bias")
    L += _both(2, 12, 20, 96, 70, 3, "f32", epi="res") + _both(2, 12, 20, 36, 64, 1, "f32", epi="acc", view="win")
    L += [S(2, 5, 7, 36, 70, 1, "f32", epi="none"), S(2, 4, 4, 96, 64, 3, "f32", splitk=4, epi="all", view="win"),
          S(2, 4, 4, 96, 64, 3, "f32", splitk=4, epi="all", view="awin"), S(2, 4, 4, 96, 8, 3, "f32", splitk=9, epi="all")]
    L += _both(2, 5, 7, 4, 8, 3, "f32", values="ints", epi="all") + [S(2, 4, 4, 96, 64, 1, "f32", splitk=2, values="ints")]
    for ar in ("bf16x3", "bf16x6", "f16"):
        # ---- igemm_bf16s_kernel<9,NP>: H < 8 or W < 8
        L += _both(2, 4, 4, 36, 72, 3, ar, epi="none") + _both(2, 3, 5, 36, 6, 3, ar, epi="bias", view="win")
        L += [S(2, 7, 20, 128, 72, 3, ar, epi="res", view="win"), S(2, 1, 1, 36, 72, 3, ar, epi="acc"),
              S(2, 4, 4, 36, 72, 3, ar, splitk=4, epi="all"),                       # 18 chunks over 4: 5, 5, 5, 3
              S(2, 4, 4, 36, 72, 3, ar, splitk=7, epi="all", view="win"),            # 18 over 7: per 3 -> 6 live, the last EMPTY
              S(2, 4, 4, 36, 72, 3, ar, splitk=40, epi="both")]                      # more shares than chunks
        L += _both(2, 3, 5, 36, 72, 3, ar, values="ints", epi="all") + [S(2, 4, 4, 36, 6, 3, ar, splitk=7, values="ints")]
        # ---- igemm_bf16s_kernel<1,NP>
        L += _both(2, 5, 3, 36, 6, 1, ar, epi="bias") + _both(2, 8, 8, 128, 72, 1, ar, epi="res", view="win")
        L += [S(2, 16, 16, 36, 72, 1, ar, epi="acc", view="awin"), S(2, 16, 16, 128, 6, 1, ar, epi="none", view="win"),
              S(2, 8, 8, 128, 72, 1, ar, splitk=2, epi="all"), S(2, 5, 3, 128, 6, 1, ar, splitk=3, epi="all"),   # 4 over 3: 2, 2, EMPTY
              S(2, 8, 8, 128, 72, 1, ar, splitk=3, epi="all", view="win")]
        L += _both(2, 5, 3, 36, 72, 1, ar, values="ints", epi="all") + [S(2, 8, 8, 128, 6, 1, ar, splitk=3, values="ints")]
    for ar in ("bf16x3", "bf16x6", "f16", "f16x3"):
        g = ar != "f16x3"
        # ---- halo 8 x 16
        L += _both(2, 8, 16, 40, 36, 3, ar, epi="none") + _both(2, 9, 17, 4, 70, 3, ar, epi="bias")
        L += _both(2, 9, 17, 40, 36, 3, ar, epi="res", view="win") + _both(2, 24, 40, 160, 96, 3, ar, epi="acc", view="awin")
        L += [S(2, 9, 17, 40, 70, 3, ar, epi="all", view="win"), S(2, 9, 17, 40, 36, 3, ar, epi="both", gn=g, view="awin"),
              S(2, 9, 17, 160, 36, 3, ar, splitk=4, epi="all", view="win"),        # 5 slabs over 4: 2, 2, 1, EMPTY -> <1> by ldy
              S(2, 9, 17, 160, 70, 3, ar, splitk=2, epi="all"),                     # 3, 2 -> <1> by Cout % 4
              S(2, 9, 17, 160, 36, 3, ar, splitk=5, epi="all", view="awin"),       # equal shares -> <4>
              S(2, 8, 16, 160, 36, 3, ar, splitk=9, epi="acc")]                     # more shares than slabs
        L += _both(2, 9, 17, 40, 36, 3, ar, values="ints", epi="all") + [S(2, 9, 17, 160, 70, 3, ar, splitk=4, values="ints"),
                                                                          S(2, 9, 17, 160, 36, 3, ar, splitk=4, values="ints")]
        # ---- halo 8 x 8
        L += _both(2, 8, 8, 40, 36, 3, ar, epi="bias") + _both(2, 10, 9, 40, 70, 3, ar, epi="res", view="win")
        L += [S(2, 9, 15, 160, 96, 3, ar, epi="acc", view="awin"), S(2, 10, 9, 40, 36, 3, ar, epi="none", gn=g),
              S(2, 8, 8, 288, 36, 3, ar, splitk=9, epi="all"),                      # deep: 9 equal shares, 8 x 8
              S(2, 8, 8, 288, 36, 3, ar, splitk=8, epi="all", view="awin"),        # deep: 9 slabs over 8 -> per 2: 2 x 4, 1, 3 EMPTY
              S(2, 10, 9, 160, 36, 3, ar, splitk=4, epi="all", view="win")]
        L += _both(2, 10, 9, 40, 36, 3, ar, values="ints", epi="all") + [S(2, 8, 8, 288, 36, 3, ar, splitk=8, values="ints")]
        # ---- narrow (Cout <= 32, W >= 16)
        L += [S(2, 9, 17, 40, 3, 3, ar, epi="bias", view="win"), S(2, 9, 17, 40, 4, 3, ar, epi="res"),
              S(2, 16, 32, 40, 6, 3, ar, epi="none", gn=g), S(2, 16, 32, 40, 8, 3, ar, epi="acc", view="awin"),
              S(2, 9, 17, 160, 32, 3, ar, epi="both", view="win"), S(2, 9, 17, 160, 32, 3, ar, splitk=4, epi="all"),
              S(2, 9, 17, 160, 6, 3, ar, splitk=2, epi="all", view="win"), S(2, 9, 17, 4, 40, 3, ar, epi="all", dgrad=True),
              S(2, 9, 17, 40, 6, 3, ar, values="ints", epi="all"), S(2, 9, 17, 160, 8, 3, ar, splitk=4, values="ints"),
              S(2, 9, 17, 8, 40, 3, ar, values="ints", epi="all", dgrad=True)]
        # ---- column sums: halo epilogue (vector and scalar form), stats combine for halo / H < 8 / 1x1; wfmt 3, 4, f16
        if ar != "bf16x3":
            for mode in (1, 2):
                L += [S(2, 9, 17, 40, 36, 3, ar, stat=mode, epi="both", view="awin"), S(2, 10, 9, 40, 70, 3, ar, stat=mode, epi="bias"),
                      S(2, 9, 17, 40, 36, 3, ar, stat=mode, epi="res", view="win"), S(2, 9, 17, 40, 36, 3, ar, stat=mode, epi="all", view="swin"),
                      S(2, 8, 16, 160, 36, 3, ar, stat=mode, splitk=4, epi="all", view="awin"),
                      ] + ([] if ar == "f16x3" else [S(2, 8, 8, 160, 72, 1, ar, stat=mode, splitk=3, epi="all")]) + (
                      [S(2, 16, 16, 512, 160, 1, ar, stat=mode, splitk=4, epi="both")] if ar == "f16x3" else
                      [S(2, 4, 4, 36, 72, 3, ar, stat=mode, splitk=4, epi="all", view="awin")])
    # ---- igemm_bf16s_kernel<1,2,true>: 1x1 f16x3, HW % 128 == 0
    L += _both(2, 8, 16, 40, 36, 1, "f16x3", epi="bias") + _both(2, 16, 16, 512, 160, 1, "f16x3", epi="res", view="awin")
    L += [S(2, 8, 16, 40, 36, 1, "f16x3", epi="acc", view="win"), S(2, 8, 16, 40, 160, 1, "f16x3", epi="none"),
          S(2, 8, 16, 512, 36, 1, "f16x3", splitk=5, epi="all"),                    # 16 over 5: per 4 -> 4 live, the last EMPTY
          S(2, 8, 16, 512, 36, 1, "f16x3", splitk=3, epi="all", view="win"), S(2, 8, 16, 40, 36, 1, "f16x3", values="scales", epi="res"),
          S(2, 8, 16, 512, 160, 1, "f16x3", values="scales", epi="none", splitk=2, dgrad=True)]
    L += _both(2, 8, 16, 40, 36, 1, "f16x3", values="ints", epi="all") + [S(2, 8, 16, 512, 36, 1, "f16x3", splitk=5, values="ints")]
    # ---- "scales" on the other wfmt 4 routes
    L += [S(2, 9, 17, 40, 36, 3, "f16x3", values="scales", epi="res"), S(2, 10, 9, 40, 36, 3, "f16x3", values="scales", epi="none", dgrad=True),
          S(2, 9, 17, 40, 8, 3, "f16x3", values="scales", epi="res"), S(2, 17, 19, 40, 64, 3, "f16x3", wino=True, values="scales", epi="res"),
          S(2, 16, 16, 64, 64, 3, "f16x3", wino=True, values="scales", epi="none", dgrad=True)]
    # ---- halo NT = 2 (fp16 family, OSM_HALO_NT2=2 by monkeypatch)
    L += [S(2, 9, 17, 40, 256, 3, "f16", epi="both", view="awin"), S(2, 9, 17, 40, 256, 3, "f16", epi="acc", view="win"),   # falls back to one tile
          S(2, 9, 17, 160, 256, 3, "f16", splitk=4, epi="all"), S(2, 9, 17, 40, 256, 3, "f16", stat=1, epi="both"),
          S(2, 9, 17, 40, 256, 3, "f16", values="ints", epi="all"), S(2, 9, 17, 40, 256, 3, "f16", epi="none", gn=True),
          S(2, 9, 17, 160, 256, 3, "f16", splitk=4, values="ints"), S(2, 9, 17, 256, 40, 3, "f16", epi="both", view="awin", dgrad=True),
          S(2, 9, 17, 256, 40, 3, "f16", values="ints", epi="all", dgrad=True)]
    # ---- Winograd
    for ar in ("f16", "bf16x3", "bf16x6"):
        L += [S(2, 16, 16, 16, 64, 3, ar, wino=True, epi="none"), S(2, 17, 19, 96, 64, 3, ar, wino=True, epi="res", dgrad=True, view="awin"),
              S(2, 17, 19, 20, 96, 3, ar, wino=True, epi="bias", view="awin"),
              S(2, 18, 30, 40, 320, 3, ar, wino=True, epi="res"), S(2, 17, 19, 272, 64, 3, ar, wino=True, epi="acc", view="awin"),
              S(2, 17, 19, 40, 96, 3, ar, wino=True, epi="both", gn=True, view="awin"),
              S(2, 17, 19, 160, 64, 3, ar, wino=True, splitk=6, epi="all", view="awin"),      # 10 slabs over 6: 2 x 5, EMPTY
              S(2, 16, 16, 272, 64, 3, ar, wino=True, splitk=4, epi="all"),                    # 18 over 4: 5, 5, 5, 3
              S(2, 16, 16, 40, 64, 3, ar, wino=True, splitk=9, epi="both"),                    # more shares than slabs
              S(2, 17, 19, 40, 96, 3, ar, wino=True, values="ints", epi="all", view="awin"),
              S(2, 16, 16, 64, 64, 3, ar, wino=True, values="ints", dgrad=True),
              S(2, 17, 19, 160, 64, 3, ar, wino=True, splitk=6, values="ints")]
    for ar in ("bf16x6", "f16"):
        for mode in (1, 2):
            L += [S(2, 17, 19, 40, 96, 3, ar, wino=True, stat=mode, epi="both", view="awin"),
                  S(2, 16, 16, 160, 64, 3, ar, wino=True, stat=mode, splitk=6, epi="all")]
    hp = dict(wino=True)
    L += _both(2, 16, 16, 64, 64, 3, "f16x3", epi="bias", **hp) + [                            # pipelined: 4 slabs
          S(2, 17, 19, 144, 96, 3, "f16x3", epi="res", view="awin", **hp), S(2, 17, 19, 272, 64, 3, "f16x3", splitk=2, epi="all", **hp),
          S(2, 18, 30, 64, 320, 3, "f16x3", epi="acc", view="awin", **hp), S(2, 17, 19, 144, 64, 3, "f16x3", epi="none", **hp),
          S(2, 17, 19, 144, 96, 3, "f16x3", values="ints", epi="all", view="awin", **hp),
          S(2, 16, 16, 272, 64, 3, "f16x3", splitk=2, values="ints", **hp),
          S(2, 16, 16, 64, 64, 3, "f16x3", values="ints", epi="all", dgrad=True, **hp)]
    L += [S(2, 16, 16, 16, 64, 3, "f16x3", epi="bias", **hp), S(2, 17, 19, 96, 72, 3, "f16x3", epi="res", dgrad=True, **hp),   # unpipelined
          S(2, 17, 19, 40, 96, 3, "f16x3", epi="res", view="awin", **hp), S(2, 17, 19, 72, 64, 3, "f16x3", epi="acc", **hp),
          S(2, 17, 19, 64, 64, 3, "f16x3", splitk=4, epi="all", view="awin", **hp),
          S(2, 17, 19, 160, 64, 3, "f16x3", splitk=6, epi="all", **hp),                        # 10 slabs over 6: the last share EMPTY
          S(2, 18, 30, 40, 320, 3, "f16x3", epi="none", **hp),
          S(2, 17, 19, 40, 96, 3, "f16x3", values="ints", epi="all", view="awin", **hp),
          S(2, 17, 19, 64, 64, 3, "f16x3", splitk=4, values="ints", **hp),
          S(2, 17, 19, 96, 72, 3, "f16x3", values="ints", epi="all", dgrad=True, **hp)]
    for mode in (1, 2):
        L += [S(2, 17, 19, 64, 96, 3, "f16x3", stat=mode, epi="both", view="awin", **hp),     # pipelined epilogue
              S(2, 17, 19, 40, 96, 3, "f16x3", stat=mode, epi="bias", **hp),                   # unpipelined epilogue
              S(2, 16, 16, 160, 64, 3, "f16x3", stat=mode, splitk=6, epi="all", **hp)]
    seen, out = set(), []
    for s in L:
        if s not in seen:
            seen.add(s)
            out.append(s)
    return out


SPECS = _specs()
NT2_SPECS = [s for s in SPECS if s.arith == "f16" and (s.Cin if s.dgrad else s.Cout) == 256 and not s.wino]
# what the process-wide switches re-route (tests/conv_env_worker.py)
HALO0_SPECS = [s for s in SPECS if s.k == 3 and not s.wino and not s.gn and s.arith in ("bf16x3", "bf16x6", "f16") and s.H >= 8
               and s.W >= 8 and 256 not in (s.Cin, s.Cout) and s.values != "scales"
               and (s.stat == 0 or s.splitk > 1)]
NARROW0_SPECS = [s for s in SPECS if s.k == 3 and not s.wino and s.W >= 16 and s.H >= 8 and (s.Cin if s.dgrad else s.Cout) <= 32
                 and s.arith != "f32"]

GemmSpec = namedtuple("GemmSpec", "M N K b_kn nb alpha epi ldc_extra splitk values", defaults=((1, 1), 1.0, "none", 0, 1, "randn"))


def _gemm_specs():
    G, L = GemmSpec, []
    for b_kn in (0, 1):
        L += [G(70, 36, 52, b_kn, epi="bias"), G(128, 64, 200, b_kn, epi="res", alpha=0.5), G(70, 160, 200, b_kn, (2, 2), 0.25, "both"),
              G(128, 36, 52, b_kn, (2, 2), -2.0, "acc", 3), G(70, 64, 200, b_kn, epi="all", ldc_extra=3),
              G(70, 160, 200, b_kn, (2, 2), 0.5, "all", 0, 3),                      # combine <4>
              G(128, 36, 200, b_kn, (2, 1), 2.0, "all", 3, 7),                      # combine <1> by ldc; 7 chunks over 7
              G(70, 64, 200, b_kn, epi="all", splitk=4),                            # 7 over 4: 2, 2, 2, 1
              G(70, 160, 260, b_kn, alpha=0.5, epi="all", splitk=9),               # deep needs >= 8 chunks: K = 260 -> 9 (batch 1)
              G(128, 64, 260, b_kn, epi="acc", splitk=8),                           # deep, 9 over 8: per 2 -> 5 live shares, 3 EMPTY
              G(70, 36, 52, b_kn, (2, 2), 2.0, "all", 3, values="ints"), G(128, 160, 200, b_kn, alpha=0.5, epi="all", splitk=3, values="ints"),
              G(70, 64, 260, b_kn, alpha=2.0, epi="all", splitk=8, values="ints")]
    L += [G(70, 70, 52, 0, epi="both"), G(128, 70, 200, 0, (2, 2), 0.5, "all", 3), G(70, 70, 200, 0, epi="all", splitk=5),    # <1> by N
          G(128, 70, 52, 0, alpha=2.0, epi="all", values="ints")]
    return L


GEMM_SPECS = _gemm_specs()


@functools.lru_cache(maxsize=None)
def gemm_case(M, N, K, b_kn, nb, values):
    g = torch.Generator().manual_seed(M + 3 * N + 7 * K + 11 * b_kn + 13 * nb[0] + 17 * nb[1] + (values == "ints"))
    nbt = nb[0] * nb[1]
    if values == "ints":
        A, Bm = _ints(g, (nbt, M, K), -4, 4), _ints(g, (nbt, N, K), -2, 2, 4)
        bias, res, prior = _ints(g, (N,), -8, 8), _ints(g, (nbt, M, N), -8, 8), _ints(g, (nbt, M, N), -8, 8)
    else:
        A, Bm = torch.randn(nbt, M, K, generator=g), torch.randn(nbt, N, K, generator=g) / math.sqrt(K)
        bias, res, prior = torch.randn(N, generator=g), torch.randn(nbt, M, N, generator=g), torch.randn(nbt, M, N, generator=g)
    prod = torch.einsum("zmk,znk->zmn", A.to(F64), Bm.to(F64))
    return SimpleNamespace(A=A, Bm=Bm, bias=bias, res=res, prior=prior, prod=prod)


def gemm_ref(c, alpha, epi):
    hb, hr, ha = EPILOGUES[epi]
    y = c.prod * alpha
    if hb:
        y = y + c.bias.to(F64)
    if hr:
        y = y + c.res.to(F64)
    if ha:
        y = y + c.prior.to(F64)
    return y


# ------------------------------------------------------------------------------------------------ checkers
def edge_mask(B, H, W, tile):
    """[B][H][W] bool: the pixels of the ragged last tiles (halo / Winograd patches of `tile` pixels per image, or -- tile None
    -- the last partial 128-row tile of the flattened pixel rows)"""
    m = torch.zeros(B, H, W, dtype=torch.bool)
    if tile is None:
        M = B * H * W
        m.view(-1)[128 * (M // 128):] = True
    else:
        th, tw = tile
        m[:, th * (H // th):, :] = True
        m[:, :, tw * (W // tw):] = True
    return m


def check_out(got, ref, B, H, W, tol, tile, tag, exact=False):
    """misses of got [B][C][H][W] (fp64) against ref: per image against its own max |ref|, then interior and ragged-edge pixels
    of each image against the max |ref| of their own; exact: bit equality with the reference instead"""
    misses = []
    if not torch.isfinite(got).all():
        return [(tag, "y has NaN / inf left", int((~torch.isfinite(got)).sum()))]
    if exact:
        if not torch.equal(got, ref):
            misses.append((tag, "not bit-equal to the integer reference", float((got - ref).abs().max()), int((got != ref).sum())))
        return misses
    em = edge_mask(B, H, W, tile)
    for b in range(B):
        regions = [("image", torch.ones(H, W, dtype=torch.bool))]
        if em[b].any() and not em[b].all():
            regions += [("interior", ~em[b]), ("edge", em[b])]
        for name, msk in regions:
            r, gq = ref[b][:, msk], got[b][:, msk]
            e = float((gq - r).abs().max() / r.abs().max().clamp_min(1e-300))
            print(f"{tag} image {b} {name}: err {e:.3e} (bar {tol:.3e})")
            if not e <= tol:
                misses.append((tag, f"image {b} {name}", e, tol))
    return misses


def check_colsum(cs, y_rows, B, HW, N, nch, mode, stat_x, table, silu, tag):
    """cs: the kernel's [B][nch][2][N] (any float tensor, CPU); y_rows: the y it wrote, [B HW][N].  Relative, per image and sum,
    against fp64 sums of that y."""
    if not torch.isfinite(cs).all():
        return [(tag, "colsum slots left NaN / inf", int((~torch.isfinite(cs)).sum()))]
    got = cs.to(F64).reshape(B, nch, 2, N).sum(1)
    ref = colsum_ref(y_rows.to(F64).reshape(B, HW, N), mode, None if stat_x is None else stat_x.reshape(B, HW, N), table, silu)
    misses = []
    for b in range(B):
        for j in range(2):
            e = float((got[b, j] - ref[b, j]).abs().max() / ref[b, j].abs().max().clamp_min(1e-300))
            print(f"{tag} image {b} colsum[{j}] mode {mode}: err {e:.3e} (bar {COLSUM_BAR[mode]:.1e})")
            if not e <= COLSUM_BAR[mode]:
                misses.append((tag, f"image {b} colsum[{j}] mode {mode}", e, COLSUM_BAR[mode]))
    return misses


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------------------------------------ runners (ops is passed in)
def _nan_window(data, c0, extra, dtype, dev, guard=4):
    """data [rows][C] as columns c0 : c0 + C of a NaN-filled [rows + 2 guard][C + extra] buffer (the header promises "Cin
    channels used": nothing outside the window may reach the result)"""
    R, C = data.shape
    buf = torch.full((R + 2 * guard, C + extra), NAN, dtype=dtype, device=dev)
    view = buf[guard:guard + R, c0:c0 + C]
    view.copy_(data.to(dtype))
    return view


def run_conv(ops, s, dev="cuda:0", env=None):
    """Run one Spec through ops.conv2d on guarded windows.  Returns dict(y [B][C][H][W] fp64, y_bits, cs, ws_bits, misses) or
    dict(refused=<message>).  misses: guards, NaN left in ws; the numeric checks are check_spec()."""
    c = case(s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.values, s.arith == "f16")
    half = s.arith == "f16"
    dt = torch.float16 if half else torch.float32
    xin, bias, res, prior, _ = operands(c, s.dgrad)
    K, N = (s.Cout, s.Cin) if s.dgrad else (s.Cin, s.Cout)
    B, H, W, M = s.B, s.H, s.W, s.B * s.H * s.W
    hb, hr, ha = EPILOGUES[s.epi]
    v = spec_views(s)
    wfmt = spec_wfmt(s)
    pack = ops.pack_conv_weight_winograd if s.wino else ops.pack_conv_weight
    wf, wd = pack(c.w.to(dev), want_fwd=not s.dgrad, want_dgrad=s.dgrad, wfmt=WFMT[s.arith])
    xv = _nan_window(rows(xin), v.x[0], v.x[1], dt, dev)
    yg = Guarded(M, N, width=N + v.y[1], c0=v.y[0], dtype=dt, device=dev,
                 data=rows(prior) if ha else torch.full((M, N), NAN))
    rg = Guarded(M, N, width=N + v.r[1], c0=v.r[0], dtype=dt, device=dev, data=rows(res)) if hr else None
    kw = {}
    table = sx = stab = None
    if s.gn:
        table = gn_table(B, K)
        kw.update(gn_table=table.to(dev), gn_silu=True)
    r = spec_reaches(s, env)
    ws = None
    if s.splitk > 1:
        ws = Guarded(s.splitk * M, N, dtype=torch.float32, device=dev, data=torch.full((s.splitk * M, N), NAN))
        kw.update(splitk=s.splitk, splitk_ws=ws.view)
    nch = ops.conv_stat_chunks(B, H, W, K, N, s.k, wfmt, s.splitk, s.gn) if s.stat else 0
    cs = sg = None
    if s.stat:
        cs = Guarded(max(1, B * nch * 2), N, dtype=torch.float32, device=dev, data=torch.full((max(1, B * nch * 2), N), NAN))
        kw.update(colsum=cs.view, stat_mode=s.stat, stat_silu=True)
        if s.stat == 2:
            g = torch.Generator().manual_seed(99 + N)
            sx = (torch.randn(M, N, generator=g) * 1.5 + 0.3).to(dt).float()
            stab = gn_table(B, N, seed=5)
            sg = Guarded(M, N, width=N + v.sx[1], c0=v.sx[0], dtype=dt, device=dev, data=sx)
            kw.update(stat_x=ops.Mat.of(sg.view), stat_table=stab.to(dev))
    xm = ops.Mat.of(xv)
    if s.arith == "f16x3":
        parts = torch.full((B * ops.MAXABS_PARTS,), NAN, device=dev)
        ops.maxabs(xm, B, parts)
        kw.update(x_maxabs=parts)
    try:
        ops.conv2d(xm, wd if s.dgrad else wf, bias.to(dev) if hb else None, ops.Mat.of(yg.view), B, H, W, s.k,
                   res=ops.Mat.of(rg.view) if hr else None, accumulate=bool(ha), wfmt=wfmt, **kw)
    except Exception as e:          # OsmosisHipError: the message is what the tests assert
        return dict(refused=str(e), nch=nch)
    torch.cuda.synchronize()
    misses = []
    tag = spec_id(s)
    for name, gd in (("y", yg), ("res", rg), ("ws", ws), ("colsum", cs), ("stat_x", sg)):
        if gd is not None and not gd.intact():
            misses.append((tag, f"bytes outside the {name} window changed"))
    for name, gd in (("res", rg), ("stat_x", sg)):
        if gd is not None and not torch.equal(gd.get(), (rows(res) if name == "res" else sx).to(F64)):
            misses.append((tag, f"the {name} operand was written"))
    ws_bits = None
    if ws is not None:
        live = ws.view[:r["splitk"] * M] if "splitk" in r else ws.view
        ws_bits = live.clone()
        if not torch.isfinite(live).all():
            misses.append((tag, "NaN left in the live split-K partials", int((~torch.isfinite(live)).sum())))
    y_rows = yg.view.detach().clone()
    return dict(y=nchw(yg.get(), B, H, W), y_bits=y_rows, y_rows=y_rows.to("cpu", F64), cs=None if cs is None else cs.view.detach().cpu().clone(),
                ws_bits=ws_bits, nch=nch, misses=misses, sx=sx, stab=stab, table=table)


def spec_ref(s):
    """fp64 reference of a Spec's result, [B][C][H][W]"""
    c = case(s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.values, s.arith == "f16")
    xin, bias, res, prior, base = operands(c, s.dgrad)
    if s.gn:
        base = conv64(gn_input(xin, gn_table(s.B, xin.shape[1]), True, s.arith == "f16" and not s.wino), flip_t(c.wref) if s.dgrad else c.wref)
    return epilogue_ref(base, bias, res, prior, s.epi)


def spec_model(s):
    """the arithmetic model of a Spec's result (see model()); the final store is not part of it (store(): at most 2^-24, or
    HALF_ULP of the element in the fp16 family, which the f16 bars contain)"""
    c = case(s.B, s.H, s.W, s.Cin, s.Cout, s.k, s.values, s.arith == "f16")
    xin, bias, res, prior, _ = operands(c, s.dgrad)
    if s.gn:
        xin = gn_input(xin, gn_table(s.B, xin.shape[1]), True, s.arith == "f16" and not s.wino)
    base = model(s.arith, xin, flip_t(c.w) if s.dgrad else c.w, s.wino)
    return epilogue_ref(base, bias, res, prior, s.epi)


def check_spec(s, out, env=None):
    """misses of run_conv()'s result against the reference, the bars and (split-K, column sums) the extra contracts"""
    r = spec_reaches(s, env)
    tag = spec_id(s)
    misses = list(out["misses"])
    ref = spec_ref(s)
    exact = s.values == "ints"
    if exact:
        ref = store(ref, s.arith == "f16")
    misses += check_out(out["y"], ref, s.B, s.H, s.W, bar(s.arith, s.wino, s.gn), r["tile"], tag, exact)
    if s.stat:
        N = s.Cin if s.dgrad else s.Cout
        if out["nch"] != r["nch"] or out["nch"] <= 0:
            misses.append((tag, "osm_conv_stat_chunks", out["nch"], r["nch"]))
        else:
            misses += check_colsum(out["cs"][:s.B * out["nch"] * 2], out["y_rows"], s.B, s.H * s.W, N, out["nch"], s.stat, out["sx"],
                                   out["stab"], True, tag)
    return misses


def run_gemm(ops, s, dev="cuda:0"):
    """one GemmSpec through ops.gemm: a two-level batch with non-dense strides, C (and res) rows ldc = N + ldc_extra inside a
    sentinel-filled buffer.  Returns dict(y [nb][M][N] fp64, bits, misses)."""
    c = gemm_case(s.M, s.N, s.K, s.b_kn, s.nb, s.values)
    M, N, K = s.M, s.N, s.K
    nb1, nb2 = s.nb
    nbt = nb1 * nb2
    hb, hr, ha = EPILOGUES[s.epi]
    lda, ldb = K + 4, (N + 8 if s.b_kn else K + 8)
    brow = K if s.b_kn else N
    sA1, sB1 = M * lda + 8, brow * ldb + 12
    sA2, sB2 = nb1 * sA1 + 16, nb1 * sB1 + 4
    ldc = N + s.ldc_extra
    sC1 = M * ldc + (4 if s.ldc_extra == 0 else 5)
    sC2 = nb1 * sC1 + (8 if s.ldc_extra == 0 else 3)
    A = torch.full((nb2 * sA2 + 64,), NAN, device=dev)
    Bt = torch.full((nb2 * sB2 + 64,), NAN, device=dev)
    Cb = torch.full((nb2 * sC2 + 64,), SENTINEL, device=dev)
    Rb = torch.full((nb2 * sC2 + 64,), SENTINEL, device=dev)
    idx = torch.zeros(nb2 * sC2 + 64, dtype=torch.bool)
    c_off = 4 if s.ldc_extra == 0 else 1
    for z in range(nbt):
        b1, b2 = z % nb1, z // nb1
        a0, b0, c0 = b1 * sA1 + b2 * sA2, b1 * sB1 + b2 * sB2, c_off + b1 * sC1 + b2 * sC2
        A[a0:a0 + M * lda].view(M, lda)[:, :K] = c.A[z].to(dev)
        bm = c.Bm[z].t() if s.b_kn else c.Bm[z]
        Bt[b0:b0 + brow * ldb].view(brow, ldb)[:, :bm.shape[1]] = bm.to(dev)
        cw = Cb[c0:c0 + M * ldc].view(M, ldc)[:, :N]
        cw.copy_((c.prior[z] if ha else torch.full((M, N), NAN)).to(dev))
        Rb[c0:c0 + M * ldc].view(M, ldc)[:, :N] = c.res[z].to(dev)
        idx[c0:c0 + M * ldc].view(M, ldc)[:, :N] = True
    before = Cb.clone()
    ws = None
    if s.splitk > 1:
        ws = Guarded(s.splitk * nbt * M, N, device=dev, data=torch.full((s.splitk * nbt * M, N), NAN))
    ops.gemm(A, lda, Bt, ldb, Cb, ldc, M, N, K, b_kn=bool(s.b_kn), alpha=s.alpha, nb1=nb1, nb2=nb2, sA=(sA1, sA2), sB=(sB1, sB2),
             sC=(sC1, sC2), bias=c.bias.to(dev) if hb else None, res=Rb if hr else None, ldr=ldc if hr else 0, accumulate=bool(ha),
             c_off=c_off, splitk=s.splitk, splitk_ws=ws.view if ws is not None else None)
    torch.cuda.synchronize()
    misses = []
    out = Cb.cpu()
    if not torch.equal(out[~idx].view(torch.int32), before.cpu()[~idx].view(torch.int32)):
        misses.append((s, "bytes outside C changed"))
    if ws is not None:
        r = reaches_gemm(M, N, K, s.b_kn, nbt, s.splitk, s.ldc_extra == 0)
        if not ws.intact():
            misses.append((s, "bytes outside the workspace changed"))
        if not torch.isfinite(ws.view[:r["splitk"] * nbt * M]).all():
            misses.append((s, "NaN left in the live split-K partials"))
    y = torch.stack([out[c_off + (z % nb1) * sC1 + (z // nb1) * sC2:][:M * ldc].view(M, ldc)[:, :N] for z in range(nbt)])
    return dict(y=y.to(F64), bits=out, misses=misses)


def check_gemm(s, out):
    c = gemm_case(s.M, s.N, s.K, s.b_kn, s.nb, s.values)
    ref = gemm_ref(c, s.alpha, s.epi)
    misses = list(out["misses"])
    y = out["y"]
    if not torch.isfinite(y).all():
        return misses + [(s, "C has NaN / inf left")]
    if s.values == "ints":
        if not torch.equal(y, ref.float().to(F64)):
            misses.append((s, "not bit-equal to the integer reference", float((y - ref).abs().max())))
        return misses
    for z in range(y.shape[0]):
        e = float((y[z] - ref[z]).abs().max() / ref[z].abs().max())
        print(f"{s} batch {z}: err {e:.3e} (bar {GEMM_BAR:.1e})")
        if not e <= GEMM_BAR:
            misses.append((s, f"batch {z}", e, GEMM_BAR))
    return misses
