"""Reference of the attention core on NHWC-style `qkv` matrices, seeded operands, the error metric and guarded views for
tests/test_attention_gpu.py (a helper, not a test).

    logits = scale * q k^T          per (image, head): q, k, v = `ch` columns at offs[c] + head * hs of a [B][T][width] matrix
    out    = softmax(logits) v      head h at columns h * ch of [B][T][heads * ch]
    lse    = logsumexp(logits)      [B][heads][T]
    delta  = sum_c dO * O           [B][heads][T], over the head's ch columns
    dqkv   = d(sum(out * dO)) / d(qkv), by autograd; columns that belong to no head stay 0

`reference` evaluates all of it in ONE dtype: float64 is the yardstick, float32 measures what the formula alone loses in
single precision (`e32`, the floor under the run-time bars of the stress operands).  oracle.unet_ref.attention_block is not used
for this: it soft-maxes through .float(), so it is no fp64 reference even on double inputs.
tests/test_attn_reference_cpu.py checks this file against a direct autograd statement and against that oracle in fp32."""
import math
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from gn_reference import SENTINEL, Guarded

F64 = torch.float64
GENERATORS = ("randn", "peaked", "ramp_up", "ramp_down", "offset")
STRESS = GENERATORS[1:]

# the project's bars against fp64 on randn operands (tests/test_ops_gpu.py::test_attn_flash_fwd_bwd): out and dqkv of the block's
# max-abs, lse absolute.  delta is checked relative to its own max-abs with the `out` bar.
BARS = {"bf16x6": dict(out=5e-6, dqkv=1e-5, lse=1e-5), "f16x3": dict(out=5e-6, dqkv=1e-5, lse=1e-5),
        "half": dict(out=2e-3, dqkv=4e-3, lse=2e-2)}
E32_FACTOR = 8.0     # stress operands: bar = max(project bar, 8 * e32), see tests/test_attention_gpu.py
ARITH_KW = {"bf16x6": {}, "f16x3": dict(f16x3=True), "half": dict(half=True)}


# ------------------------------------------------------------------------------------------------ head layouts
def layout(kind, heads, ch):
    """(offs, hs, width): column of q | k | v of head 0, head stride, width of the qkv matrix"""
    C = heads * ch
    if kind == "legacy":        # per head [q | k | v]
        return (0, ch, 2 * ch), 3 * ch, 3 * C
    if kind == "new":           # [q of every head | k ... | v ...]
        return (0, C, 2 * C), ch, 3 * C
    if kind == "rev":           # synthetic 1: the new order with v first
        return (2 * C, C, 0), ch, 3 * C
    if kind == "padded":        # synthetic 2: the legacy order with gaps of 8, 4 and 4 columns that belong to no head
        hs = 3 * ch + 16
        return (0, ch + 8, 2 * ch + 12), hs, heads * hs
    raise ValueError(kind)


def head_cols(offs, hs, ch, comp, h):
    return slice(offs[comp] + h * hs, offs[comp] + h * hs + ch)


# ------------------------------------------------------------------------------------------------ the reference
def core(x, heads, ch, offs, hs, scale):
    """differentiable (out [B][T][heads * ch], lse [B][heads][T]) of a [B][T][width] matrix, in x's dtype"""
    outs, lses = [], []
    for h in range(heads):
        q, k, v = (x[:, :, head_cols(offs, hs, ch, c, h)] for c in range(3))
        logits = torch.einsum("btc,bsc->bts", q, k) * scale
        lses.append(torch.logsumexp(logits, dim=-1))
        outs.append(torch.einsum("bts,bsc->btc", torch.softmax(logits, dim=-1), v))
    return torch.cat(outs, dim=-1), torch.stack(lses, dim=1)


def reference(qkv, dout, heads, ch, offs, hs, scale, dtype=F64):
    """(out, lse, delta, dqkv) evaluated in `dtype`, as CPU tensors of that dtype"""
    B, T, _ = qkv.shape
    x = qkv.detach().to("cpu", dtype).requires_grad_(True)
    g = dout.detach().to("cpu", dtype)
    out, lse = core(x, heads, ch, offs, hs, scale)
    (dqkv,) = torch.autograd.grad(out, x, g)
    out = out.detach()
    delta = (g * out).reshape(B, T, heads, ch).sum(dim=-1).permute(0, 2, 1).contiguous()
    return out, lse.detach(), delta, dqkv


# ------------------------------------------------------------------------------------------------ operands
def make_qkv(gen, B, T, heads, ch, offs, hs, width, seed=0):
    """fp32 [B][T][width].  Every generator starts from the existing test's 1.2 * randn (gap columns of a padded layout included)."""
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + 31 * heads + B + 101 * GENERATORS.index(gen))
    x = torch.randn(B, T, width, generator=g) * 1.2
    ramp = torch.linspace(0.2, 3.0, T).reshape(1, T, 1)
    for h in range(heads):
        cq, ck = head_cols(offs, hs, ch, 0, h), head_cols(offs, hs, ch, 1, h)
        if gen == "peaked":          # logit maxima near 40: the softmax saturates
            x[:, :, cq] *= 3.0
            x[:, :, ck] *= 3.0
        elif gen == "ramp_up":       # |k| grows along the sequence: the running maximum rises tile after tile
            x[:, :, ck] *= ramp
        elif gen == "ramp_down":
            x[:, :, ck] *= ramp.flip(1)
        elif gen == "offset":        # a common offset of 1.5 * 1.5 * ch * scale on every logit: shift invariance and lse
            x[:, :, cq] += 1.5
            x[:, :, ck] += 1.5
        elif gen != "randn":
            raise ValueError(gen)
    return x


def make_dout(B, T, C, seed=0):
    g = torch.Generator().manual_seed(1000003 * seed + 7919 * T + C + B + 5)
    return torch.randn(B, T, C, generator=g)


def vdo_ramp(qkv, dout, heads, ch, offs, hs):
    """the existing f16x3 test's million-fold ramps: v rows times logspace(-3, 3), dO rows times logspace(2, -4)"""
    T = qkv.shape[1]
    q2 = qkv.clone()
    for h in range(heads):
        q2[:, :, head_cols(offs, hs, ch, 2, h)] *= torch.logspace(-3, 3, T).reshape(1, T, 1)
    return q2, dout * torch.logspace(2, -4, T).reshape(1, T, 1)


# ------------------------------------------------------------------------------------------------ the metric
def block_err(got, ref, heads, ch, ncomp, offs=None, hs=None):
    """max over (image, head, component) of max |got - ref| / max |ref| of that [T][ch] block.  ncomp = 1: out-like matrices
    (head h at columns h * ch); ncomp = 3: qkv-like ones (offs, hs).  A per-row ratio is not usable: rows with a saturated
    softmax have gradients near zero."""
    if ncomp == 1:
        offs, hs = (0,), ch
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    worst = 0.0
    for c in range(ncomp):
        for h in range(heads):
            sl = head_cols(offs, hs, ch, c, h)
            d = (got[:, :, sl] - ref[:, :, sl]).abs().amax(dim=(1, 2))
            s = ref[:, :, sl].abs().amax(dim=(1, 2))
            if not bool(torch.isfinite(d).all()):
                return float("inf")
            worst = max(worst, float((d / (s + 1e-300)).max()))
    return worst


def max_ratio(got, ref):
    """max |got - ref| / max |ref| of the whole tensor (delta; the metric of tests/test_ops_gpu.py)"""
    got, ref = got.detach().to("cpu", F64), ref.detach().to("cpu", F64)
    d = (got - ref).abs().max()
    return float(d / (ref.abs().max() + 1e-300)) if bool(torch.isfinite(d)) else float("inf")


def abs_err(got, ref):
    d = (got.detach().to("cpu", F64) - ref.detach().to("cpu", F64)).abs().max()
    return float(d) if bool(torch.isfinite(d)) else float("inf")


def errors(got, ref, heads, ch, offs, hs):
    """got, ref: objects with out, lse, delta, dqkv -> dict of the four figures the bars are stated for"""
    return dict(out=block_err(got.out, ref.out, heads, ch, 1), lse=abs_err(got.lse, ref.lse),
                delta=max_ratio(got.delta, ref.delta), dqkv=block_err(got.dqkv, ref.dqkv, heads, ch, 3, offs, hs))


def bars(arith, e32=None):
    """the project bars; with the reference's own fp32 error e32 (a dict as from `errors`): max(project bar, 8 * e32)"""
    b = dict(BARS[arith], delta=BARS[arith]["out"])
    if e32 is not None:
        b = {k: max(v, E32_FACTOR * e32[k]) for k, v in b.items()}
    return b


def case(gen, B, T, heads, ch, kind, seed=0, ramp=False, want_e32=False):
    """operands (fp32 CPU), the fp64 reference of them and, on request, e32"""
    offs, hs, width = layout(kind, heads, ch)
    scale = 1.0 / math.sqrt(ch)
    qkv = make_qkv(gen, B, T, heads, ch, offs, hs, width, seed)
    dout = make_dout(B, T, heads * ch, seed)
    if ramp:
        qkv, dout = vdo_ramp(qkv, dout, heads, ch, offs, hs)
    ref = SimpleNamespace(**dict(zip(("out", "lse", "delta", "dqkv"), reference(qkv, dout, heads, ch, offs, hs, scale, F64))))
    c = SimpleNamespace(gen=gen, B=B, T=T, heads=heads, ch=ch, C=heads * ch, kind=kind, offs=offs, hs=hs, width=width, scale=scale,
                        qkv=qkv, dout=dout, ref=ref, e32=None)
    if want_e32:
        r32 = SimpleNamespace(**dict(zip(("out", "lse", "delta", "dqkv"),
                                         reference(qkv, dout, heads, ch, offs, hs, scale, torch.float32))))
        c.e32 = errors(r32, ref, heads, ch, offs, hs)
    return c


# ------------------------------------------------------------------------------------------------ guarded views
class Views:
    """qkv, out, dout, dqkv and the backward's copy of out as column windows of wider sentinel-filled buffers with pairwise
    different leading dimensions; every window starts at a multiple of 4 floats.  Outputs are prefilled with NaN inside the
    window.  `plain=True`: the same five operands contiguous (ld = width / C), the call the views are compared with."""
    PAD = dict(qkv=(32, 8), dqkv=(64, 12), out=(16, 4), dout=(48, 16), o=(80, 20))      # name -> (extra width, first column)

    def __init__(self, c, device, plain=False):
        rows = c.B * c.T
        self.rows, self.c = rows, c

        def buf(name, cols, data=None):
            extra, c0 = (0, 0) if plain else self.PAD[name]
            g = Guarded(rows, cols, width=cols + extra, c0=c0, device=device, data=data)
            if data is None:
                g.view.fill_(float("nan"))
            return g
        self.qkv = buf("qkv", c.width, c.qkv)
        self.dout = buf("dout", c.C, c.dout)
        self.out = buf("out", c.C)
        self.dqkv = buf("dqkv", c.width)
        self.o = buf("o", c.C)                     # filled from `out` between forward and backward
        self.lse = torch.full((c.B * c.heads * c.T,), float("nan"), device=device)
        self.delta = torch.full((c.B * c.heads * c.T,), float("nan"), device=device)

    def copy_out_for_backward(self):
        self.o.view.copy_(self.out.view)
        self._inputs = [b.buf.clone() for b in (self.qkv, self.dout, self.o)]

    def inputs_unchanged(self):
        return all(torch.equal(a.view(torch.int32), b.buf.view(torch.int32))
                   for a, b in zip(self._inputs, (self.qkv, self.dout, self.o)))

    def outputs_guarded(self):
        """every sentinel element of out and dqkv still has its bytes"""
        return self.out.intact() and self.dqkv.intact()

    def result(self):
        c = self.c
        return SimpleNamespace(out=self.out.get().reshape(c.B, c.T, c.C), dqkv=self.dqkv.get().reshape(c.B, c.T, c.width),
                               lse=self.lse.to("cpu", F64).reshape(c.B, c.heads, c.T),
                               delta=self.delta.to("cpu", F64).reshape(c.B, c.heads, c.T))


def same_bits(a, b):
    """two results of `Views.result` / `run_flash`, bit for bit on what the kernels write (NaN-prefilled gap columns of a padded
    layout compare equal as bytes)"""
    return all(torch.equal(getattr(a, k).view(torch.int64), getattr(b, k).view(torch.int64)) for k in ("out", "lse", "delta", "dqkv"))


def run_flash(ops, c, arith, v=None, device="cuda:0"):
    """osm_attn_flash_fwd then _bwd on the buffers of `v` (default: fresh contiguous ones); returns (result, v)"""
    v = Views(c, device, plain=True) if v is None else v
    M = ops.Mat.of
    kw = ARITH_KW[arith]
    ops.attn_flash_fwd(M(v.qkv.view), M(v.out.view), v.lse, c.B, c.T, c.heads, c.ch, c.offs, c.hs, c.scale, **kw)
    v.copy_out_for_backward()
    ops.attn_flash_bwd(M(v.qkv.view), M(v.o.view), M(v.dout.view), M(v.dqkv.view), v.lse, v.delta, c.B, c.T, c.heads, c.ch,
                       c.offs, c.hs, c.scale, **kw)
    return v.result(), v


def run_small(ops, c, v=None, device="cuda:0"):
    """osm_attn_small_fwd then _bwd (the ws-based backward); lse / delta do not exist there"""
    v = Views(c, device, plain=True) if v is None else v
    M = ops.Mat.of
    ops.attn_small_fwd(M(v.qkv.view), M(v.out.view), c.B, c.T, c.heads, c.ch, c.offs, c.hs, c.scale)
    v.copy_out_for_backward()
    ws = torch.empty(2 * c.B * c.heads * c.T * c.T, device=device)
    ops.attn_small_bwd(M(v.qkv.view), M(v.dout.view), M(v.dqkv.view), ws, c.B, c.T, c.heads, c.ch, c.offs, c.hs, c.scale)
    return v.result(), v


def check_flash(got, c, arith, tag, stress=False):
    """prints every figure (and its ratio to e32 where that is known), then returns the list of misses"""
    e = errors(got, c.ref, c.heads, c.ch, c.offs, c.hs)
    b = bars(arith, c.e32 if stress else None)
    misses = []
    for k in ("out", "lse", "delta", "dqkv"):
        ratio = f"  = {e[k] / c.e32[k]:.2f} x e32 ({c.e32[k]:.2e})" if c.e32 is not None and c.e32[k] > 0 else ""
        print(f"{tag} {arith} {k}: err {e[k]:.2e}  bar {b[k]:.2e}{ratio}")
        if not e[k] <= b[k]:
            misses.append((tag, arith, k, e[k], b[k]))
    return misses


# ------------------------------------------------------------------------------------------------ one AttentionBlock
def block_state_dict(C, seed):
    """seeded AttentionBlock parameters with non-trivial norm weights and a NON-ZERO proj_out (the reference zero-initialises
    it, which would hide the whole core)"""
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g)      # noqa: E731
    return {"norm.weight": 1 + 0.2 * r(C), "norm.bias": 0.1 * r(C),
            "qkv.weight": r(3 * C, C, 1) / math.sqrt(C), "qkv.bias": 0.1 * r(3 * C),
            "proj_out.weight": r(C, C, 1) / math.sqrt(C), "proj_out.bias": 0.1 * r(C)}


def block(sd, x, heads, new_order, dy=None, dtype=F64):
    """GroupNorm32 -> qkv -> `reference` -> proj_out -> + x of an NCHW x, every step in `dtype`; (y, dx) with dx = None without
    dy.  The backward chains the pieces by hand around `reference`'s dqkv."""
    B, C, H, W = x.shape
    T, ch = H * W, C // heads
    offs, hs, _ = layout("new" if new_order else "legacy", heads, ch)
    sd = {k: v.to("cpu", dtype) for k, v in sd.items()}
    xf = x.detach().to("cpu", dtype).reshape(B, C, T).requires_grad_(True)
    xn = F.group_norm(xf, 32, sd["norm.weight"], sd["norm.bias"], eps=1e-5)
    wq, wp = sd["qkv.weight"][:, :, 0], sd["proj_out.weight"][:, :, 0]
    qkv = torch.einsum("bct,oc->bto", xn, wq) + sd["qkv.bias"]                     # [B][T][3C]
    da = torch.zeros(B, T, C, dtype=dtype) if dy is None else torch.einsum("bot,oc->btc", dy.to("cpu", dtype).reshape(B, C, T), wp)
    out, _, _, dqkv = reference(qkv, da, heads, ch, offs, hs, 1.0 / math.sqrt(ch), dtype)
    y = xf.detach() + torch.einsum("btc,oc->bot", out, wp) + sd["proj_out.bias"].reshape(1, C, 1)
    dx = None
    if dy is not None:
        dxn = torch.einsum("bto,oc->bct", dqkv, wq)
        (dx,) = torch.autograd.grad(xn, xf, dxn)
        dx = (dx + dy.to("cpu", dtype).reshape(B, C, T)).reshape(B, C, H, W)
    return y.reshape(B, C, H, W), dx
