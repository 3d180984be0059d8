"""Thin tensor-level wrappers over the C ABI (see include/osmosis_hip.h).

`Mat` is an NHWC "matrix view": rows = pixels (b*H*W), cols = channels, ld = row stride.  Any 2-D
torch view with unit column stride qualifies, so channel slices of a wider buffer (zero-copy
concatenation / split) are first-class.
"""
import ctypes as C
from dataclasses import dataclass
from typing import Optional

import torch

from . import _lib
from ._lib import AttnDesc, ConvDesc, DepthDesc, GainDesc, GemmDesc, GroupDesc, LinDesc, PhysDesc, ReconDesc, RobustDesc, call, current_stream_ptr, ptr, ptr_f64, query


@dataclass
class Mat:
    t: torch.Tensor      # backing 2-D view (kept alive)
    rows: int
    cols: int
    ld: int

    @staticmethod
    def of(t: torch.Tensor) -> "Mat":
        if t.dim() != 2 or (t.shape[1] > 1 and t.stride(1) != 1):
            raise _lib.OsmosisHipError("Mat.of needs a 2-D view with unit column stride")
        return Mat(t, t.shape[0], t.shape[1], t.stride(0) if t.shape[0] > 1 else max(t.stride(0), t.shape[1]))

    @property
    def p(self) -> int:
        return ptr(self.t)

    def cols_slice(self, c0: int, c1: int) -> "Mat":
        return Mat(self.t[:, c0:c1], self.rows, c1 - c0, self.ld)


def _s():
    return current_stream_ptr()


def _fam(t: torch.Tensor) -> str:
    """Entry-point family of an activation tensor: fp32 storage -> osm_*, IEEE-half storage -> osm_*_h."""
    if t.dtype == torch.float16:
        return "_h"
    if t.dtype != torch.float32:
        raise _lib.OsmosisHipError(f"activations must be float32 or float16, got {t.dtype}")
    return ""


def _same_family(*ts):
    fams = {_fam(t) for t in ts if t is not None}
    if len(fams) != 1:
        raise _lib.OsmosisHipError("activation tensors of one call must share a storage type")
    return fams.pop()


def conv2d(x: Mat, w_packed: torch.Tensor, bias: Optional[torch.Tensor], y: Mat, B: int, H: int, W: int,
           ksize: int, res: Optional[Mat] = None, accumulate: bool = False,
           splitk: int = 1, splitk_ws: Optional[torch.Tensor] = None, wfmt: int = 0,
           gn_table: Optional[torch.Tensor] = None, gn_silu: bool = True,
           colsum: Optional[torch.Tensor] = None, stat_mode: int = 0, stat_x: Optional[Mat] = None,
           stat_table: Optional[torch.Tensor] = None, stat_silu: bool = True, x_maxabs: Optional[torch.Tensor] = None):
    """colsum (+ stat_*): optional per-column sums of the result for the GroupNorm that follows (stat_mode 1) or whose
    backward consumes the result (stat_mode 2: stat_x = that GroupNorm's input, stat_table = its per-channel table)."""
    d = ConvDesc()
    d.x, d.w, d.bias = x.p, ptr(w_packed), ptr(bias)
    d.res = res.p if res is not None else None
    d.y = y.p
    d.splitk_ws = ptr(splitk_ws)
    d.B, d.H, d.W, d.Cin, d.Cout = B, H, W, x.cols, y.cols
    d.ksize, d.splitk, d.accumulate = ksize, splitk, int(accumulate)
    d.ldx, d.ldy, d.ldr = x.ld, y.ld, (res.ld if res is not None else 0)
    d.wfmt = wfmt
    d.gn_table, d.gn_silu = ptr(gn_table), int(gn_silu)
    d.colsum, d.stat_mode, d.stat_silu = ptr(colsum), int(stat_mode), int(stat_silu)
    d.stat_x, d.ld_sx = (stat_x.p, stat_x.ld) if stat_x is not None else (None, 0)
    d.stat_table = ptr(stat_table)
    d.x_maxabs = ptr(x_maxabs)
    fam = _same_family(x.t, y.t, res.t if res is not None else None, stat_x.t if stat_x is not None else None)
    if (fam == "_h") != ((wfmt & ~WINOGRAD) == 1):
        raise _lib.OsmosisHipError("fp16 activations go with the fp16 weight image (wfmt 1), fp32 with 0 / 2 / 3")
    call("osm_conv2d_nhwc" + fam, C.byref(d), _s(),
         keep=(x.t, w_packed, bias, y.t, res.t if res else None, splitk_ws, gn_table, colsum,
               stat_x.t if stat_x is not None else None, stat_table, x_maxabs))


MAXABS_PARTS = 1024    # OSM_MAXABS_PARTS


def maxabs(x: Mat, B: int, out: torch.Tensor):
    """out[b][:] = MAXABS_PARTS partial maxima of |x| over image b of an [B * rows][C] fp32 matrix (device-side; no host
    sync, no clearing needed); conv2d(x_maxabs=out) folds them."""
    assert out.numel() >= B * MAXABS_PARTS
    call("osm_maxabs", x.p, x.ld, B, x.rows // B, x.cols, ptr(out), _s(), keep=(x.t, out))


# conv arithmetic modes: weight-image format code of the C ABI
# "f16": activations AND weights in IEEE half, fp32 accumulation (the reference's use_fp16): fp16-storage family
WFMT = {"f32": 0, "f16": 1, "bf16x3": 2, "bf16x6": 3, "f16x3": 4}   # 4: Winograd images and 1x1 layers
WINOGRAD = 0x10   # OSM_WFMT_WINOGRAD: the weight image is in the Winograd F(2x2, 3x3) domain (pack_conv_weight_winograd)


def conv_winograd_ok(H, W, Cin, Cout, ksize, wfmt) -> bool:
    return bool(query("osm_conv_winograd_ok", H, W, Cin, Cout, ksize, wfmt))


def pack_conv_weight_winograd(w_oihw: torch.Tensor, want_fwd=True, want_dgrad=True, wfmt: int = 3):
    """OIHW 3x3 -> (fwd, dgrad) Winograd-domain split-bf16 images; run them with conv2d(wfmt=wfmt | WINOGRAD)."""
    w = w_oihw.contiguous()
    O, I = w.shape[0], w.shape[1]
    assert w.dim() == 4 and w.shape[2] == 3 and w.shape[3] == 3
    lib = _lib.load()
    wf = torch.empty(lib.osm_winograd_weight_elems(O, I, wfmt, 0), device=w.device, dtype=torch.int16) if want_fwd else None
    wd = torch.empty(lib.osm_winograd_weight_elems(O, I, wfmt, 1), device=w.device, dtype=torch.int16) if want_dgrad else None
    call("osm_pack_conv_weight_winograd", ptr(w), ptr(wf), ptr(wd), O, I, wfmt, _s(), keep=(w, wf, wd))
    return wf, wd


def pack_conv_weight(w_oihw: torch.Tensor, want_fwd=True, want_dgrad=True, wfmt: int = 0):
    """OIHW (or [O][I][1] conv1d / [O][I] linear) -> (fwd image, dgrad image).
    wfmt 0: fp32 [k*k][O][I] / [k*k][I][O];  2 / 3: split-bf16 planes, 1: one fp16 plane (int16 tensors)."""
    w = w_oihw.contiguous()
    O, I = w.shape[0], w.shape[1]
    k = w.shape[2] if w.dim() >= 3 else 1
    if wfmt == 0:
        wf = torch.empty(k * k * O * I, device=w.device, dtype=torch.float32) if want_fwd else None
        wd = torch.empty(k * k * O * I, device=w.device, dtype=torch.float32) if want_dgrad else None
        call("osm_pack_conv_weight", ptr(w), ptr(wf), ptr(wd), O, I, k, _s(), keep=(w, wf, wd))
        return wf, wd
    lib = _lib.load()
    nf = lib.osm_packed_weight_elems(O, I, k, wfmt, 0)
    nd = lib.osm_packed_weight_elems(O, I, k, wfmt, 1)
    wf = torch.empty(nf, device=w.device, dtype=torch.int16) if want_fwd else None
    wd = torch.empty(nd, device=w.device, dtype=torch.int16) if want_dgrad else None
    call("osm_pack_conv_weight_bf16s", ptr(w), ptr(wf), ptr(wd), O, I, k, wfmt, _s(), keep=(w, wf, wd))
    return wf, wd


def gemm(A: torch.Tensor, lda: int, Bm: torch.Tensor, ldb: int, Cm: torch.Tensor, ldc: int, M: int, N: int,
         K: int, b_kn: bool = False, alpha: float = 1.0, nb1: int = 1, nb2: int = 1,
         sA=(0, 0), sB=(0, 0), sC=(0, 0), bias=None, res: Optional[torch.Tensor] = None, ldr: int = 0,
         accumulate: bool = False, a_off: int = 0, b_off: int = 0, c_off: int = 0,
         splitk: int = 1, splitk_ws: Optional[torch.Tensor] = None):
    """Raw-pointer GEMM: element offsets (in floats) select sub-matrices of the backing tensors."""
    d = GemmDesc()
    d.A, d.Bm, d.C = ptr(A) + 4 * a_off, ptr(Bm) + 4 * b_off, ptr(Cm) + 4 * c_off
    d.bias = ptr(bias)
    d.res = (ptr(res) + 4 * c_off) if res is not None else None
    d.M, d.N, d.K, d.b_kn = M, N, K, int(b_kn)
    d.nb1, d.nb2, d.accumulate, d.alpha = nb1, nb2, int(accumulate), alpha
    d.lda, d.ldb, d.ldc, d.ldr = lda, ldb, ldc, ldr
    d.sA1, d.sA2 = sA
    d.sB1, d.sB2 = sB
    d.sC1, d.sC2 = sC
    d.splitk, d.splitk_ws = splitk, ptr(splitk_ws)
    call("osm_gemm", C.byref(d), _s(), keep=(A, Bm, Cm, bias, res, splitk_ws))


def attn_small_supported(T: int, ch: int) -> bool:
    return bool(query("osm_attn_small_supported", T, ch))


def _attn_desc(qkv: Mat, B, T, heads, ch, offsets, head_stride, scale) -> AttnDesc:
    d = AttnDesc()
    d.qkv, d.ldqkv = qkv.p, qkv.ld
    d.q_off, d.k_off, d.v_off = offsets
    d.head_stride, d.B, d.T, d.heads, d.ch, d.scale = head_stride, B, T, heads, ch, scale
    return d


def attn_small_fwd(qkv: Mat, out: Mat, B, T, heads, ch, offsets, head_stride, scale):
    """out = softmax(scale q k^T) v per (image, head) in one launch (T in {64, 256})."""
    d = _attn_desc(qkv, B, T, heads, ch, offsets, head_stride, scale)
    d.out, d.ldout = out.p, out.ld
    call("osm_attn_small_fwd", C.byref(d), _s(), keep=(d, qkv.t, out.t))


def attn_small_bwd(qkv: Mat, dout: Mat, dqkv: Mat, ws: torch.Tensor, B, T, heads, ch, offsets, head_stride, scale):
    """dq | dk | dv (qkv column layout) from d(out); ws: 2*B*heads*T*T floats of scratch."""
    d = _attn_desc(qkv, B, T, heads, ch, offsets, head_stride, scale)
    d.dout, d.lddout = dout.p, dout.ld
    d.dqkv, d.lddqkv = dqkv.p, dqkv.ld
    d.ws = ptr(ws)
    call("osm_attn_small_bwd", C.byref(d), _s(), keep=(d, qkv.t, dout.t, dqkv.t, ws))


def attn_flash_supported(T: int, ch: int) -> bool:
    return bool(query("osm_attn_flash_supported", T, ch))


def attn_flash_fwd(qkv: Mat, out: Mat, lse: torch.Tensor, B, T, heads, ch, offsets, head_stride, scale, half: bool = False,
                   f16x3: bool = False):
    """out = softmax(scale q k^T) v per (image, head) on the matrix cores; lse [B*heads*T] is kept for the backward.
    half: one fp16 MFMA per product (the reference's use_fp16 attention arithmetic) instead of bf16x6; f16x3: two IEEE-half
    terms per fp32 operand after a power-of-two scaling found in the kernel, three fp16 MFMAs per product (fp32-class)."""
    d = _attn_desc(qkv, B, T, heads, ch, offsets, head_stride, scale)
    d.arith = 1 if half else (2 if f16x3 else 0)
    d.out, d.ldout = out.p, out.ld
    call("osm_attn_flash_fwd", C.byref(d), ptr(lse), _s(), keep=(d, qkv.t, out.t, lse))


def attn_flash_bwd(qkv: Mat, out: Mat, dout: Mat, dqkv: Mat, lse, delta, B, T, heads, ch, offsets, head_stride, scale,
                   half: bool = False, f16x3: bool = False):
    """dq | dk | dv (qkv column layout) from d(out), the forward output and its lse; delta: [B*heads*T] scratch."""
    d = _attn_desc(qkv, B, T, heads, ch, offsets, head_stride, scale)
    d.arith = 1 if half else (2 if f16x3 else 0)
    d.dout, d.lddout = dout.p, dout.ld
    d.dqkv, d.lddqkv = dqkv.p, dqkv.ld
    call("osm_attn_flash_bwd", C.byref(d), out.p, out.ld, ptr(lse), ptr(delta), _s(),
         keep=(d, qkv.t, out.t, dout.t, dqkv.t, lse, delta))


def splitk_hint(M, N, K, taps, nbatch=1) -> int:
    return query("osm_splitk_hint", M, N, K, taps, nbatch)


def conv_splitk(B, H, W, Cin, Cout, ksize, wfmt, has_gn_table=False) -> int:
    return query("osm_conv_splitk", B, H, W, Cin, Cout, ksize, wfmt, int(bool(has_gn_table)))


def conv_stat_chunks(B, H, W, Cin, Cout, ksize, wfmt, splitk, has_gn_table=False) -> int:
    """Chunks per image of the column sums conv2d(colsum=...) writes for this layer; 0 = its kernel cannot."""
    return query("osm_conv_stat_chunks", B, H, W, Cin, Cout, ksize, wfmt, splitk, int(bool(has_gn_table)))


def gn_finalize_cols(colsum, nchunk, B, HW, C, G, stats, mode=0, gamma=None, beta=None, film=None, table=None,
                     eps: float = 1e-5):
    """GroupNorm statistics (mode 0: mean, rstd [+ the per-channel table]; mode 1: the two backward means) from the
    column sums a convolution wrote next to its output."""
    fp, ldf = _film(film)
    call("osm_gn_finalize_cols", ptr(colsum), nchunk, B, HW, C, G, eps, mode, ptr(stats), ptr(gamma), ptr(beta), fp, ldf,
         ptr(table), _s(), keep=(colsum, stats, gamma, beta, film, table))


def gn_bwd_apply(x: Mat, dy: Mat, dx: Mat, B: int, HW: int, G: int, stats, gstats, gamma, beta, film=None, silu=True,
                 addend: Optional[Mat] = None, addend2: Optional[Mat] = None, maxabs: Optional[torch.Tensor] = None):
    """maxabs (here and in gn_apply / gn_fwd / gn_bwd): [B][MAXABS_PARTS] -- the pass also leaves the per-image partial max of
    |output| there (the ops.maxabs format), for the f16x3 convolution that reads the output next."""
    fp, ldf = _film(film)
    fam = _same_family(x.t, dy.t, dx.t, addend.t if addend is not None else None, addend2.t if addend2 is not None else None)
    call("osm_gn_bwd_apply" + fam, x.p, x.ld, dy.p, dy.ld, dx.p, dx.ld, *_addends(addend, addend2),
         B, HW, x.cols, G, ptr(stats), ptr(gstats), ptr(gamma), ptr(beta), fp, ldf, int(silu), ptr(maxabs), _s(),
         keep=(x.t, dy.t, dx.t, addend.t if addend else None, addend2.t if addend2 else None, stats, gstats, gamma, beta,
               film, maxabs))


def gn_nchunk(HW: int) -> int:
    return query("osm_gn_nchunk", HW)


def gn_stats(x: Mat, B: int, HW: int, G: int, part: torch.Tensor, stats: torch.Tensor, eps: float = 1e-5):
    call("osm_gn_stats" + _fam(x.t), x.p, x.ld, B, HW, x.cols, G, eps, ptr(part), ptr(stats), _s(), keep=(x.t, part, stats))


def _film(film):
    """film: None or a 2-D [B][>=2C] view (row stride = ldfilm)."""
    if film is None:
        return None, 0
    return ptr(film), (film.stride(0) if film.shape[0] > 1 else film.shape[1])


def gn_apply(x: Mat, y: Mat, B: int, HW: int, G: int, stats, gamma, beta, film=None, silu=True, maxabs=None):
    fp, ldf = _film(film)
    call("osm_gn_apply" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, HW, x.cols, G, ptr(stats), ptr(gamma), ptr(beta), fp, ldf,
         int(silu), ptr(maxabs), _s(), keep=(x.t, y.t, stats, gamma, beta, film, maxabs))


def gn_fwd(x: Mat, y: Mat, B: int, HW: int, G: int, part, stats, gamma, beta, film=None, silu=True, eps: float = 1e-5,
           maxabs=None, maxabs_in=None):
    """statistics (written to `stats`) + normalise/FiLM/SiLU; a single launch for HW <= 256.
    maxabs_in: [B][MAXABS_PARTS], the partial max |x| of the INPUT (from the statistics pass; HW > 256 only)."""
    fp, ldf = _film(film)
    call("osm_gn_fwd" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, HW, x.cols, G, eps, ptr(part), ptr(stats), ptr(gamma), ptr(beta),
         fp, ldf, int(silu), ptr(maxabs), ptr(maxabs_in), _s(), keep=(x.t, y.t, part, stats, gamma, beta, film, maxabs, maxabs_in))


def gn_prep(x: Mat, B: int, HW: int, G: int, part, stats, gamma, beta, table, film=None, eps: float = 1e-5, maxabs_in=None):
    """statistics (-> `stats`) + per-channel table [B][4][C] that conv2d(gn_table=...) applies while staging (or that a
    data-gradient convolution's epilogue uses for the GroupNorm-backward reductions).  maxabs_in: as in gn_fwd."""
    fp, ldf = _film(film)
    call("osm_gn_prep" + _fam(x.t), x.p, x.ld, B, HW, x.cols, G, eps, ptr(part), ptr(stats), ptr(gamma), ptr(beta), fp, ldf,
         ptr(table), ptr(maxabs_in), _s(), keep=(x.t, part, stats, gamma, beta, film, table, maxabs_in))


def _addends(addend, addend2):
    a1 = (addend.p, addend.ld) if addend is not None else (None, 0)
    a2 = (addend2.p, addend2.ld) if addend2 is not None else (None, 0)
    return a1 + a2


def gn_bwd(x: Mat, dy: Mat, dx: Mat, B: int, HW: int, G: int, stats, gamma, beta, part, gstats,
           film=None, silu=True, addend: Optional[Mat] = None, addend2: Optional[Mat] = None, maxabs=None):
    """dx = dGN(dy) (+ addend) (+ addend2); an addend may be dx itself (accumulate in place)."""
    fp, ldf = _film(film)
    fam = _same_family(x.t, dy.t, dx.t, addend.t if addend is not None else None, addend2.t if addend2 is not None else None)
    call("osm_gn_bwd" + fam, x.p, x.ld, dy.p, dy.ld, dx.p, dx.ld, *_addends(addend, addend2),
         B, HW, x.cols, G, ptr(stats), ptr(gamma), ptr(beta), fp, ldf, int(silu), ptr(part), ptr(gstats), ptr(maxabs), _s(),
         keep=(x.t, dy.t, dx.t, addend.t if addend else None, addend2.t if addend2 else None, stats, gamma, beta, film,
               part, gstats, maxabs))


def pool2x2(x: Mat, y: Mat, B, H, W, scale=0.25):
    call("osm_pool2x2" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, H, W, x.cols, scale, _s(), keep=(x.t, y.t))


def upsample2x(x: Mat, y: Mat, B, H, W, scale=1.0):
    call("osm_upsample2x" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, H, W, x.cols, scale, _s(), keep=(x.t, y.t))


def softmax_rows(S, P, PT, nmat, T):
    call("osm_softmax_rows", ptr(S), ptr(P), ptr(PT), nmat, T, _s(), keep=(S, P, PT))


def softmax_rows_bwd(P, dP, dS, dST, nmat, T):
    call("osm_softmax_rows_bwd", ptr(P), ptr(dP), ptr(dS), ptr(dST), nmat, T, _s(), keep=(P, dP, dS, dST))


def timestep_embedding(t, out, B, dim, max_period=10000.0):
    call("osm_timestep_embedding", ptr(t), ptr(out), B, dim, max_period, _s(), keep=(t, out))


def linear(x, W, b, y, B, K, N, silu_in=False, silu_out=False):
    call("osm_linear", ptr(x), ptr(W), ptr(b), ptr(y), B, K, N, int(silu_in), int(silu_out), _s(),
         keep=(x, W, b, y))


def resample_pair(up: bool, x1: Mat, y1: Mat, x2: Mat, y2: Mat, B, H, W, scale):
    """pool2x2 (up False) / upsample2x (up True) of two tensors of the same shape in one launch."""
    assert x1.cols == x2.cols == y1.cols == y2.cols
    call("osm_resample_pair" + _same_family(x1.t, y1.t, x2.t, y2.t), int(bool(up)), x1.p, x1.ld, y1.p, y1.ld, x2.p, x2.ld, y2.p, y2.ld,
         B, H, W, x1.cols, scale, _s(), keep=(x1.t, y1.t, x2.t, y2.t))


def stride2_pick(x: Mat, y: Mat, B, H, W):
    """y[b][i][j] = x[b][2i][2j]  (x: [B*H*W][C] -> y: [B*(H/2)*(W/2)][C]): a stride-2 convolution from its stride-1 result."""
    call("osm_stride2_pick" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, H, W, x.cols, _s(), keep=(x.t, y.t))


def stride2_place(x: Mat, y: Mat, B, H, W):
    """y[b][2i][2j] = x[b][i][j], zero elsewhere (H, W: the output's): the adjoint of stride2_pick."""
    call("osm_stride2_place" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, B, H, W, x.cols, _s(), keep=(x.t, y.t))


def add_rowvec(y: Mat, v: torch.Tensor, ldv: int, B, HW):
    """y[b][p][c] += v[b][c] (v fp32 [B][ldv])."""
    call("osm_add_rowvec" + _fam(y.t), y.p, y.ld, ptr(v), ldv, B, HW, y.cols, _s(), keep=(y.t, v))


def nchw_to_nhwc(x, y: Mat, B, Cc, HW):
    call("osm_nchw_to_nhwc" + _fam(y.t), ptr(x), y.p, y.ld, B, Cc, HW, _s(), keep=(x, y.t))


def nhwc_to_nchw(x: Mat, y, B, Cc, HW):
    call("osm_nhwc_to_nchw" + _fam(x.t), x.p, x.ld, ptr(y), B, Cc, HW, _s(), keep=(x.t, y))


def copy2d(x: Mat, y: Mat, accumulate=False):
    call("osm_copy2d" + _same_family(x.t, y.t), x.p, x.ld, y.p, y.ld, x.rows, x.cols, int(accumulate), _s(),
         keep=(x.t, y.t))


def convert(x: Mat, y: Mat):
    """y = x across the two activation storage types (half -> fp32 or fp32 -> half), [rows][cols] strided."""
    fx, fy = _fam(x.t), _fam(y.t)
    if fx == fy:
        raise _lib.OsmosisHipError("convert() is for half <-> fp32; use copy2d within one storage type")
    call("osm_half_to_f32" if fx == "_h" else "osm_f32_to_half", x.p, x.ld, y.p, y.ld, x.rows, x.cols, _s(),
         keep=(x.t, y.t))


# ----------------------------------------------------------------------------- sampler step
def posterior(model_out, x, coef, x0, mean, logvar, B, HW, mean_kind=0, var_kind=0, x0_raw=None):
    """mean_kind / var_kind: `MeanProcessor.kernel_kind` / `VarianceProcessor.kernel_kind` (include/osmosis_hip.h osm_posterior_typed);
    (0, 0) = the epsilon / learned_range pair of every shipped config.  x0_raw given = `clip_denoised`: x0 is clamped to [-1, 1] and
    the unclamped prediction lands in x0_raw (for `clamp_bwd`)."""
    call("osm_posterior_typed", ptr(model_out), ptr(x), ptr(coef), int(mean_kind), int(var_kind), 0 if x0_raw is None else 1,
         ptr(x0_raw), ptr(x0), ptr(mean), ptr(logvar), B, HW, _s(), keep=(model_out, x, coef, x0_raw, x0, mean, logvar))


def clamp_bwd(g, x_raw, lo=-1.0, hi=1.0):
    """g (in place) = 0 where x_raw is outside [lo, hi]: the backward of `x_raw.clamp(lo, hi)`."""
    assert g.numel() == x_raw.numel() and g.is_contiguous() and x_raw.is_contiguous()
    call("osm_clamp_bwd", ptr(g), ptr(x_raw), float(lo), float(hi), g.numel(), _s(), keep=(g, x_raw))


QUANTILE_MAX_N = 1 << 24      # torch.quantile's limit, kept by osm_quantile_abs


def quantile_ws_bytes(n: int) -> int:
    """Bytes of the device workspace `quantile_abs` / `posterior_dynthr` / `dynthr_bwd` take for n elements."""
    b = query("osm_quantile_abs_ws_bytes", int(n))
    if b < 0:
        raise _lib.OsmosisHipError(f"quantile() input tensor is too large ({n} elements > 2^24)" if n > QUANTILE_MAX_N
                                   else f"quantile of {n} elements")
    return int(b)


def quantile_workspace(n: int, device) -> torch.Tensor:
    """A workspace for `quantile_abs` / `posterior_dynthr` / `dynthr_bwd` over n elements (int32, 16-byte aligned)."""
    return torch.empty(-(-quantile_ws_bytes(n) // 4), device=device, dtype=torch.int32)


def quantile_abs(x, s, q, idx, ws):
    """q[0] = torch.quantile(x.abs(), s) (linear), idx[0:2] = flat indices of the two order statistics (stable-sort order); x is read
    as a flat fp32 tensor.  q: fp32 [1], idx: int32 [2], ws: `quantile_workspace(x.numel())`."""
    assert x.is_contiguous() and q.numel() >= 1 and idx.numel() >= 2 and idx.dtype == torch.int32
    call("osm_quantile_abs", ptr(x), x.numel(), float(s), ptr(q), ptr(idx), ptr(ws), _s(), keep=(x, q, idx, ws))


def posterior_dynthr(model_out, x, coef, x0, mean, logvar, x0_raw, q, idx, ws, B, HW, mean_kind=0, var_kind=0, s=0.98):
    """`posterior` with dynamic_threshold: x0 = clip(q x0_raw, -1, 1), q = quantile(|x0_raw|, s) over the whole [B,4,H,W] batch (left on
    the device in q, its order statistics in idx), the mean formed from that x0."""
    call("osm_posterior_dynthr", ptr(model_out), ptr(x), ptr(coef), int(mean_kind), int(var_kind), float(s), ptr(x0_raw), ptr(x0),
         ptr(mean), ptr(logvar), ptr(q), ptr(idx), ptr(ws), B, HW, _s(), keep=(model_out, x, coef, x0_raw, x0, mean, logvar, q, idx, ws))


def dynthr_bwd(g, x_raw, q, idx, ws, s=0.98):
    """g (in place) = d loss/d x0_raw from d loss/d x0 through x0 = clip(x_raw * quantile(|x_raw|, s), -1, 1) (q / idx of the forward)."""
    assert g.numel() == x_raw.numel() and g.is_contiguous() and x_raw.is_contiguous()
    call("osm_dynthr_bwd", ptr(g), ptr(x_raw), ptr(q), ptr(idx), float(s), g.numel(), ptr(ws), _s(), keep=(g, x_raw, q, idx, ws))


def phys_nblk(HW):
    return query("osm_phys_nblk", HW)


def _check_lm_part(desc, part):
    """The Levenberg-Marquardt solver's reduce (desc.optimizer = 9) writes 32 floats per workgroup where the plain one writes 16."""
    if desc.optimizer == 9 and part.numel() < desc.B * phys_nblk(desc.HW) * 32:
        raise ValueError(f"optimizer 9 (lm): part must hold B * nblk * 32 = {desc.B * phys_nblk(desc.HW) * 32} floats, got {part.numel()}")


def phys_reduce(desc: PhysDesc, x0, y, phi, part):
    _check_lm_part(desc, part)
    call("osm_phys_reduce", C.byref(desc), ptr(x0), ptr(y), ptr(phi), ptr(part), _s(), keep=(desc, x0, y, phi, part))


def phys_finalize(desc: PhysDesc, part, red, phi, do_update, loss_out, opt_state=None):
    call("osm_phys_finalize", C.byref(desc), ptr(part), ptr(red), ptr(phi), int(do_update), ptr(loss_out), ptr(opt_state), _s(),
         keep=(part, red, phi, loss_out, opt_state))


def phys_grad(desc: PhysDesc, x0, y, phi, red, g):
    call("osm_phys_grad", C.byref(desc), ptr(x0), ptr(y), ptr(phi), ptr(red), ptr(g), _s(),
         keep=(desc, x0, y, phi, red, g))


def phys_optimize(desc: PhysDesc, x0, y, phi, part, red, loss_out, g, n_inner: int, freeze_phi: bool, opt_state=None):
    """The whole inner phi loop of a guided step (n_inner reduce / finalize pairs, loss and dL/dx0 at the last phi, then its step)
    enqueued by one call."""
    _check_lm_part(desc, part)
    call("osm_phys_optimize", C.byref(desc), ptr(x0), ptr(y), ptr(phi), ptr(part), ptr(red), ptr(loss_out), ptr(g), int(n_inner),
         int(bool(freeze_phi)), ptr(opt_state), _s(), keep=(desc, x0, y, phi, part, red, loss_out, g, opt_state))


def _check_mask(mask, y):
    """A mask travels as [B,3,HW] rows laid out like the measurement it weighs (the kernels address it like y)."""
    if mask is not None and (mask.numel() != y.numel() or not mask.is_contiguous() or mask.dtype != torch.float32):
        raise ValueError(f"mask must be contiguous fp32 with the measurement's {y.numel()} elements ([B,3,HW]), "
                         f"got {tuple(mask.shape)} {mask.dtype}")


def phys_reduce_m(desc: PhysDesc, x0, y, mask, phi, part):
    """osm_phys_reduce with a validity mask [B,3,HW] in the residual (None: the plain launch)."""
    _check_mask(mask, y)
    _check_lm_part(desc, part)
    call("osm_phys_reduce_m", C.byref(desc), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(part), _s(), keep=(desc, x0, y, mask, phi, part))


def phys_finalize_m(desc: PhysDesc, part, red, phi, do_update, loss_out, opt_state=None, masked=True):
    """The finalize of the masked path: an image whose residual sum is exactly 0 (fully masked) takes no phi step."""
    call("osm_phys_finalize_m", C.byref(desc), ptr(part), ptr(red), ptr(phi), int(do_update), ptr(loss_out), ptr(opt_state),
         int(bool(masked)), _s(), keep=(part, red, phi, loss_out, opt_state))


def phys_grad_m(desc: PhysDesc, x0, y, mask, phi, red, g):
    _check_mask(mask, y)
    call("osm_phys_grad_m", C.byref(desc), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(red), ptr(g), _s(),
         keep=(desc, x0, y, mask, phi, red, g))


def phys_optimize_m(desc: PhysDesc, x0, y, mask, phi, part, red, loss_out, g, n_inner: int, freeze_phi: bool, opt_state=None):
    """`phys_optimize` with a validity mask [B,3,HW] (None: the same launches as `phys_optimize`)."""
    _check_mask(mask, y)
    _check_lm_part(desc, part)
    call("osm_phys_optimize_m", C.byref(desc), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(part), ptr(red), ptr(loss_out), ptr(g),
         int(n_inner), int(bool(freeze_phi)), ptr(opt_state), _s(), keep=(desc, x0, y, mask, phi, part, red, loss_out, g, opt_state))


def exposure_mask(y, mask_out, B, HW, low, high, soft=0.0, per_pixel=False):
    """mask_out [B,3,HW] from the exposure of y [B,3,HW] in [-1, 1] (osm_exposure_mask)."""
    assert y.numel() == B * 3 * HW and mask_out.numel() == B * 3 * HW and y.is_contiguous() and mask_out.is_contiguous()
    call("osm_exposure_mask", ptr(y), float(low), float(high), float(soft), int(bool(per_pixel)), ptr(mask_out), B, HW, _s(),
         keep=(y, mask_out))


def posterior_bwd(g, coef, d_out, B, HW):
    call("osm_posterior_bwd", ptr(g), ptr(coef), ptr(d_out), B, HW, _s(), keep=(g, coef, d_out))


def guide_update(mean, logvar, g, dx_unet, noise, coef, scale4, clip, x_next, grad_out, B, HW):
    call("osm_guide_update", ptr(mean), ptr(logvar), ptr(g), ptr(dx_unet), ptr(noise), ptr(coef), ptr(scale4),
         float(clip), ptr(x_next), ptr(grad_out), B, HW, _s(),
         keep=(mean, logvar, g, dx_unet, noise, coef, scale4, x_next, grad_out))


def guide_update_rng(mean, logvar, g, dx_unet, coef, scale4, clip, x_next, grad_out, noise_out, B, HW, seed, step, step_offset=0,
                     img0=0, img_stride=1):
    """osm_guide_update with the step noise drawn in the kernel: Philox-4x32-10 keyed by `seed`, counter (element / 4,
    img0 + b * img_stride, *step + step_offset)."""
    call("osm_guide_update_rng", ptr(mean), ptr(logvar), ptr(g), ptr(dx_unet), ptr(coef), ptr(scale4), float(clip), ptr(x_next),
         ptr(grad_out), ptr(noise_out), B, HW, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_offset), int(img0), int(img_stride), _s(),
         keep=(mean, logvar, g, dx_unet, coef, scale4, x_next, grad_out, noise_out, step))


def guide_update_rng_sub(mean, logvar, g, dx_unet, coef, scale4, clip, x_next, grad_out, noise_out, B, HW, seed, step, step_offset=0,
                         sub=0, img0=0, img_stride=1):
    """guide_update_rng for sub-step `sub` of a step repeated at the same t (PCGS local_M): counter word 2 =
    (*step + step_offset) | sub << 16; sub = 0 draws what guide_update_rng draws."""
    call("osm_guide_update_rng_sub", ptr(mean), ptr(logvar), ptr(g), ptr(dx_unet), ptr(coef), ptr(scale4), float(clip), ptr(x_next),
         ptr(grad_out), ptr(noise_out), B, HW, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_offset), int(sub), int(img0),
         int(img_stride), _s(), keep=(mean, logvar, g, dx_unet, coef, scale4, x_next, grad_out, noise_out, step))


def randn(out, B, n, seed, step=None, step_const=0, img0=0, img_stride=1):
    """out[B][n] ~ N(0, 1) from the library's generator (what osm_guide_update_rng draws for (seed, image, step) when n = 4 H W)."""
    call("osm_randn", ptr(out), int(B), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_const), int(img0), int(img_stride), _s(),
         keep=(out, step))


def randn_sub(out, B, n, seed, step=None, step_const=0, sub=0, img0=0, img_stride=1):
    """randn for sub-step `sub` (counter word 2 = step | sub << 16): what guide_update_rng_sub draws for (seed, image, step, sub)."""
    call("osm_randn_sub", ptr(out), int(B), int(n), int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_const), int(sub), int(img0),
         int(img_stride), _s(), keep=(out, step))


def philox_raw(out, n4, c1, c2, c3, k0, k1):
    call("osm_philox_raw", ptr(out), int(n4), int(c1), int(c2), int(c3), int(k0), int(k1), _s(), keep=(out,))


def ddim_update(x0, x, g, dx_unet, noise, coef, dcoef, scale4, clip, x_next, grad_out, B, HW):
    call("osm_ddim_update", ptr(x0), ptr(x), ptr(g), ptr(dx_unet), ptr(noise), ptr(coef), ptr(dcoef), ptr(scale4), float(clip),
         ptr(x_next), ptr(grad_out), B, HW, _s(), keep=(x0, x, g, dx_unet, noise, coef, dcoef, scale4, x_next, grad_out))


def fetch_coefs(table, step, delta, coef_out, t_out, B):
    """table: [n_rows][8] device fp32; the device-side row counter `step` is clamped to the table."""
    call("osm_fetch_coefs", ptr(table), int(table.shape[0]), ptr(step), delta, ptr(coef_out), ptr(t_out), B, _s(),
         keep=(table, step, coef_out, t_out))


def ancestral_step(model_out, x, z, coef, x_next, x0, B, Cc, Cout, HW):
    call("osm_ancestral_step", ptr(model_out), ptr(x), ptr(z), ptr(coef), ptr(x_next), ptr(x0), B, Cc, Cout, HW, _s(),
         keep=(model_out, x, z, coef, x_next, x0))


# ----------------------------------------------------------------------------- channel-generic sampler step ([B,C,HW] / [B,Cout,HW])
def posterior_c(model_out, x, coef, x0, mean, logvar, B, Cc, Cout, HW, mean_kind=0, var_kind=0, x0_raw=None):
    """`posterior` for a C-channel state and a Cout-channel network output (Cout = C: no variance half, the variance processor
    reads model_out itself)."""
    call("osm_posterior_c", ptr(model_out), ptr(x), ptr(coef), int(mean_kind), int(var_kind), 0 if x0_raw is None else 1,
         ptr(x0_raw), ptr(x0), ptr(mean), ptr(logvar), B, Cc, Cout, HW, _s(), keep=(model_out, x, coef, x0_raw, x0, mean, logvar))


def posterior_dynthr_c(model_out, x, coef, x0, mean, logvar, x0_raw, q, idx, ws, B, Cc, Cout, HW, mean_kind=0, var_kind=0, s=0.98):
    """`posterior_dynthr` over a [B,C,H,W] batch (ws: `quantile_workspace(B * C * HW)`)."""
    call("osm_posterior_dynthr_c", ptr(model_out), ptr(x), ptr(coef), int(mean_kind), int(var_kind), float(s), ptr(x0_raw), ptr(x0),
         ptr(mean), ptr(logvar), ptr(q), ptr(idx), ptr(ws), B, Cc, Cout, HW, _s(),
         keep=(model_out, x, coef, x0_raw, x0, mean, logvar, q, idx, ws))


def posterior_bwd_c(g, coef, d_out, B, Cc, Cout, HW):
    call("osm_posterior_bwd_c", ptr(g), ptr(coef), ptr(d_out), B, Cc, Cout, HW, _s(), keep=(g, coef, d_out))


def guide_update_c(mean, logvar, g, dx_unet, noise, coef, scale, clip, x_next, grad_out, B, Cc, HW):
    call("osm_guide_update_c", ptr(mean), ptr(logvar), ptr(g), ptr(dx_unet), ptr(noise), ptr(coef), ptr(scale),
         float(clip), ptr(x_next), ptr(grad_out), B, Cc, HW, _s(),
         keep=(mean, logvar, g, dx_unet, noise, coef, scale, x_next, grad_out))


def guide_update_rng_c(mean, logvar, g, dx_unet, coef, scale, clip, x_next, grad_out, noise_out, B, Cc, HW, seed, step, step_offset=0,
                       sub=0, img0=0, img_stride=1):
    """`guide_update_rng_sub` on [B,C,HW]: counter (element / 4 of the image's C HW elements, img0 + b * img_stride,
    (*step + step_offset) | sub << 16)."""
    call("osm_guide_update_rng_c", ptr(mean), ptr(logvar), ptr(g), ptr(dx_unet), ptr(coef), ptr(scale), float(clip), ptr(x_next),
         ptr(grad_out), ptr(noise_out), B, Cc, HW, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_offset), int(sub), int(img0),
         int(img_stride), _s(), keep=(mean, logvar, g, dx_unet, coef, scale, x_next, grad_out, noise_out, step))


def ddim_update_c(x0, x, g, dx_unet, noise, coef, dcoef, scale, clip, x_next, grad_out, B, Cc, HW):
    call("osm_ddim_update_c", ptr(x0), ptr(x), ptr(g), ptr(dx_unet), ptr(noise), ptr(coef), ptr(dcoef), ptr(scale), float(clip),
         ptr(x_next), ptr(grad_out), B, Cc, HW, _s(), keep=(x0, x, g, dx_unet, noise, coef, dcoef, scale, x_next, grad_out))


def solver_update_c(x0, x, hist, g, dx_unet, noise, coef, srow, scale, clip, x_next, grad_out, noise_out, B, Cc, HW):
    """The few-step solver step (osm_solver_update_c, include/osmosis_solver.h): x_next = A x + B0 x0 + B1 hist + S noise -
    scale[c] clamp(c0 g + dx_unet) with srow = [A, B0, B1, S, noise_on, ..] (`gaussian_diffusion.solver_table`), then hist <- x0.
    x_next may alias x; hist is read only when B1 != 0."""
    call("osm_solver_update_c", ptr(x0), ptr(x), ptr(hist), ptr(g), ptr(dx_unet), ptr(noise), ptr(coef), ptr(srow), ptr(scale),
         float(clip), ptr(x_next), ptr(grad_out), ptr(noise_out), B, Cc, HW, _s(),
         keep=(x0, x, hist, g, dx_unet, noise, coef, srow, scale, x_next, grad_out, noise_out))


def solver_update_rng_c(x0, x, hist, g, dx_unet, coef, srow, scale, clip, x_next, grad_out, noise_out, B, Cc, HW, seed, step,
                        step_offset=0, sub=0, img0=0, img_stride=1):
    """`solver_update_c` with the noise drawn in the kernel: the counter words of `guide_update_rng_c`, so `randn_sub` draws the same."""
    call("osm_solver_update_rng_c", ptr(x0), ptr(x), ptr(hist), ptr(g), ptr(dx_unet), ptr(coef), ptr(srow), ptr(scale), float(clip),
         ptr(x_next), ptr(grad_out), ptr(noise_out), B, Cc, HW, int(seed) & 0xFFFFFFFFFFFFFFFF, ptr(step), int(step_offset), int(sub),
         int(img0), int(img_stride), _s(), keep=(x0, x, hist, g, dx_unet, coef, srow, scale, x_next, grad_out, noise_out, step))


def ps_loss_grad_c(x0, y, part, loss, g, B, Cc, HW):
    """loss[b] = ||y[b] - x0[b, 0:3]||, g = d loss / d x0 (zero beyond channel 2); part: fp32 [B * phys_nblk(HW)] workspace."""
    call("osm_ps_loss_grad_c", ptr(x0), ptr(y), ptr(part), ptr(loss), ptr(g), B, Cc, HW, _s(), keep=(x0, y, part, loss, g))


def ps_loss_grad_mc(x0, y, mask, part, loss, g, B, Cc, HW):
    """`ps_loss_grad_c` with a validity mask [B,3,HW]: loss[b] = ||M (y - x0[0:3])||, g = -M^2 (y - x0) / loss (None: unmasked)."""
    _check_mask(mask, y)
    call("osm_ps_loss_grad_mc", ptr(x0), ptr(y), ptr(mask), ptr(part), ptr(loss), ptr(g), B, Cc, HW, _s(),
         keep=(x0, y, mask, part, loss, g))


RECON_MODES = {"bilinear": 0, "joint_bilateral": 1}


def recon_fullres(depth, guide, image, phi_a, phi_b, phi_inf, depth_type, dval, amap, rgb, rgb_u8=None, depth_full=None,
                  mode=0, radius=2, sigma_s=1.0, sigma_r=0.1):
    """rgb [3,Hc,Wc] = exp(phi_a D) (image - phi_inf (1 - exp(-phi_b D))), D = convert_depth(raw depth [h,w] upsampled to the
    image's grid) (osm_recon_fullres).  guide [3,h,w] and image [3,Hc,Wc] in [0,1]; phi_*: fp32 [3]; amap = (ay, by, ax, bx):
    image pixel (i, j) -> network-grid coordinate (ay i + by, ax j + bx); mode 0 bilinear, 1 joint bilateral upsampling.
    Optional outputs: rgb_u8 [Hc,Wc,3] uint8 (truncated), depth_full [Hc,Wc] (the upsampled raw depth)."""
    h, w = depth.shape[-2:]
    Hc, Wc = image.shape[-2:]
    f32 = [depth, guide, image, phi_a, phi_b, phi_inf, rgb] + ([depth_full] if depth_full is not None else [])
    if any(t.dtype != torch.float32 or not t.is_contiguous() for t in f32):
        raise _lib.OsmosisHipError("recon_fullres takes contiguous fp32 tensors")
    if (depth.numel() != h * w or tuple(guide.shape) != (3, h, w) or image.dim() != 3 or image.shape[0] != 3
            or tuple(rgb.shape) != (3, Hc, Wc) or min(phi_a.numel(), phi_b.numel(), phi_inf.numel()) < 3):
        raise _lib.OsmosisHipError("recon_fullres: expected depth [h,w], guide [3,h,w], image / rgb [3,Hc,Wc], phi [3]")
    if depth_full is not None and tuple(depth_full.shape) != (Hc, Wc):
        raise _lib.OsmosisHipError("recon_fullres: depth_full must be [Hc,Wc]")
    u8p = None
    if rgb_u8 is not None:
        if not rgb_u8.is_cuda or rgb_u8.dtype != torch.uint8 or not rgb_u8.is_contiguous() or tuple(rgb_u8.shape) != (Hc, Wc, 3):
            raise _lib.OsmosisHipError("recon_fullres: rgb_u8 must be a contiguous CUDA(HIP) uint8 [Hc,Wc,3] tensor")
        u8p = rgb_u8.data_ptr()
    d = ReconDesc()
    d.depth, d.guide, d.image = ptr(depth), ptr(guide), ptr(image)
    d.phi_a, d.phi_b, d.phi_inf = ptr(phi_a), ptr(phi_b), ptr(phi_inf)
    d.rgb, d.rgb_u8, d.depth_full = ptr(rgb), u8p, ptr(depth_full)
    d.h, d.w, d.Hc, d.Wc = h, w, Hc, Wc
    d.depth_type = int(depth_type)
    for i in range(3):
        d.dval[i] = float(dval[i])
    d.ay, d.by, d.ax, d.bx = (float(v) for v in amap)
    d.mode, d.radius, d.sigma_s, d.sigma_r = int(mode), int(radius), float(sigma_s), float(sigma_r)
    call("osm_recon_fullres", C.byref(d), _s(), keep=(d, depth, guide, image, phi_a, phi_b, phi_inf, rgb, rgb_u8, depth_full))


# ----------------------------------------------------------------------------- tiled sampling (canvas <-> overlapping tiles)
def _tile_args(what, canvas, tiles, origins, wy, wx, inv_norm):
    """Shapes of one osm_tile_* call: canvas [C,Hc,Wc] (or [1,C,Hc,Wc]), tiles [n,C,th,tw], origins int32 [n,2] on the device,
    wy [th] / wx [tw] / inv_norm [Hc,Wc] all None or all given."""
    if canvas.dim() == 4 and canvas.shape[0] == 1:
        canvas = canvas[0]
    if canvas.dim() != 3 or tiles.dim() != 4 or tiles.shape[1] != canvas.shape[0]:
        raise _lib.OsmosisHipError(f"{what}: expected canvas [C,Hc,Wc] and tiles [n,C,th,tw], got {tuple(canvas.shape)} and "
                                   f"{tuple(tiles.shape)}")
    Cc, Hc, Wc = canvas.shape
    n, _, th, tw = tiles.shape
    weights = (wy, wx, inv_norm)
    if any(w is None for w in weights) != all(w is None for w in weights):
        raise _lib.OsmosisHipError(f"{what}: wy, wx and inv_norm are given together or not at all")
    for t in (canvas, tiles) + tuple(w for w in weights if w is not None):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError(f"{what} takes contiguous fp32 tensors")
    if origins.dtype != torch.int32 or not origins.is_contiguous() or tuple(origins.shape) != (n, 2):
        raise _lib.OsmosisHipError(f"{what}: origins must be a contiguous int32 [{n},2] tensor, got {tuple(origins.shape)} {origins.dtype}")
    if wy is not None and (wy.numel() != th or wx.numel() != tw or inv_norm.numel() != Hc * Wc):
        raise _lib.OsmosisHipError(f"{what}: expected wy [{th}], wx [{tw}] and inv_norm [{Hc},{Wc}]")
    return canvas, (n, Cc, Hc, Wc, th, tw)


def tile_gather(canvas, tiles, origins, wy=None, wx=None, inv_norm=None):
    """tiles[t,c,y,x] = canvas[c,oy+y,ox+x] k (osm_tile_gather): k = 1 without weights (a bit-exact crop), else
    wy[y] wx[x] inv_norm[oy+y,ox+x] -- the adjoint of `tile_blend` with the same weights."""
    canvas, dims = _tile_args("tile_gather", canvas, tiles, origins, wy, wx, inv_norm)
    call("osm_tile_gather", ptr(canvas), ptr(tiles), ptr(origins), ptr(wy), ptr(wx), ptr(inv_norm), *dims, _s(),
         keep=(canvas, tiles, origins, wy, wx, inv_norm))


def tile_blend(tiles, canvas, origins, wy=None, wx=None, inv_norm=None):
    """canvas[c,Y,X] = inv_norm[Y,X] sum_t wy wx tiles[t,c,Y-oy,X-ox] over the covering tiles in ascending t (osm_tile_blend; no
    weights: the plain sum; an uncovered pixel is 0).  Deterministic: gather form, no atomics."""
    canvas, dims = _tile_args("tile_blend", canvas, tiles, origins, wy, wx, inv_norm)
    call("osm_tile_blend", ptr(tiles), ptr(canvas), ptr(origins), ptr(wy), ptr(wx), ptr(inv_norm), *dims, _s(),
         keep=(canvas, tiles, origins, wy, wx, inv_norm))


# ----------------------------------------------------------------------------- separable banded linear operators
def linop_apply(x, out, start_h, wt_h, start_w, wt_w, B, P, x_img_stride, out_img_stride, Hin, Win, zero_planes=0):
    """out[b,p,i,j] = sum_a wt_h[i][a] sum_c wt_w[j][c] x[b,p,start_h[i]+a,start_w[j]+c] for p < P (osm_linop_apply,
    include/osmosis_linop.h); `zero_planes` further planes of every output image are written as 0.  x / out: contiguous fp32
    with image strides in elements (the colour planes of a [B,4,HW] tensor: stride 4 HW, P = 3); tables on the device: start int32
    [n_out], wt fp32 [n_out,K].  With the transposed tables the call is the exact adjoint; deterministic (gather form, no atomics)."""
    for t in (x, out, wt_h, wt_w):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("linop_apply takes contiguous fp32 tensors")
    for s, w in ((start_h, wt_h), (start_w, wt_w)):
        if s.dtype != torch.int32 or not s.is_contiguous() or w.dim() != 2 or s.dim() != 1 or s.shape[0] != w.shape[0]:
            raise _lib.OsmosisHipError(f"linop_apply: a band table is start int32 [n] with wt fp32 [n,K], got {tuple(s.shape)} {s.dtype} "
                                       f"and {tuple(w.shape)}")
    (Hout, Kh), (Wout, Kw) = wt_h.shape, wt_w.shape
    B, P, Z = int(B), int(P), int(zero_planes)
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * Hin * Win
                   or out.numel() < (B - 1) * int(out_img_stride) + (P + Z) * Hout * Wout):
        raise _lib.OsmosisHipError(f"linop_apply: x ({x.numel()} elements) / out ({out.numel()}) are smaller than {B} images of "
                                   f"{P} x {Hin} x {Win} -> {P + Z} x {Hout} x {Wout} at strides {x_img_stride} / {out_img_stride}")
    call("osm_linop_apply", ptr(x), ptr(out), ptr(start_h), ptr(wt_h), ptr(start_w), ptr(wt_w), B, P, int(x_img_stride),
         int(out_img_stride), int(Hin), int(Win), int(Hout), int(Wout), int(Kh), int(Kw), Z, _s(),
         keep=(x, out, start_h, wt_h, start_w, wt_w))


# ----------------------------------------------------------------------------- point-spread-function operators
def psf_apply(x, out, dy, dx, w, Ry, Rx, B, P, x_img_stride, out_img_stride, H, W, adjoint=False, zero_planes=0):
    """out[b,p,i,j] = sum_t w[t] x[b,p,refl(i+dy[t]),refl(j+dx[t])] for p < P over torch 'reflect' padding (osm_psf_apply,
    include/osmosis_psf.h), or with `adjoint` the exact transpose of that map; `zero_planes` further planes of every output image
    are written as 0.  x / out: contiguous fp32 on the same H x W grid with image strides in elements (the colour planes of a
    [B,4,HW] tensor: stride 4 HW, P = 3); the tap list on the device: dy, dx int32 [T], w fp32 [T]; Ry >= max |dy|, Rx >= max |dx|
    (a tap beyond them is skipped).  Deterministic (gather form, no atomics)."""
    for t in (x, out, w):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_apply takes contiguous fp32 tensors")
    for d in (dy, dx):
        if d.dtype != torch.int32 or not d.is_contiguous() or d.dim() != 1 or w.dim() != 1 or d.shape[0] != w.shape[0]:
            raise _lib.OsmosisHipError(f"psf_apply: a tap list is dy, dx int32 [T] with w fp32 [T], got {tuple(d.shape)} {d.dtype} "
                                       f"and {tuple(w.shape)}")
    B, P, Z, H, W = int(B), int(P), int(zero_planes), int(H), int(W)
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * H * W
                   or out.numel() < (B - 1) * int(out_img_stride) + (P + Z) * H * W):
        raise _lib.OsmosisHipError(f"psf_apply: x ({x.numel()} elements) / out ({out.numel()}) are smaller than {B} images of "
                                   f"{P} -> {P + Z} planes of {H} x {W} at strides {x_img_stride} / {out_img_stride}")
    call("osm_psf_apply", ptr(x), ptr(out), ptr(dy), ptr(dx), ptr(w), int(w.shape[0]), int(Ry), int(Rx), B, P, int(x_img_stride),
         int(out_img_stride), H, W, 1 if adjoint else 0, Z, _s(), keep=(x, out, dy, dx, w))


# ----------------------------------------------------------------------------- blind deblurring (include/osmosis_blind.h)
BLIND_MAX_TAPS = 4225
BLIND_MAX_RADIUS = 32


def tap_grad_nparts(P, H, W):
    """Partials per image osm_psf_tap_grad writes for P planes of H x W: one per 32 x 32 tile and plane."""
    return int(P) * (-(-int(H) // 32)) * (-(-int(W) // 32))


def _check_tap_lists(name, dy, dx, w=None):
    for d in (dy, dx):
        if d.dtype != torch.int32 or not d.is_contiguous() or d.dim() != 1 or d.shape[0] != dy.shape[0]:
            raise _lib.OsmosisHipError(f"{name}: a tap list is dy, dx int32 [T], got {tuple(d.shape)} {d.dtype}")
    if w is not None and (w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 1 or w.shape[0] != dy.shape[0]):
        raise _lib.OsmosisHipError(f"{name}: the weights are fp32 [T = {dy.shape[0]}], got {tuple(w.shape)} {w.dtype}")


def psf_tap_grad(x, r, dy, dx, Ry, Rx, B, P, x_img_stride, r_img_stride, H, W, part):
    """part[b][q][t] = the tile partials of c_b[t] = sum_p sum_ij r[b,p,i,j] x[b,p,refl(i+dy[t]),refl(j+dx[t])] (osm_psf_tap_grad,
    include/osmosis_blind.h): q = p ntiles + tile, `tap_grad_nparts(P, H, W)` per image; c is their sum (fp64 in `psf_tap_step`).
    x / r: contiguous fp32 with image strides in elements; part fp32 with at least B nparts T elements, every one written.
    Deterministic (gather form, no atomics)."""
    for t in (x, r, part):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_tap_grad takes contiguous fp32 tensors")
    _check_tap_lists("psf_tap_grad", dy, dx)
    B, P, H, W, T = int(B), int(P), int(H), int(W), int(dy.shape[0])
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * H * W or r.numel() < (B - 1) * int(r_img_stride) + P * H * W
                   or part.numel() < B * tap_grad_nparts(P, H, W) * T):
        raise _lib.OsmosisHipError(f"psf_tap_grad: x ({x.numel()} elements) / r ({r.numel()}) / part ({part.numel()}) are smaller than "
                                   f"{B} images of {P} x {H} x {W} at strides {x_img_stride} / {r_img_stride} with {T} taps")
    call("osm_psf_tap_grad", ptr(x), ptr(r), ptr(dy), ptr(dx), T, int(Ry), int(Rx), B, P, int(x_img_stride), int(r_img_stride), H, W,
         ptr(part), _s(), keep=(x, r, dy, dx, part))


def psf_tap_step(w, part, loss, B, nparts, hw3, eta, l1=0.0):
    """One projected step of the PSF weights w fp32 [T], in place (osm_psf_tap_step): fp64 throughout, g = sum_b loss[b] c_b / hw3,
    u = max(w - eta (g - mean g) - eta l1, 0), w = u / sum u -- left untouched when the sum is 0 or not finite."""
    for t in (w, part, loss):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_tap_step takes contiguous fp32 tensors")
    B, nparts, T = int(B), int(nparts), int(w.numel())
    if B >= 1 and (part.numel() < B * nparts * T or loss.numel() < B):
        raise _lib.OsmosisHipError(f"psf_tap_step: part ({part.numel()} elements) / loss ({loss.numel()}) are smaller than {B} x {nparts} x {T} / {B}")
    call("osm_psf_tap_step", ptr(w), ptr(part), ptr(loss), B, nparts, T, int(hw3), float(eta), float(l1), _s(), keep=(w, part, loss))


def ps_blind_optimize(x0, y, mask, dy, dx, w, Ry, Rx, B, Cc, H, W, Ax, r, lpart, tpart, loss, g, n_iter, eta, l1=0.0):
    """One guided sub-step of the 'ps' data term through a PSF whose weights are learnt, enqueued by one call
    (osm_ps_blind_optimize): n_iter x (A, loss / r, tap gradient, step of w), loss and g = A^T r those before the last step."""
    B, Cc, H, W, T = int(B), int(Cc), int(H), int(W), int(dy.shape[0])
    HW = H * W
    _check_tap_lists("ps_blind_optimize", dy, dx, w)
    need = dict(x0=B * Cc * HW, y=B * 3 * HW, Ax=B * 3 * HW, r=B * 3 * HW, lpart=B * phys_nblk(HW), tpart=B * tap_grad_nparts(3, H, W) * T,
                loss=B, g=B * Cc * HW)
    if mask is not None:
        need["mask"] = B * 3 * HW
    have = dict(x0=x0, y=y, Ax=Ax, r=r, lpart=lpart, tpart=tpart, loss=loss, g=g, mask=mask)
    for k, n in need.items():
        t = have[k]
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise _lib.OsmosisHipError(f"ps_blind_optimize: {k} must be contiguous fp32 with at least {n} elements, got {tuple(t.shape)} {t.dtype}")
    call("osm_ps_blind_optimize", ptr(x0), ptr(y), ptr(mask), ptr(dy), ptr(dx), ptr(w), T, int(Ry), int(Rx), B, Cc, H, W, ptr(Ax), ptr(r),
         ptr(lpart), ptr(tpart), ptr(loss), ptr(g), int(n_iter), float(eta), float(l1), _s(),
         keep=(x0, y, mask, dy, dx, w, Ax, r, lpart, tpart, loss, g))


# ----------------------------------------------------------------------------- PSF weight sets (include/osmosis_psfset.h)
def _check_weight_sets(name, dy, dx, w, B, P):
    """(nb, nc, T) of the weight sets w fp32 [nb,nc,T] beside the tap list dy, dx int32 [T]: nb in {1, B}, nc in {1, P}."""
    _check_tap_lists(name, dy, dx)
    T = int(dy.shape[0])
    if w.dtype != torch.float32 or not w.is_contiguous() or w.dim() != 3 or w.shape[2] != T or w.shape[0] not in (1, int(B)) \
            or w.shape[1] not in (1, int(P)):
        raise _lib.OsmosisHipError(f"{name}: the weight sets are contiguous fp32 [nb,nc,T = {T}] with nb in (1, {int(B)}) and nc in (1, {int(P)}), "
                                   f"got {tuple(w.shape)} {w.dtype}")
    return int(w.shape[0]), int(w.shape[1]), T


def psf_apply_s(x, out, dy, dx, w, Ry, Rx, B, P, x_img_stride, out_img_stride, H, W, adjoint=False, zero_planes=0):
    """`psf_apply` with weight sets w fp32 [nb,nc,T] (osm_psf_apply_s, include/osmosis_psfset.h): plane p of image b is blurred with
    set (nb > 1 ? b : 0, nc > 1 ? p : 0); nb in {1, B}, nc in {1, P}.  Everything else is `psf_apply`'s."""
    for t in (x, out):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_apply_s takes contiguous fp32 tensors")
    B, P, Z, H, W = int(B), int(P), int(zero_planes), int(H), int(W)
    nb, nc, T = _check_weight_sets("psf_apply_s", dy, dx, w, B, P)
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * H * W
                   or out.numel() < (B - 1) * int(out_img_stride) + (P + Z) * H * W):
        raise _lib.OsmosisHipError(f"psf_apply_s: x ({x.numel()} elements) / out ({out.numel()}) are smaller than {B} images of "
                                   f"{P} -> {P + Z} planes of {H} x {W} at strides {x_img_stride} / {out_img_stride}")
    call("osm_psf_apply_s", ptr(x), ptr(out), ptr(dy), ptr(dx), ptr(w), T, int(Ry), int(Rx), B, P, int(x_img_stride),
         int(out_img_stride), H, W, 1 if adjoint else 0, Z, nc * T if nb > 1 else 0, T if nc > 1 else 0, _s(), keep=(x, out, dy, dx, w))


def psf_tap_step_s(w, part, loss, B, P, ntiles, hw3, eta, l1=0.0, per_image=False, per_channel=False):
    """One projected step of every weight set of w fp32 [nb,nc,T], in place (osm_psf_tap_step_s): nb = B if per_image else 1,
    nc = P if per_channel else 1; set (bi, ci) takes `psf_tap_step`'s step from its own images and its own plane's partials of
    part [B][P ntiles][T], and is left untouched when its own sum is 0 or not finite."""
    for t in (w, part, loss):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_tap_step_s takes contiguous fp32 tensors")
    B, P, ntiles = int(B), int(P), int(ntiles)
    want = (B if per_image else 1, P if per_channel else 1)
    if w.dim() != 3 or tuple(w.shape[:2]) != want:
        raise _lib.OsmosisHipError(f"psf_tap_step_s: the weight sets are [nb,nc,T] = [{want[0]},{want[1]},T] for per_image={bool(per_image)}, "
                                   f"per_channel={bool(per_channel)} at B = {B}, P = {P}, got {tuple(w.shape)}")
    T = int(w.shape[2])
    if B >= 1 and (part.numel() < B * P * ntiles * T or loss.numel() < B):
        raise _lib.OsmosisHipError(f"psf_tap_step_s: part ({part.numel()} elements) / loss ({loss.numel()}) are smaller than "
                                   f"{B} x {P * ntiles} x {T} / {B}")
    call("osm_psf_tap_step_s", ptr(w), ptr(part), ptr(loss), B, P, ntiles, T, int(hw3), float(eta), float(l1), 1 if per_image else 0,
         1 if per_channel else 0, _s(), keep=(w, part, loss))


def ps_blind_optimize_s(x0, y, mask, dy, dx, w, Ry, Rx, B, Cc, H, W, Ax, r, lpart, tpart, loss, g, n_iter, eta, l1=0.0):
    """`ps_blind_optimize` with weight sets w fp32 [nb,nc,T], nb in {1, B}, nc in {1, 3} (osm_ps_blind_optimize_s): every set is
    stepped from its own images / planes; the flags are read off w's shape."""
    B, Cc, H, W = int(B), int(Cc), int(H), int(W)
    HW = H * W
    nb, nc, T = _check_weight_sets("ps_blind_optimize_s", dy, dx, w, B, 3)
    need = dict(x0=B * Cc * HW, y=B * 3 * HW, Ax=B * 3 * HW, r=B * 3 * HW, lpart=B * phys_nblk(HW), tpart=B * tap_grad_nparts(3, H, W) * T,
                loss=B, g=B * Cc * HW)
    if mask is not None:
        need["mask"] = B * 3 * HW
    have = dict(x0=x0, y=y, Ax=Ax, r=r, lpart=lpart, tpart=tpart, loss=loss, g=g, mask=mask)
    for k, n in need.items():
        t = have[k]
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < n:
            raise _lib.OsmosisHipError(f"ps_blind_optimize_s: {k} must be contiguous fp32 with at least {n} elements, got {tuple(t.shape)} {t.dtype}")
    call("osm_ps_blind_optimize_s", ptr(x0), ptr(y), ptr(mask), ptr(dy), ptr(dx), ptr(w), T, int(Ry), int(Rx), B, Cc, H, W, ptr(Ax), ptr(r),
         ptr(lpart), ptr(tpart), ptr(loss), ptr(g), int(n_iter), float(eta), float(l1), 1 if nb > 1 else 0, 1 if nc > 1 else 0, _s(),
         keep=(x0, y, mask, dy, dx, w, Ax, r, lpart, tpart, loss, g))


# ----------------------------------------------------------------------------- the water / haze data term through a linear operator
def lin_desc(operator, H, W, device) -> LinDesc:
    """The osm_lin_desc of a `measurements.GRID_OPERATORS` instance at the image grid H x W (include/osmosis_physlin.h).  The device
    tables / taps it points at are the operator's own cached tensors; they are also kept on the descriptor (`_keep`)."""
    from .guided_diffusion.measurements import BlindFieldOperator, PSFFieldOperator, PSFOperator, SeparableOperator
    if isinstance(operator, BlindFieldOperator):
        raise _lib.OsmosisHipError("lin_desc: 'blind_field_blur' carries a learnt field of point-spread functions; the composed water / "
                                   "haze data term takes one fixed point-spread function (osm_lin_desc has no such family)")
    if isinstance(operator, PSFFieldOperator):
        raise _lib.OsmosisHipError("lin_desc: 'field_blur' carries a field of point-spread functions; the composed water / haze data term "
                                   "takes one (osm_lin_desc has no such family)")
    d = LinDesc()
    h, w = operator.out_shape(H, W)
    d.H, d.W, d.h, d.w = int(H), int(W), int(h), int(w)
    if isinstance(operator, PSFOperator):
        if operator.weight_sets != (1, 1):
            raise _lib.OsmosisHipError(f"lin_desc: the operator carries weight sets {operator.weight_sets} (per_image / per_channel); the "
                                       "composed water / haze data term takes one point-spread function")
        dy, dx, tw = operator.taps(device)
        d.family, d.dy, d.dx, d.tap_w, d.T = 1, ptr(dy), ptr(dx), ptr(tw), int(tw.shape[0])
        d.Ry, d.Rx = operator.radius()
        d._keep = (dy, dx, tw)
    elif isinstance(operator, SeparableOperator):
        t = operator.tables(H, W, device)
        (sh, wh, sw, ww), (tsh, twh, tsw, tww) = t["fwd"], t["adj"]
        d.family = 0
        d.start_h, d.wt_h, d.start_w, d.wt_w, d.Kh, d.Kw = ptr(sh), ptr(wh), ptr(sw), ptr(ww), int(wh.shape[1]), int(ww.shape[1])
        d.tstart_h, d.twt_h, d.tstart_w, d.twt_w = ptr(tsh), ptr(twh), ptr(tsw), ptr(tww)
        d.tKh, d.tKw = int(twh.shape[1]), int(tww.shape[1])
        d._keep = t["fwd"] + t["adj"]
    else:
        raise _lib.OsmosisHipError(f"lin_desc: {type(operator).__name__} is neither a SeparableOperator nor a PSFOperator")
    return d


def phys_lin_planes(desc: PhysDesc) -> int:
    """Planes of the forward workspace F: the image, and the depth weight when the loss is weighted."""
    return 4 if desc.weight_type == 1 else 3


def _check_lin_ws(name, desc, hw, **ws):
    B, HW, P = desc.B, desc.HW, phys_lin_planes(desc)
    need = {"F": B * P * HW, "AF": B * P * hw, "u": B * 3 * hw, "v": B * 3 * HW, "part_r": B * phys_nblk(hw), "y": B * 3 * hw,
            "mask": B * 3 * hw, "part": B * phys_nblk(HW) * 16, "x0": B * 4 * HW, "g": B * 4 * HW, "phi": B * 9, "red": B * 16}
    for k, t in ws.items():
        if t is None:
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need[k] or (k in ("y", "mask") and t.numel() != need[k]):
            raise ValueError(f"{name}: `{k}` must be contiguous fp32 with {need[k]} elements, got {tuple(t.shape)} {t.dtype}")


def phys_forward(desc: PhysDesc, x0, phi, F):
    """F [B,P,HW] = the water / haze image I (and the depth weight, P = 4) of x0 at phi (osm_phys_forward)."""
    _check_lin_ws("phys_forward", desc, 1, x0=x0, phi=phi, F=F)
    call("osm_phys_forward", C.byref(desc), ptr(x0), ptr(phi), ptr(F), _s(), keep=(desc, x0, phi, F))


def phys_resid(desc: PhysDesc, hw, AF, y, mask, u, part_r):
    """u [B,3,hw] = d S / d (A I) and the partial sums of the squared residual on the measurement's grid (osm_phys_resid)."""
    _check_lin_ws("phys_resid", desc, hw, AF=AF, y=y, mask=mask, u=u, part_r=part_r)
    call("osm_phys_resid", C.byref(desc), int(hw), ptr(AF), ptr(y), ptr(mask), ptr(u), ptr(part_r), _s(),
         keep=(desc, AF, y, mask, u, part_r))


def phys_reduce_lin(desc: PhysDesc, x0, phi, v, part):
    _check_lin_ws("phys_reduce_lin", desc, 1, x0=x0, phi=phi, v=v, part=part)
    call("osm_phys_reduce_lin", C.byref(desc), ptr(x0), ptr(phi), ptr(v), ptr(part), _s(), keep=(desc, x0, phi, v, part))


def phys_finalize_lin(desc: PhysDesc, hw, part, part_r, red, phi, do_update, loss_out, opt_state=None, masked=False):
    _check_lin_ws("phys_finalize_lin", desc, hw, part=part, part_r=part_r, red=red, phi=phi)
    call("osm_phys_finalize_lin", C.byref(desc), int(hw), ptr(part), ptr(part_r), ptr(red), ptr(phi), int(do_update), ptr(loss_out),
         ptr(opt_state), int(bool(masked)), _s(), keep=(desc, part, part_r, red, phi, loss_out, opt_state))


def phys_grad_lin(desc: PhysDesc, hw, x0, phi, v, red, g, masked=False):
    _check_lin_ws("phys_grad_lin", desc, hw, x0=x0, phi=phi, v=v, red=red, g=g)
    call("osm_phys_grad_lin", C.byref(desc), int(hw), ptr(x0), ptr(phi), ptr(v), ptr(red), ptr(g), int(bool(masked)), _s(),
         keep=(desc, x0, phi, v, red, g))


def phys_lin_apply(lin: LinDesc, x, out, B, P, adjoint=False):
    """out [B,P,hw] = A x [B,P,HW], or with `adjoint` out [B,P,HW] = A^T x [B,P,hw]: the launch osm_phys_optimize_lin makes."""
    HW, hw = lin.H * lin.W, lin.h * lin.w
    n_in, n_out = (hw, HW) if adjoint else (HW, hw)
    keep = lin._keep
    if lin.family == 1:
        psf_apply(x, out, *keep, lin.Ry, lin.Rx, B, P, P * n_in, P * n_out, lin.H, lin.W, adjoint=adjoint)
    elif adjoint:
        linop_apply(x, out, *keep[4:], B, P, P * n_in, P * n_out, lin.h, lin.w)
    else:
        linop_apply(x, out, *keep[:4], B, P, P * n_in, P * n_out, lin.H, lin.W)


def phys_optimize_lin(desc: PhysDesc, lin: LinDesc, x0, y, mask, phi, F, AF, u, v, part_r, part, red, loss_out, g, n_inner: int,
                      freeze_phi: bool, opt_state=None):
    """The inner phi loop of a guided step with a linear operator between the image-formation model and the residual, enqueued by
    one call (osm_phys_optimize_lin): per iteration forward, A, resid, A^T, reduce_lin, finalize_lin."""
    if lin.H * lin.W != desc.HW:
        raise ValueError(f"phys_optimize_lin: the operator's image grid {lin.H} x {lin.W} does not have HW = {desc.HW} pixels")
    _check_lin_ws("phys_optimize_lin", desc, lin.h * lin.w, x0=x0, y=y, mask=mask, phi=phi, F=F, AF=AF, u=u, v=v, part_r=part_r,
                  part=part, red=red, g=g)
    call("osm_phys_optimize_lin", C.byref(desc), C.byref(lin), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(F), ptr(AF), ptr(u), ptr(v),
         ptr(part_r), ptr(part), ptr(red), ptr(loss_out), ptr(g), int(n_inner), int(bool(freeze_phi)), ptr(opt_state), _s(),
         keep=(desc, lin, x0, y, mask, phi, F, AF, u, v, part_r, part, red, loss_out, g, opt_state) + tuple(lin._keep))


# ----------------------------------------------------------------------------- shared water parameters (include/osmosis_physgroup.h)
def group_desc(group_sizes, reduce="mean") -> GroupDesc:
    """The group descriptor of a batch partitioned into contiguous groups of `group_sizes` images (a Python tuple: the offsets stay
    on the host and travel in the kernel's arguments, nothing is allocated on the device)."""
    return GroupDesc.of(group_sizes, reduce)


def _check_group(name, desc: PhysDesc, grp: GroupDesc):
    if grp.G < 1 or grp.off[grp.G] != desc.B:
        raise ValueError(f"{name}: the groups cover {grp.off[grp.G] if grp.G >= 1 else 0} images, the descriptor has B = {desc.B}")


def phys_finalize_g(desc: PhysDesc, grp: GroupDesc, part, red, phi, do_update, loss_out, opt_state=None, masked=False):
    """`phys_finalize_m` with ONE phi step per group: the members' gradients pooled (fp64, ascending order; sum or mean), every member
    row receives the new phi and optimizer state."""
    _check_group("phys_finalize_g", desc, grp)
    call("osm_phys_finalize_g", C.byref(desc), C.byref(grp), ptr(part), ptr(red), ptr(phi), int(do_update), ptr(loss_out), ptr(opt_state),
         int(bool(masked)), _s(), keep=(desc, grp, part, red, phi, loss_out, opt_state))


def phys_finalize_lin_g(desc: PhysDesc, grp: GroupDesc, hw, part, part_r, red, phi, do_update, loss_out, opt_state=None, masked=False):
    _check_group("phys_finalize_lin_g", desc, grp)
    _check_lin_ws("phys_finalize_lin_g", desc, hw, part=part, part_r=part_r, red=red, phi=phi)
    call("osm_phys_finalize_lin_g", C.byref(desc), C.byref(grp), int(hw), ptr(part), ptr(part_r), ptr(red), ptr(phi), int(do_update),
         ptr(loss_out), ptr(opt_state), int(bool(masked)), _s(), keep=(desc, grp, part, part_r, red, phi, loss_out, opt_state))


def phys_optimize_g(desc: PhysDesc, grp: GroupDesc, x0, y, mask, phi, part, red, loss_out, g, n_inner: int, freeze_phi: bool, opt_state=None):
    """`phys_optimize_m` (mask None: `phys_optimize`) with the grouped finalize in the place of the plain one."""
    _check_group("phys_optimize_g", desc, grp)
    _check_mask(mask, y)
    call("osm_phys_optimize_g", C.byref(desc), C.byref(grp), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(part), ptr(red), ptr(loss_out),
         ptr(g), int(n_inner), int(bool(freeze_phi)), ptr(opt_state), _s(),
         keep=(desc, grp, x0, y, mask, phi, part, red, loss_out, g, opt_state))


def phys_optimize_lin_g(desc: PhysDesc, grp: GroupDesc, lin: LinDesc, x0, y, mask, phi, F, AF, u, v, part_r, part, red, loss_out, g,
                        n_inner: int, freeze_phi: bool, opt_state=None):
    """`phys_optimize_lin` with the grouped finalize in the place of the plain one."""
    _check_group("phys_optimize_lin_g", desc, grp)
    if lin.H * lin.W != desc.HW:
        raise ValueError(f"phys_optimize_lin_g: the operator's image grid {lin.H} x {lin.W} does not have HW = {desc.HW} pixels")
    _check_lin_ws("phys_optimize_lin_g", desc, lin.h * lin.w, x0=x0, y=y, mask=mask, phi=phi, F=F, AF=AF, u=u, v=v, part_r=part_r,
                  part=part, red=red, g=g)
    call("osm_phys_optimize_lin_g", C.byref(desc), C.byref(grp), C.byref(lin), ptr(x0), ptr(y), ptr(mask), ptr(phi), ptr(F), ptr(AF),
         ptr(u), ptr(v), ptr(part_r), ptr(part), ptr(red), ptr(loss_out), ptr(g), int(n_inner), int(bool(freeze_phi)), ptr(opt_state), _s(),
         keep=(desc, grp, lin, x0, y, mask, phi, F, AF, u, v, part_r, part, red, loss_out, g, opt_state) + tuple(lin._keep))


# ----------------------------------------------------------------------------- range-map depth prior (include/osmosis_depthprior.h)
DEPTH_ALIGN = {"none": 0, "scale": 1, "affine": 2}
DEPTH_LOSS = {"norm": 0, "mse": 1}


def depth_nblk(HW: int) -> int:
    return query("osm_depth_nblk", int(HW))


def depth_desc(align, loss, weight, scale, scale_min, depth_type, dval, B, HW) -> DepthDesc:
    """The osm_depth_desc of a prior: align 'none' | 'scale' | 'affine', loss 'norm' | 'mse', weight = lambda; depth_type / dval: the
    operator's depth conversion (`PhysDesc.depth_type`, `.dval`)."""
    if align not in DEPTH_ALIGN:
        raise ValueError(f"depth prior: align must be one of {sorted(DEPTH_ALIGN)}, got {align!r}")
    if loss not in DEPTH_LOSS:
        raise ValueError(f"depth prior: loss must be one of {sorted(DEPTH_LOSS)}, got {loss!r}")
    d = DepthDesc()
    d.align, d.loss_type, d.lam, d.scale, d.scale_min = DEPTH_ALIGN[align], DEPTH_LOSS[loss], float(weight), float(scale), float(scale_min)
    d.depth_type = int(depth_type)
    for i in range(3):
        d.dval[i] = float(dval[i])
    d.B, d.HW = int(B), int(HW)
    return d


def _check_depth(name, desc: DepthDesc, **ts):
    B, HW = desc.B, desc.HW
    need = {"x0": B * 4 * HW, "g": B * 4 * HW, "z": B * HW, "m": B * HW, "depth_loss": B}
    need64 = {"part": B * depth_nblk(HW) * 8, "fit": B * 4}
    for k, t in ts.items():
        if k in need64:
            if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() < need64[k]:
                raise ValueError(f"{name}: `{k}` must be contiguous float64 with at least {need64[k]} elements, got {tuple(t.shape)} {t.dtype}")
        elif t.dtype != torch.float32 or not t.is_contiguous() or t.numel() < need[k] or (k in ("z", "m") and t.numel() != need[k]):
            raise ValueError(f"{name}: `{k}` must be contiguous fp32 with {need[k]} elements, got {tuple(t.shape)} {t.dtype}")


def depth_reduce(desc: DepthDesc, x0, z, m, part):
    """part (float64 [B][depth_nblk(HW)][8]) = the workgroup partials of the six moments of (m, z, d) (osm_depth_reduce)."""
    _check_depth("depth_reduce", desc, x0=x0, z=z, m=m, part=part)
    call("osm_depth_reduce", C.byref(desc), ptr(x0), ptr(z), ptr(m), ptr_f64(part), _s(), keep=(desc, x0, z, m, part))


def depth_fit(desc: DepthDesc, part, fit, depth_loss):
    """fit (float64 [B][4] = a, c, gs, L) and depth_loss (fp32 [B]) from the partials (osm_depth_fit)."""
    _check_depth("depth_fit", desc, part=part, fit=fit, depth_loss=depth_loss)
    call("osm_depth_fit", C.byref(desc), ptr_f64(part), ptr_f64(fit), ptr(depth_loss), _s(), keep=(desc, part, fit, depth_loss))


def depth_grad(desc: DepthDesc, x0, z, m, fit, g):
    """g[b,3,p] += (float)(gs m (d - (a z + c)) dd) where m > 0; nothing else of g [B,4,HW] is written (osm_depth_grad)."""
    _check_depth("depth_grad", desc, x0=x0, z=z, m=m, fit=fit, g=g)
    call("osm_depth_grad", C.byref(desc), ptr(x0), ptr(z), ptr(m), ptr_f64(fit), ptr(g), _s(), keep=(desc, x0, z, m, fit, g))


def depth_loss_grad(desc: DepthDesc, x0, z, m, part, fit, depth_loss, g):
    """The prior's three launches (reduce, fit, grad) enqueued by one call (osm_depth_loss_grad)."""
    _check_depth("depth_loss_grad", desc, x0=x0, z=z, m=m, part=part, fit=fit, depth_loss=depth_loss, g=g)
    call("osm_depth_loss_grad", C.byref(desc), ptr(x0), ptr(z), ptr(m), ptr_f64(part), ptr_f64(fit), ptr(depth_loss), ptr(g), _s(),
         keep=(desc, x0, z, m, part, fit, depth_loss, g))


# ----------------------------------------------------------------------------- robust data term (include/osmosis_robust.h)
ROBUST_LOSS = {"huber": 0, "tukey": 1, "cauchy": 2}
ROBUST_C = {"huber": 1.345, "tukey": 4.685, "cauchy": 2.385}      # 95 % efficiency at the normal (Holland & Welsch 1977)


def robust_desc(loss, c, scale, sigma_min, per_pixel, B, hw) -> RobustDesc:
    """The osm_robust_desc of a setting: loss 'huber' | 'tukey' | 'cauchy', c > 0 (None: the loss's default), scale 'mad' or a fixed
    sigma > 0, sigma_min >= 0, per_pixel."""
    if loss not in ROBUST_LOSS:
        raise ValueError(f"robust: loss must be one of {sorted(ROBUST_LOSS)}, got {loss!r}")
    c = ROBUST_C[loss] if c is None else float(c)
    if not (c > 0.0 and c < float("inf")):
        raise ValueError(f"robust: c must be finite and > 0, got {c}")
    sigma_min = float(sigma_min)
    if not (sigma_min >= 0.0 and sigma_min < float("inf")):
        raise ValueError(f"robust: sigma_min must be finite and >= 0, got {sigma_min}")
    d = RobustDesc()
    if isinstance(scale, str):
        if scale != "mad":
            raise ValueError(f"robust: scale must be 'mad' or a float > 0, got {scale!r}")
        d.scale_mode, d.scale = 0, 0.0
    else:
        scale = float(scale)
        if not (scale > 0.0 and scale < float("inf")):
            raise ValueError(f"robust: a fixed scale must be finite and > 0, got {scale}")
        d.scale_mode, d.scale = 1, scale
    d.loss, d.c, d.sigma_min, d.per_pixel, d.B, d.hw = ROBUST_LOSS[loss], c, sigma_min, int(bool(per_pixel)), int(B), int(hw)
    return d


def _check_robust(name, desc: RobustDesc, pred=None, **ts):
    B, hw = desc.B, desc.hw
    for k, t in ts.items():
        if t is None:
            continue
        if k == "n_valid":
            if t.dtype != torch.int32 or not t.is_contiguous() or t.numel() != B:
                raise ValueError(f"{name}: `n_valid` must be contiguous int32 [{B}], got {tuple(t.shape)} {t.dtype}")
            continue
        need = B if k == "sigma" else B * 3 * hw
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != need:
            raise ValueError(f"{name}: `{k}` must be contiguous fp32 with {need} elements, got {tuple(t.shape)} {t.dtype}")
    if pred is not None:
        if pred.dtype != torch.float32 or not pred.is_contiguous() or pred.dim() < 2 or pred.shape[0] != B or \
                pred.numel() // B < 3 * hw or (pred.numel() // B) % hw != 0:
            raise ValueError(f"{name}: `pred` must be contiguous fp32 [{B},P>=3,{hw}], got {tuple(pred.shape)} {pred.dtype}")
        return pred.numel() // B
    return None


def robust_resid(desc: RobustDesc, pred, pa, pb, y, e):
    """e [B,3,hw] = y - (pa pred + pb), unfused; pred [B,P>=3,hw]: its first three planes are read (osm_robust_resid)."""
    bs = _check_robust("robust_resid", desc, pred=pred, y=y, e=e)
    call("osm_robust_resid", C.byref(desc), ptr(pred), bs, float(pa), float(pb), ptr(y), ptr(e), _s(), keep=(desc, pred, y, e))


def robust_scale(desc: RobustDesc, e, M0, sigma, n_valid):
    """sigma [B] = max(1.4826 median |e|, sigma_min) over the entries with M0 > 0 (None: all) and e finite; n_valid [B] int32 their
    number (osm_robust_scale: an exact select, one workgroup per image)."""
    _check_robust("robust_scale", desc, e=e, M0=M0, sigma=sigma, n_valid=n_valid)
    call("osm_robust_scale", C.byref(desc), ptr(e), ptr(M0), ptr(sigma), ptr(n_valid), _s(), keep=(desc, e, M0, sigma, n_valid))


def robust_weights(desc: RobustDesc, e, M0, sigma, M_eff, omega=None):
    """M_eff [B,3,hw] = M0 sqrt(omega) (and omega) from e, M0 (None: ones) and sigma [B] (None with a fixed scale)
    (osm_robust_weights)."""
    _check_robust("robust_weights", desc, e=e, M0=M0, sigma=sigma, M_eff=M_eff, omega=omega)
    if sigma is None and desc.scale_mode != 1:
        raise ValueError("robust_weights: the mad scale reads `sigma`")
    call("osm_robust_weights", C.byref(desc), ptr(e), ptr(M0), ptr(sigma), ptr(M_eff), ptr(omega), _s(),
         keep=(desc, e, M0, sigma, M_eff, omega))


def robust_mask(desc: RobustDesc, pred, pa, pb, y, M0, e, sigma, n_valid, M_eff, omega=None):
    """The launches of the robust weights from one call (osm_robust_mask): resid, scale (the mad scale only), weights."""
    bs = _check_robust("robust_mask", desc, pred=pred, y=y, M0=M0, e=e, sigma=sigma, n_valid=n_valid, M_eff=M_eff, omega=omega)
    if (sigma is None or n_valid is None) and desc.scale_mode != 1:
        raise ValueError("robust_mask: the mad scale writes `sigma` and `n_valid`")
    call("osm_robust_mask", C.byref(desc), ptr(pred), bs, float(pa), float(pb), ptr(y), ptr(M0), ptr(e), ptr(sigma), ptr(n_valid),
         ptr(M_eff), ptr(omega), _s(), keep=(desc, pred, y, M0, e, sigma, n_valid, M_eff, omega))


# ----------------------------------------------------------------------------- learnt vignetting gain field (include/osmosis_gain.h)
GAIN_MAX_GRID = 32
_gain_tables = {}       # (H, W, gh, gw, device) -> (iy0, fy, ix0, fx) on the device


def gain_tables_host(H, W, gh, gw):
    """The interpolation tables of include/osmosis_gain.h on the host: (iy0 [H] int32, fy [H] fp32, ix0 [W] int32, fx [W] fp32), the
    positions j (n - 1) / (g - 1) in float64, the fractions rounded to fp32."""
    import numpy as np

    def axis(n, g):
        pos = np.arange(n, dtype=np.float64) * (g - 1) / (n - 1)
        i0 = np.minimum(np.floor(pos), g - 2).astype(np.int32)
        return i0, (pos - i0).astype(np.float32)
    iy0, fy = axis(int(H), int(gh))
    ix0, fx = axis(int(W), int(gw))
    return iy0, fy, ix0, fx


def gain_tables(H, W, gh, gw, device):
    """`gain_tables_host` as device tensors, cached per (H, W, gh, gw, device)."""
    key = (int(H), int(W), int(gh), int(gw), str(device))
    tabs = _gain_tables.get(key)
    if tabs is None:
        while len(_gain_tables) >= 16:
            _gain_tables.pop(next(iter(_gain_tables)))
        tabs = _gain_tables[key] = tuple(torch.from_numpy(a).to(device) for a in gain_tables_host(H, W, gh, gw))
    return tabs


# ----------------------------------------------------------------------------- a field of PSFs (include/osmosis_psffield.h)
def field_tables(H, W, gh, gw, device):
    """The interpolation tables (iy0, fy, ix0, fx) of a gh x gw node grid on an H x W image as device tensors: the gain field's
    (`gain_tables`: same nodes, same cache), after the limits 2 <= gh <= min(H, 32), 2 <= gw <= min(W, 32)."""
    H, W, gh, gw = int(H), int(W), int(gh), int(gw)
    if not (2 <= gh <= min(H, GAIN_MAX_GRID) and 2 <= gw <= min(W, GAIN_MAX_GRID)):
        raise ValueError(f"field_tables: the node grid must be within 2 .. min({GAIN_MAX_GRID}, the image side) per axis, got {gh} x {gw} "
                         f"on a {H} x {W} image")
    return gain_tables(H, W, gh, gw, device)


def psf_field_apply(x, out, dy, dx, w, tabs, Ry, Rx, B, P, x_img_stride, out_img_stride, H, W, adjoint=False, zero_planes=0):
    """The blur of planes p < P with a FIELD of point-spread functions (osm_psf_field_apply,
    include/osmosis_psffield.h): w fp32 [gh,gw,T] holds one PSF per node over the shared tap list dy, dx int32 [T], the nodes sit
    on the image corners inclusive and every pixel is blurred with the bilinear interpolation of its cell's four corner PSFs; with
    `adjoint` the exact transpose.  tabs = `field_tables(H, W, gh, gw, device)`.  Everything else is `psf_apply`'s."""
    for t in (x, out, w):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("psf_field_apply takes contiguous fp32 tensors")
    _check_tap_lists("psf_field_apply", dy, dx)
    T = int(dy.shape[0])
    if w.dim() != 3 or w.shape[2] != T:
        raise _lib.OsmosisHipError(f"psf_field_apply: the node weights are fp32 [gh,gw,T = {T}], got {tuple(w.shape)}")
    gh, gw = int(w.shape[0]), int(w.shape[1])
    B, P, Z, H, W = int(B), int(P), int(zero_planes), int(H), int(W)
    iy0, fy, ix0, fx = tabs
    for k, t, n, dt in (("iy0", iy0, H, torch.int32), ("fy", fy, H, torch.float32), ("ix0", ix0, W, torch.int32), ("fx", fx, W, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise _lib.OsmosisHipError(f"psf_field_apply: table `{k}` must be contiguous {dt} [{n}], got {tuple(t.shape)} {t.dtype}")
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * H * W
                   or out.numel() < (B - 1) * int(out_img_stride) + (P + Z) * H * W):
        raise _lib.OsmosisHipError(f"psf_field_apply: x ({x.numel()} elements) / out ({out.numel()}) are smaller than {B} images of "
                                   f"{P} -> {P + Z} planes of {H} x {W} at strides {x_img_stride} / {out_img_stride}")
    call("osm_psf_field_apply", ptr(x), ptr(out), ptr(dy), ptr(dx), ptr(w), T, int(Ry), int(Rx), gh, gw, ptr(iy0), ptr(fy), ptr(ix0),
         ptr(fx), B, P, int(x_img_stride), int(out_img_stride), H, W, 1 if adjoint else 0, Z, _s(),
         keep=(x, out, dy, dx, w, iy0, fy, ix0, fx))


# ----------------------------------------------------------------------------- learning a field of PSFs (include/osmosis_blindfield.h)
_field_layouts = {}     # (H, W, gh, gw, P, device) -> (lay on the device, partials per image, lay on the host)


def field_tap_layout(H, W, gh, gw, P=3, device=None):
    """The compact layout of the per-node tap partials (osm_field_tap_layout, host only): returns
    (lay, NP, host) -- `lay` int32 [2 gh + 2 gw + gh gw + 1] = ty0[gh], ty1[gh], tx0[gw], tx1[gw], off[gh gw + 1] (the 32 x 32 tile
    rows / columns every node row / column reaches and the nodes' offsets in partials per image), on `device` when one is given
    (cached), else None; NP = off[-1] partials of T floats per image; `host` the same array as numpy."""
    import ctypes as C
    import numpy as np
    H, W, gh, gw, P = int(H), int(W), int(gh), int(gw), int(P)
    key = (H, W, gh, gw, P, str(device))
    hit = _field_layouts.get(key)
    if hit is not None:
        return hit
    iy0, _, ix0, _ = gain_tables_host(H, W, gh, gw) if 2 <= gh <= H and 2 <= gw <= W else (np.zeros(1, np.int32),) * 4
    lay = np.zeros(2 * gh + 2 * gw + gh * gw + 1 if gh > 0 and gw > 0 else 1, dtype=np.int32)
    n = _lib.query("osm_field_tap_layout", gh, gw, iy0.ctypes.data_as(C.c_void_p), ix0.ctypes.data_as(C.c_void_p), H, W, P, 1, 1,
                   lay.ctypes.data_as(C.c_void_p))
    if n < 0:
        raise _lib.OsmosisHipError(f"osm_field_tap_layout failed ({n}): {_lib.last_error('osm_field_tap_layout')}")
    while len(_field_layouts) >= 16:
        _field_layouts.pop(next(iter(_field_layouts)))
    out = _field_layouts[key] = (None if device is None else torch.from_numpy(lay).to(device), int(n), lay)
    return out


def _check_field_lay(name, lay, gh, gw):
    if lay.dtype != torch.int32 or not lay.is_contiguous() or lay.numel() != 2 * gh + 2 * gw + gh * gw + 1:
        raise _lib.OsmosisHipError(f"{name}: the layout is int32 [{2 * gh + 2 * gw + gh * gw + 1}] (`field_tap_layout`), got "
                                   f"{tuple(lay.shape)} {lay.dtype}")


def field_tap_grad(x, r, dy, dx, tabs, lay, NP, gh, gw, Ry, Rx, B, P, x_img_stride, r_img_stride, H, W, part):
    """The per-node tile partials of c_n[b][t] = sum_p sum_ij hat_n(i,j) r[b,p,i,j] x[b,p,refl(i+dy[t]),refl(j+dx[t])]
    (osm_field_tap_grad): the tap gradient of the field operator `psf_field_apply`, in the compact layout of
    `field_tap_layout(H, W, gh, gw, P, device)` = (lay, NP, _); part fp32 with at least B NP T elements, every one written.
    tabs = `field_tables(H, W, gh, gw, device)`.  Deterministic (gather form, no atomics)."""
    for t in (x, r, part):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("field_tap_grad takes contiguous fp32 tensors")
    _check_tap_lists("field_tap_grad", dy, dx)
    B, P, H, W, T, gh, gw, NP = int(B), int(P), int(H), int(W), int(dy.shape[0]), int(gh), int(gw), int(NP)
    _check_field_lay("field_tap_grad", lay, gh, gw)
    iy0, fy, ix0, fx = tabs
    for k, t, n, dt in (("iy0", iy0, H, torch.int32), ("fy", fy, H, torch.float32), ("ix0", ix0, W, torch.int32), ("fx", fx, W, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise _lib.OsmosisHipError(f"field_tap_grad: table `{k}` must be contiguous {dt} [{n}], got {tuple(t.shape)} {t.dtype}")
    if NP != field_tap_layout(H, W, gh, gw, P)[1]:
        raise _lib.OsmosisHipError(f"field_tap_grad: NP {NP} is not the layout's partial count for {P} x {H} x {W} under {gh} x {gw} nodes")
    if B >= 1 and (x.numel() < (B - 1) * int(x_img_stride) + P * H * W or r.numel() < (B - 1) * int(r_img_stride) + P * H * W
                   or part.numel() < B * NP * T):
        raise _lib.OsmosisHipError(f"field_tap_grad: x ({x.numel()} elements) / r ({r.numel()}) / part ({part.numel()}) are smaller than "
                                   f"{B} images of {P} x {H} x {W} at strides {x_img_stride} / {r_img_stride} with {NP} partials of {T} taps")
    call("osm_field_tap_grad", ptr(x), ptr(r), ptr(dy), ptr(dx), T, int(Ry), int(Rx), gh, gw, ptr(iy0), ptr(fy), ptr(ix0), ptr(fx),
         ptr(lay), B, P, int(x_img_stride), int(r_img_stride), H, W, ptr(part), _s(), keep=(x, r, dy, dx, iy0, fy, ix0, fx, lay, part))


def field_tap_step(w, w_new, part, loss, lay, NP, B, hw3, eta, l1=0.0, smooth=0.0):
    """One projected step of every node of the field w fp32 [gh,gw,T], in place (osm_field_tap_step): per node `psf_tap_step`'s fp64
    arithmetic on that node's partials, plus eta smooth times the 4-neighbour Laplacian of the field; w_new fp32 [gh,gw,T] is the
    workspace the kernel writes (nodes read their neighbours while they step) before w_new is copied over w on the same stream."""
    for t in (w, w_new, part, loss):
        if t.dtype != torch.float32 or not t.is_contiguous():
            raise _lib.OsmosisHipError("field_tap_step takes contiguous fp32 tensors")
    if w.dim() != 3 or w_new.shape != w.shape:
        raise _lib.OsmosisHipError(f"field_tap_step: w and w_new are fp32 [gh,gw,T], got {tuple(w.shape)} and {tuple(w_new.shape)}")
    gh, gw, T = (int(v) for v in w.shape)
    _check_field_lay("field_tap_step", lay, gh, gw)
    B, NP = int(B), int(NP)
    if B >= 1 and (part.numel() < B * NP * T or loss.numel() < B):
        raise _lib.OsmosisHipError(f"field_tap_step: part ({part.numel()} elements) / loss ({loss.numel()}) are smaller than {B} x {NP} x {T} / {B}")
    call("osm_field_tap_step", ptr(w), ptr(w_new), ptr(part), ptr(loss), ptr(lay), gh, gw, B, T, int(hw3), float(eta), float(l1),
         float(smooth), _s(), keep=(w, w_new, part, loss, lay))


def gain_check(grid, eta, n_iter, smooth, g_min, H=None, W=None):
    """The host-side range checks of a gain-field setting; returns (gh, gw, eta, n_iter, smooth, g_min)."""
    try:
        gh, gw = (int(v) for v in grid)
        ok = (gh, gw) == tuple(grid)
    except (TypeError, ValueError):
        ok = False
    if not ok:
        raise ValueError(f"gain_field: grid must be a pair of ints (gh, gw), got {grid!r}")
    if not (2 <= gh <= GAIN_MAX_GRID and 2 <= gw <= GAIN_MAX_GRID):
        raise ValueError(f"gain_field: grid must be within 2 .. {GAIN_MAX_GRID} per side, got {gh} x {gw}")
    if H is not None and (gh > H or gw > W):
        raise ValueError(f"gain_field: grid {gh} x {gw} has more nodes than the image has pixels ({H} x {W})")
    eta, smooth, g_min = float(eta), float(smooth), float(g_min)
    if not (eta >= 0.0 and eta < float("inf")):
        raise ValueError(f"gain_field: eta must be finite and >= 0, got {eta}")
    if not (smooth >= 0.0 and smooth < float("inf")):
        raise ValueError(f"gain_field: smooth must be finite and >= 0, got {smooth}")
    if not (g_min > 0.0 and g_min <= 1.0):
        raise ValueError(f"gain_field: g_min must be in (0, 1], got {g_min}")
    if int(n_iter) != n_iter or not 1 <= int(n_iter) <= 1024:
        raise ValueError(f"gain_field: n_iter must be an int in [1, 1024], got {n_iter!r}")
    return gh, gw, eta, int(n_iter), smooth, g_min


def gain_desc(grid, eta, n_iter, smooth, g_min, learn, loss_type, P, B, H, W) -> GainDesc:
    """The osm_gain_desc of a setting on a [B,*,H,W] batch: loss_type 0 norm / 1 mse, P the planes of F (3, or 4 with the depth
    weight)."""
    gh, gw, eta, n_iter, smooth, g_min = gain_check(grid, eta, n_iter, smooth, g_min, H, W)
    d = GainDesc()
    d.B, d.H, d.W, d.gh, d.gw, d.P, d.loss_type = int(B), int(H), int(W), gh, gw, int(P), int(loss_type)
    d.eta, d.g_min, d.n_iter, d.learn = eta, g_min, n_iter, int(bool(learn))
    setattr(d, "lambda", smooth)
    return d


def gain_workspace(desc: GainDesc, device):
    """(t [B,H,gw] fp32, s [B,H] fp32, cs [B, gh gw + 1] float64) of a learning sub-step."""
    return (torch.empty(desc.B, desc.H, desc.gw, device=device, dtype=torch.float32),
            torch.empty(desc.B, desc.H, device=device, dtype=torch.float32),
            torch.empty(desc.B, desc.gh * desc.gw + 1, device=device, dtype=torch.float64))


def _check_gain(name, desc: GainDesc, tabs, **ts):
    B, HW, ng = desc.B, desc.H * desc.W, desc.gh * desc.gw
    need = {"nodes": B * ng, "y": B * 3 * HW, "M0": B * 3 * HW, "y_eff": B * 3 * HW, "m_eff": B * 3 * HW, "field": B * HW,
            "F": B * desc.P * HW, "t": B * desc.H * desc.gw, "s": B * desc.H}
    for k, t in ts.items():
        if t is None:
            continue
        if k == "cs":
            if t.dtype != torch.float64 or not t.is_contiguous() or t.numel() != B * (ng + 1):
                raise ValueError(f"{name}: `cs` must be contiguous float64 with {B * (ng + 1)} elements, got {tuple(t.shape)} {t.dtype}")
            continue
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != need[k]:
            raise ValueError(f"{name}: `{k}` must be contiguous fp32 with {need[k]} elements, got {tuple(t.shape)} {t.dtype}")
    iy0, fy, ix0, fx = tabs
    for k, t, n, dt in (("iy0", iy0, desc.H, torch.int32), ("fy", fy, desc.H, torch.float32), ("ix0", ix0, desc.W, torch.int32),
                        ("fx", fx, desc.W, torch.float32)):
        if t.dtype != dt or not t.is_contiguous() or t.numel() != n:
            raise ValueError(f"{name}: table `{k}` must be contiguous {dt} [{n}], got {tuple(t.shape)} {t.dtype}")


def gain_expand(desc: GainDesc, tabs, nodes, y, M0, y_eff, m_eff, field):
    """y_eff = (y + 1) / G - 1, m_eff = M0 G (M0 None: ones) and field = G from the nodes [B,gh,gw] (osm_gain_expand)."""
    _check_gain("gain_expand", desc, tabs, nodes=nodes, y=y, M0=M0, y_eff=y_eff, m_eff=m_eff, field=field)
    iy0, fy, ix0, fx = tabs
    call("osm_gain_expand", C.byref(desc), ptr(iy0), ptr(fy), ptr(ix0), ptr(fx), ptr(nodes), ptr(y), ptr(M0), ptr(y_eff), ptr(m_eff),
         ptr(field), _s(), keep=(desc, tabs, nodes, y, M0, y_eff, m_eff, field))


def gain_rows(desc: GainDesc, tabs, nodes, F, y, M0, t, s):
    """t [B,H,gw] and s [B,H]: the node gradient's row sums and the rows' sums of r^2 at the nodes, on F [B,P,HW] (osm_gain_rows)."""
    _check_gain("gain_rows", desc, tabs, nodes=nodes, F=F, y=y, M0=M0, t=t, s=s)
    iy0, fy, ix0, fx = tabs
    call("osm_gain_rows", C.byref(desc), ptr(iy0), ptr(fy), ptr(ix0), ptr(fx), ptr(nodes), ptr(F), ptr(y), ptr(M0), ptr(t), ptr(s), _s(),
         keep=(desc, tabs, nodes, F, y, M0, t, s))


def gain_step(desc: GainDesc, tabs, t, s, nodes, cs):
    """cs [B, gh gw + 1] float64 = (c_raw, S) from t and s, then the projected step on the nodes in place (osm_gain_step)."""
    _check_gain("gain_step", desc, tabs, t=t, s=s, nodes=nodes, cs=cs)
    iy0, fy, _, _ = tabs
    call("osm_gain_step", C.byref(desc), ptr(iy0), ptr(fy), ptr(t), ptr(s), ptr(nodes), ptr_f64(cs), _s(), keep=(desc, tabs, t, s, nodes, cs))


def gain_prepare(desc: GainDesc, tabs, F, y, M0, nodes, t, s, cs, y_eff, m_eff, field, freeze_phi=False):
    """The sub-step's launches from one call (osm_gain_prepare): n_iter x (rows, step), then the expand; freeze_phi or a desc with
    learn = 0: the expand alone (F, t, s, cs may then be None)."""
    _check_gain("gain_prepare", desc, tabs, F=F, y=y, M0=M0, nodes=nodes, t=t, s=s, cs=cs, y_eff=y_eff, m_eff=m_eff, field=field)
    if desc.learn == 1 and not freeze_phi and any(v is None for v in (F, t, s, cs)):
        raise ValueError("gain_prepare: a learning sub-step needs F, t, s and cs")
    iy0, fy, ix0, fx = tabs
    call("osm_gain_prepare", C.byref(desc), ptr(iy0), ptr(fy), ptr(ix0), ptr(fx), ptr(F), ptr(y), ptr(M0), ptr(nodes), ptr(t), ptr(s),
         ptr_f64(cs), ptr(y_eff), ptr(m_eff), ptr(field), int(bool(freeze_phi)), _s(),
         keep=(desc, tabs, F, y, M0, nodes, t, s, cs, y_eff, m_eff, field))
