"""tests/attn_reference.py against independent statements of the same thing (CPU only): a direct softmax / einsum autograd
statement per head in double, the oracle's attention_block in fp32, and a cap on what `reference` loses when it is evaluated in
fp32 -- the figure `e32` that scales the run-time bars of the stress operands in tests/test_attention_gpu.py."""
import math

import pytest
import torch

import attn_reference as R
from oracle import unet_ref as U

F64 = torch.float64


@pytest.mark.parametrize("kind", ["legacy", "new", "rev", "padded"])
@pytest.mark.parametrize("gen", ["randn", "peaked"])
def test_reference_equals_a_direct_autograd_statement(kind, gen):
    B, T, heads, ch = 2, 96, 3, 64
    offs, hs, width = R.layout(kind, heads, ch)
    scale = 1.0 / math.sqrt(ch)
    qkv = R.make_qkv(gen, B, T, heads, ch, offs, hs, width, seed=3)
    dout = R.make_dout(B, T, heads * ch, seed=3)
    out, lse, delta, dqkv = R.reference(qkv, dout, heads, ch, offs, hs, scale, F64)
    assert out.dtype == lse.dtype == delta.dtype == dqkv.dtype == F64
    assert out.shape == (B, T, heads * ch) and lse.shape == delta.shape == (B, heads, T) and dqkv.shape == (B, T, width)
    x = qkv.double().requires_grad_(True)
    loss = 0.0
    for b in range(B):
        for h in range(heads):
            q = x[b, :, offs[0] + h * hs: offs[0] + h * hs + ch]
            k = x[b, :, offs[1] + h * hs: offs[1] + h * hs + ch]
            v = x[b, :, offs[2] + h * hs: offs[2] + h * hs + ch]
            s = (q @ k.t()) / math.sqrt(ch)
            o = torch.softmax(s, dim=-1) @ v
            g = dout[b, :, h * ch:(h + 1) * ch].double()
            sd, od = s.detach(), o.detach()
            assert float((od - out[b, :, h * ch:(h + 1) * ch]).abs().max()) <= 1e-12
            assert float((torch.log(torch.exp(sd - sd.max()).sum(-1)) + sd.max() - lse[b, h]).abs().max()) <= 1e-12
            assert float(((od * g).sum(-1) - delta[b, h]).abs().max()) <= 1e-12
            loss = loss + (o * g).sum()
    (dx,) = torch.autograd.grad(loss, x)
    assert float((dx - dqkv).abs().max()) <= 1e-12 * max(1.0, float(dx.abs().max()))
    used = torch.zeros(width, dtype=torch.bool)
    for c in range(3):
        for h in range(heads):
            used[R.head_cols(offs, hs, ch, c, h)] = True
    assert int(used.sum()) == 3 * heads * ch                         # the head blocks do not overlap
    assert float(dqkv[:, :, ~used].abs().sum()) == 0.0               # columns of no head get no gradient


@pytest.mark.parametrize("new_order", [False, True])
def test_block_statement_equals_the_oracle_in_fp32(new_order):
    """reference + the 1x1 convolutions + GroupNorm32 is the oracle's attention_block (which the rest of the suite trusts)"""
    B, heads, C, H, W = 2, 2, 128, 8, 8
    sd = R.block_state_dict(C, 11)
    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, C, H, W, generator=g) * 1.5 + 0.3
    dy = torch.randn(B, C, H, W, generator=g)
    want = U.attention_block(sd, "", x, heads, new_order)
    y32, _ = R.block(sd, x, heads, new_order, dtype=torch.float32)
    assert float((y32 - want).abs().max()) <= 1e-5 * float(want.abs().max())
    y64, dx64 = R.block(sd, x, heads, new_order, dy=dy, dtype=F64)
    assert float((y64 - want).abs().max()) <= 1e-5 * float(want.abs().max())
    xg = x.clone().requires_grad_(True)                              # the hand-chained backward against the oracle's autograd
    (dxo,) = torch.autograd.grad(U.attention_block(sd, "", xg, heads, new_order), xg, dy)
    assert float((dx64 - dxo).abs().max()) <= 1e-5 * float(dxo.abs().max())


@pytest.mark.parametrize("T", [64, 384, 1536])
@pytest.mark.parametrize("gen", R.GENERATORS)
def test_fp32_evaluation_of_the_reference_stays_under_its_cap(gen, T):
    """e32 <= 1e-5 for out and dqkv (block_err) and <= 4e-5 absolute for lse: the run-time bars max(project bar, 8 * e32) stay
    meaningful.  If a generator breaks the cap, the generator changes, not the cap.  Worst on the CPU: 7.5e-6 (`peaked`,
    gradient, T = 1536), 2.2e-5 (`peaked`, lse, T = 1536)."""
    c = R.case(gen, 1, T, 2, 64, "legacy", want_e32=True)
    print(f"{gen} T={T}: e32 out {c.e32['out']:.2e} dqkv {c.e32['dqkv']:.2e} lse {c.e32['lse']:.2e} delta {c.e32['delta']:.2e}")
    assert c.e32["out"] <= 1e-5 and c.e32["dqkv"] <= 1e-5 and c.e32["delta"] <= 1e-5
    assert c.e32["lse"] <= 4e-5


def test_block_err_and_views():
    c = R.case("randn", 2, 64, 2, 16, "padded")
    assert R.block_err(c.ref.dqkv, c.ref.dqkv, 2, 16, 3, c.offs, c.hs) == 0.0
    bad = c.ref.dqkv.clone()
    sl = R.head_cols(c.offs, c.hs, 16, 1, 1)
    bad[1, 5, sl.start + 3] += 0.5 * float(c.ref.dqkv[1, :, sl].abs().max())        # half of ITS block's max-abs, wherever others are
    assert abs(R.block_err(bad, c.ref.dqkv, 2, 16, 3, c.offs, c.hs) - 0.5) < 1e-12
    bad[0, 0, sl.start] = float("nan")
    assert R.block_err(bad, c.ref.dqkv, 2, 16, 3, c.offs, c.hs) == float("inf")
    v = R.Views(c, "cpu")
    lds = [b.buf.shape[1] for b in (v.qkv, v.dqkv, v.out, v.dout, v.o)]
    assert lds == [c.width + 32, c.width + 64, c.C + 16, c.C + 48, c.C + 80] and len(set(lds)) == 5
    for b in (v.qkv, v.dqkv, v.out, v.dout, v.o):
        assert b.c0 % 4 == 0 and b.view.data_ptr() % 16 == 0 and b.view.stride(1) == 1
    assert torch.equal(v.qkv.view, c.qkv.reshape(-1, c.width)) and bool(torch.isnan(v.out.view).all())
    v.copy_out_for_backward()
    assert v.inputs_unchanged() and v.outputs_guarded()
    v.out.buf[0, 0] = 1.0
    v.qkv.view[3, 3] += 1.0
    assert not v.outputs_guarded() and not v.inputs_unchanged()
