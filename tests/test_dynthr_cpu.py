"""The oracle's `process_xstart` with dynamic_threshold (util/img_utils.py:8-15: clip(x * quantile(|x|, 0.98), -1, 1) over the whole
tensor) reproduces the REAL reference's forward and VJP vectors of tests/golden/loop_dynthr.npz (tools/gen_dynthr_golden.py)."""
import os

import numpy as np
import pytest
import torch

from oracle import diffusion_ref as D

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.mark.parametrize("tag", ["free", "ties"])
def test_oracle_dynamic_threshold_matches_the_reference_vectors(tag):
    g = np.load(os.path.join(GOLD, "loop_dynthr.npz"))
    x = torch.from_numpy(g[f"px.{tag}.x"]).requires_grad_(True)
    y = D.process_xstart(x, clip_denoised=False, dynamic_threshold=True)
    assert torch.equal(y.detach(), torch.from_numpy(g[f"px.{tag}.y"]))
    assert torch.equal(torch.quantile(x.detach().abs(), 0.98).reshape(1), torch.from_numpy(g[f"px.{tag}.q"]))
    (dx,) = torch.autograd.grad((y * torch.from_numpy(g[f"px.{tag}.w"])).sum(), x)
    want = torch.from_numpy(g[f"px.{tag}.dx"])
    assert float((dx - want).abs().max()) <= 1e-6 * float(want.abs().max())      # (S is a reduction: its order may vary by CPU)
    # with clip_denoised on as well, the second clamp changes nothing
    assert torch.equal(D.process_xstart(x.detach(), clip_denoised=True, dynamic_threshold=True), y.detach())


def test_chain_fixture_records_an_active_threshold():
    g = np.load(os.path.join(GOLD, "loop_dynthr.npz"))
    for tag in ("osmosis.clip0", "osmosis.clip1"):
        assert g[f"{tag}.q"].shape == (10,) and (g[f"{tag}.q"] > 1.0).all()      # the reference MULTIPLIES by q (> 1 here)
        assert np.abs(g[f"{tag}.x0"]).max() == 1.0
    assert np.array_equal(g["osmosis.clip0.x0"], g["osmosis.clip1.x0"])            # clip_denoised after the threshold: no-op
