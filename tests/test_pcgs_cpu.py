"""The PCGS schedule (`pcgs_schedule`: guidance flag, freeze_phi and alternate length per index) vs the REAL reference's decisions
recorded in tests/golden/loop_pcgs.npz (tools/gen_pcgs_golden.py), and the fixture's own bookkeeping."""
import os

import numpy as np
import pytest

from osmosis_diffusion_code_amd.guided_diffusion import gaussian_diffusion as gd

GOLD = os.path.join(os.path.dirname(__file__), "golden")


@pytest.fixture(scope="module")
def g():
    return np.load(os.path.join(GOLD, "loop_pcgs.npz"))


def as_pattern(row):
    us, ue, ss, se, lm, sg, tg, orig = (float(v) for v in row)
    return dict(pattern="original" if orig else "pcgs", update_start=us, update_end=ue, s_start=ss, s_end=se, local_M=int(lm),
                global_N=1, n_iter=1, start_guidance=sg, stop_guidance=tg)


def pattern(s_start, s_end, local_M):
    return dict(pattern="pcgs", update_start=0.7, update_end=0, global_N=1, local_M=local_M, s_start=s_start, s_end=s_end, n_iter=20,
                start_guidance=1, stop_guidance=0)


@pytest.mark.parametrize("T", [10, 1000])
def test_schedule_matches_the_reference(g, T):
    want, calls = g[f"sched.T{T}"], g[f"sched.calls.T{T}"]
    for p, row in enumerate(g["sched.pat"]):
        got = np.array(gd.pcgs_schedule(as_pattern(row), T), dtype=np.int8)
        assert got.shape == (T, 3)
        assert np.array_equal(got, want[p]), (row, np.argwhere(got != want[p])[:5])
        # the reference calls the conditioner alternate_len times at a guided index, never at an unguided one
        assert np.array_equal(got[:, 0] * got[:, 2], calls[p]), row


def test_schedule_raises_where_the_reference_asserts(g):
    assert len(g["sched.bad"]) > 0
    for row in g["sched.bad"]:
        with pytest.raises(AssertionError):
            gd.pcgs_schedule(as_pattern(row), 10)
    for row in g["sched.ok"]:                      # an s window outside the update window is accepted at local_M = 1
        assert all(a == 1 for _, _, a in gd.pcgs_schedule(as_pattern(row), 10))


def test_schedule_without_a_pattern_is_one_guided_step_per_index():
    assert gd.pcgs_schedule(None, 7) == [(True, False, 1)] * 7
    assert gd.pcgs_schedule(dict(pattern="original", local_M=4), 7) == [(True, False, 1)] * 7


def test_fixture_counts_one_call_and_one_draw_per_sub_step(g):
    for tag, pat in (("osm.revised.w62", pattern(0.6, 0.2, 3)), ("osm.revised.w50", pattern(0.5, 0.0, 3)),
                     ("osm.haze.w62", pattern(0.6, 0.2, 3)), ("ps.ddpm", pattern(0.5, 0.0, 2)), ("ps.ddim", pattern(0.5, 0.0, 2))):
        n = sum(a for _, _, a in gd.pcgs_schedule(pat, 10))
        assert n > 10, tag
        assert len(g[f"{tag}.loss"]) == n, tag
        assert len(g[f"{tag}.noise" if tag.startswith("osm") else f"{tag}.draws_x"]) == n, tag
        if tag.startswith("osm"):
            assert len(g[f"{tag}.x0_s2"]) == len(g[f"{tag}.grad_s2"]) == n, tag
            assert all(len(g[k]) == n for k in g.files if k.startswith(f"{tag}.phi.")), tag
    assert sum(a for _, _, a in gd.pcgs_schedule(pattern(0.6, 0.2, 3), 10)) == 20
    assert sum(a for _, _, a in gd.pcgs_schedule(pattern(0.5, 0.0, 3), 10)) == 22
