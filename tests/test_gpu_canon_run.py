"""GPU: Fast64::canonical_run (bft_fast64.h) -- a run of canonical heights applied at once, one lane per
height, rows stored straight to the record table -- through the C ABI against the oracle: every per-height
field, the launch statistics and both histograms. Byzantine counts around the quorum (runs that stop in the
middle), heights around the 64-lane pass boundaries, the tick limit, phase caps; and pipelined launches over
different instance ranges whose row-table sets are reused by instances that stop at other heights (a row
stored above the recorded height, or a stale row read by the prediction check or the chain repair, shows
there)."""
import functools

import numpy as np
import pytest

import oracle_lib as O
from bftsim.configs import BftConfig
from bftsim.distributed import stats_from_result
from parity_util import FIELDS, assert_same

pytestmark = pytest.mark.gpu


def _sim(cfg):
    from bftsim.runtime import Simulator
    return Simulator(cfg)


def _check_stats(st, cfg, first, n, ref, what):
    """the launch totals (bft_stats_kernel and the in-kernel histograms) against the oracle's sums"""
    want = stats_from_result(ref)
    for k in ("instances", "committed_heights", "views", "ticks", "flagged", "round_hist"):
        assert st[k] == want[k], (what, k, st[k], want[k])
    lat = O.run_stream(cfg, first, n, threads=8)["latency_hist"]
    assert st["latency_hist"] == [int(x) for x in lat], (what, "latency_hist")


def _run_check(cfg, first, n, what):
    sim = _sim(cfg)
    try:
        got = sim.run(first, n)
        st = sim.stats()
    finally:
        sim.close()
    ref = O.run(cfg, first, n, threads=8)
    assert_same(ref, got, what)
    assert all(np.array_equal(ref[k], got[k]) for k in FIELDS)
    _check_stats(st, cfg, first, n, ref, what)
    return got


@pytest.mark.parametrize("f", [0, 20, 21, 22, 42])
def test_byzantine_counts_130_heights(f):
    got = _run_check(BftConfig(n=64, heights=130, seed=51, byz_count=f), 0, 64, f"f={f}")
    assert int((got["committed_height"] == 130).sum()) == {0: 64, 20: 46, 21: 64, 22: 44, 42: 23}[f]


def test_heights_sweep():
    for heights in [1, 2, 3, 4] + list(range(62, 69)) + list(range(126, 133)):
        _run_check(BftConfig(n=64, heights=heights, seed=51, byz_count=21), 0, 3, f"heights={heights}")


def test_max_ticks_stops_the_run():
    got = _run_check(BftConfig(n=64, heights=70, seed=51, byz_count=21, max_ticks=33), 0, 3, "max_ticks=33")
    assert (got["committed_height"] == 33).all()


@pytest.mark.parametrize("cap", [4, 5])
def test_phase_caps(cap):
    _run_check(BftConfig(n=64, heights=70, seed=51, byz_count=21, phase_cap=cap), 0, 3, f"phase_cap={cap}")


PIPE_CFG = dict(n=64, heights=70, seed=51, byz_count=22)
PIPE_N, PIPE_LAUNCHES = 96, 7                      # 96 is not a multiple of 64


@functools.lru_cache(maxsize=None)
def _pipe_ref(k):
    """launch k's oracle result, computed once and shared (read-only) by both pipelined tests"""
    return O.run(BftConfig(**PIPE_CFG), k * PIPE_N, PIPE_N, threads=8)


def _head(ref, n):
    return {k: ref[k][:n] for k in FIELDS}


def _pipelined(sizes):
    cfg = BftConfig(**PIPE_CFG)
    stops = set()
    sim = _sim(cfg)
    try:
        sim.set_pipeline(True, 3)
        sim.set_hash_batch(2)
        sim.prepare(PIPE_N)
        for k in range(PIPE_LAUNCHES):
            n = sizes[k % len(sizes)]
            if len(sizes) > 1:
                sim.prepare(n)
            sim.launch(k * PIPE_N)
            sim.sync()
            got = sim.fetch()
            st = sim.stats()
            ref = _head(_pipe_ref(k), n)
            assert_same(ref, got, f"launch {k} of {n}")
            assert st["views"] == int(ref["views"].sum()) and st["committed_heights"] == int(ref["committed_height"].sum())
            stops.update(int(x) for x in ref["committed_height"])
    finally:
        sim.close()
    assert len(stops) > 3                          # instances stop at assorted heights: the sets see them all


def test_pipelined_ranges_reuse_sets():
    """depth 3 x batch 2, 7 launches over different ranges, sync + fetch after every launch: the ring wraps and
    each set is reused by instances that stop at other heights"""
    _pipelined([PIPE_N])


def test_pipelined_ranges_alternating_sizes():
    """the same sequence with prepare(96) / prepare(40) between the launches"""
    _pipelined([PIPE_N, 40])
