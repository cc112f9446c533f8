"""CPU: Fast64::canonical_run (bft_fast64.h) -- a run of canonical heights applied at once, one lane per
height -- in the wave emulator against the oracle, bit for bit, with both histograms: Byzantine counts around
the quorum (runs that stop in the middle because neither or both variants commit), heights around the 64-lane
pass boundaries, the tick limit, phase caps with and without the canonical path, a silent validator,
little-endian seeds (path unchanged), the headline shape; that the run is really taken; run off against on."""
import ctypes
import dataclasses

import numpy as np
import pytest

import oracle_lib as O
import emu_lib as E
from bftsim.configs import BftConfig, cfg3
from parity_util import assert_same

HISTS = ("round_hist", "latency_hist")


def _check(cfg, first, n, what):
    got = E.run(cfg, first, n)
    assert_same(O.run(cfg, first, n), got, what)
    ref = O.run_stream(cfg, first, n, threads=4)
    for k in HISTS:
        assert np.array_equal(ref[k], got[k]), (what, k)
    return got


@pytest.mark.parametrize("f", [0, 20, 21, 22, 42])
def test_byzantine_counts_130_heights(f):
    """130 heights span three passes. f = 20: some instances stop inside a run (neither variant commits) and time
    out; f = 22 and 42: forks freeze instances at assorted ticks."""
    cfg = BftConfig(n=64, heights=130, seed=51, byz_count=f)
    got = _check(cfg, 0, 64, f"f={f}")
    full = int((got["committed_height"] == 130).sum())
    # the oracle's spread: the others stop at assorted heights, so the mid-run stop is exercised
    assert full == {0: 64, 20: 46, 21: 64, 22: 44, 42: 23}[f]


@pytest.mark.parametrize("heights", [1, 2, 3, 4] + list(range(62, 69)) + list(range(126, 133)))
def test_heights_sweep(heights):
    _check(BftConfig(n=64, heights=heights, seed=51, byz_count=21), 0, 3, f"heights={heights}")


def test_max_ticks_stops_the_run():
    cfg = BftConfig(n=64, heights=70, seed=51, byz_count=21, max_ticks=33)
    got = _check(cfg, 0, 3, "max_ticks=33")
    assert (got["committed_height"] == 33).all()


@pytest.mark.parametrize("cap", [4, 5])
def test_phase_caps(cap):
    """phase_cap = 4: no canonical path; 5: the smallest cap with it."""
    _check(BftConfig(n=64, heights=70, seed=51, byz_count=21, phase_cap=cap), 0, 3, f"phase_cap={cap}")


def test_silent_validator():
    _check(BftConfig(n=64, heights=70, seed=51, byz_count=10, silent=[3]), 0, 3, "silent")


def test_little_endian_seeds_unchanged():
    cfg = dataclasses.replace(cfg3(heights=20), seed_byte_order=1)
    got = E.run(cfg, 0, 3)
    assert_same(O.run(cfg, 0, 3), got, "cfg3-le")


def test_cfg3_100_heights():
    _check(cfg3(heights=100), 0, 4, "cfg3-100")


def _counts(reset=True):
    fn = E.lib().bft_emu_canon_counts
    fn.argtypes = [ctypes.POINTER(ctypes.c_uint64), ctypes.c_int]
    fn.restype = None
    out = (ctypes.c_uint64 * 2)()
    fn(out, 1 if reset else 0)
    return int(out[0]), int(out[1])


def test_the_run_is_taken():
    """cfg3, 100 heights: tick 0 (the T-step and phase loop) and the entry tick (canonical_tick) are the only
    heights allowed outside the run, one more is slack: at least 97 of every instance's 100 come from the run."""
    cfg = cfg3(heights=100)
    for inst in range(4):
        _counts()
        got = E.run(cfg, inst, 1)
        by_run, by_tick = _counts()
        assert got["committed_height"][0] == 100
        assert by_run + by_tick == 100, (inst, by_run, by_tick)
        assert by_run >= 97, (inst, by_run, by_tick)


@pytest.mark.parametrize("f", [20, 21, 22])
def test_run_off_and_on(f, monkeypatch):
    cfg = BftConfig(n=64, heights=130, seed=51, byz_count=f)
    on = E.run(cfg, 0, 16)
    monkeypatch.setenv("BFT_EMU_CANON_RUN", "0")
    _counts()
    off = E.run(cfg, 0, 16)
    assert _counts()[0] == 0            # the switch really turned the run off
    assert_same(on, off, f"run on vs off, f={f}")
    for k in HISTS:
        assert np.array_equal(on[k], off[k]), k
