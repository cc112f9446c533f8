"""The HIP kernel bodies (bft_wave.h, bft_fast64.h) run by the CPU wave emulator against the oracle, bit for bit, at
every MessagePack width of the header's `time` field and across a change of width inside a chain (tests/time_cases.py):
test_emu_parity.py runs every shape at the default genesis time and block period alone, where `time` is always the
5-byte form. The oracle side is pinned to the msgpack package at the same widths by test_oracle_kat.py. Every case
first asserts, on the oracle's result, that it has the sizes it is there for."""
import pytest

import emu_lib as E
import oracle_lib as O
import time_cases as T
from bftsim.configs import BftConfig, cfg5
from parity_util import assert_same


# name -> (config, first instance, instances); the smallest shapes that reach each kernel body. Fewer heights and
# instances than time_cases.PLAIN and LONG (and seeds that show every size in them): the emulator runs on one CPU thread
SHAPES = {
    "n4-drop10": (lambda: BftConfig(n=4, heights=40, seed=2, drop_ppm=100_000, name="n4-drop10"), 0, 8),
    "n7-drop5": (lambda: cfg5(heights=40), 0, 8),
    "n64-byz21": (lambda: BftConfig(n=64, heights=30, seed=3, byz_count=21, name="n64-byz21"), 0, 3),
    "n64-byz21-le": (lambda: T.le(BftConfig(n=64, heights=30, seed=3, byz_count=21, name="n64-byz21")), 0, 3),
    "n64-byz21-drop5": (lambda: BftConfig(n=64, heights=30, seed=15, byz_count=21, drop_ppm=50_000, name="n64-drop5"), 0, 3),
    # with little-endian seeds the time case changes the schedule and most lossy Byzantine chains fork within 10
    # heights: seed 6, whose first 8 instances hold one that commits past tick 13 at every case
    "n64-byz21-drop5-le": (lambda: T.le(BftConfig(n=64, heights=20, seed=6, byz_count=21, drop_ppm=50_000,
                                                 name="n64-drop5")), 0, 8),
    "n100": (lambda: BftConfig(n=100, heights=20, seed=4, name="n100"), 0, 2),
}
LONG = {
    "n64-byz21-260": (lambda: BftConfig(n=64, heights=260, seed=3, byz_count=21, name="n64-byz21-260"), 0, 2),
    "n7-drop5-260": (lambda: cfg5(heights=260), 0, 4),
}


def _check(case, cfg, first, n, what):
    ref = O.run(cfg, first, n)
    T.assert_case(case, cfg, ref, what)
    assert_same(ref, E.run(cfg, first, n), what)
    return ref


@pytest.mark.parametrize("shape", list(SHAPES))
@pytest.mark.parametrize("case", T.SHORT_IDS)
def test_emulated_kernel_matches_oracle_at_every_time_width(case, shape):
    mk, first, n = SHAPES[shape]
    cfg = T.with_time(mk(), case)
    _check(case, cfg, first, n, f"{shape} {case}")


@pytest.mark.parametrize("shape", list(LONG))
def test_time_and_height_change_width_together(shape):
    """t-0: time = tick + 1, so on a lossless chain `height` and `time` go from 1 to 2 to 3 bytes at the same blocks"""
    mk, first, n = LONG[shape]
    cfg = T.with_time(mk(), "t-0")
    ref = _check("t-0", cfg, first, n, f"{shape} t-0")
    assert (ref["committed_height"] == 260).all()


@pytest.mark.parametrize("case", T.SHORT_IDS)
def test_full_kernel_alone_n64_at_every_time_width(case, monkeypatch):
    """BFT_EMU_FAST=0 (bftsim_set_fast(h, 0) on the GPU): the full kernel's own header sites at N = 64"""
    monkeypatch.setenv("BFT_EMU_FAST", "0")
    mk, first, n = SHAPES["n64-byz21"]
    cfg = T.with_time(mk(), case)
    _check(case, cfg, first, n, f"n64 full kernel {case}")


@pytest.mark.parametrize("case", T.SHORT_IDS)
def test_wave_hash_alone_le_at_every_time_width(case, monkeypatch):
    """BFT_EMU_SPEC=0: little-endian seeds at N = 64 with every height hashed by the wave, none taken from the seed
    chain's predictions; equal to the run with predictions and to the oracle"""
    mk, first, n = SHAPES["n64-byz21-le"]
    cfg = T.with_time(mk(), case)
    with_spec = E.run(cfg, first, n)
    monkeypatch.setenv("BFT_EMU_SPEC", "0")
    ref = _check(case, cfg, first, n, f"n64 le wave hash {case}")
    assert_same(ref, with_spec, f"n64 le predictions {case}")
