"""CPU: the trace's frame emitter (consensus-rs_amd/csrc/bft_trace.h, host build tests/emu/trace_host.cpp) against
the Python reference of the trace (tests/trace_ref.py: msgpack oracle + Python secp256k1 over the oracle's broadcast
log), the golden pin of that reference, and the emitter as a stand-alone program under ASan + UBSan."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import trace_lib as TL
import trace_ref as TR
import wire_ref as R

HERE = os.path.dirname(__file__)
PIN = json.load(open(os.path.join(HERE, "golden", "trace_cfg1_n5.json")))


@pytest.fixture(scope="module")
def cfg1_ref():
    stream, off, meta, ms = TR.reference("cfg1")["inst"][0]
    return dict(stream=stream, off=off, meta=meta, ms=ms)


@pytest.fixture(scope="module")
def n4_ref():
    return TR.reference("n4")["inst"]


def test_reference_pinned_to_golden(cfg1_ref):
    """the Python reference alone: frame count, bytes and Keccak-256 of cfg1's instance 0 (6 heights)"""
    assert len(cfg1_ref["ms"]) == PIN["frames"]
    assert len(cfg1_ref["stream"]) == PIN["bytes"]
    assert O.keccak256(cfg1_ref["stream"]).hex() == PIN["keccak256"]
    codes = [m["code"] for m in cfg1_ref["ms"]]
    assert {1, 2, 3, 4} <= set(codes)                        # round changes: the 9-byte create_time too
    assert [int(x) for x in R.split_frames(cfg1_ref["stream"])] == [int(x) for x in cfg1_ref["off"]]


def _check_emitter(ms, stream, off):
    for k, m in enumerate(ms):
        want = stream[int(off[k]):int(off[k + 1])]
        got, n, counted = TL.frame(m)
        assert counted == n == len(want), (k, m["code"], counted, n, len(want))
        assert got == want, (k, m["code"])


def test_emitter_equals_reference_cfg1(cfg1_ref):
    _check_emitter(cfg1_ref["ms"], cfg1_ref["stream"], cfg1_ref["off"])


def test_emitter_equals_reference_forged_lossy(n4_ref):
    """N=4, drops, validator 2 forged, instances 3..5: forged frames, non-canonical blocks, unequal counts"""
    assert len({len(ms) for _, _, _, ms in n4_ref}) > 1
    for stream, off, meta, ms in n4_ref:
        assert (meta[:, 2] & 1).any()
        _check_emitter(ms, stream, off)


def test_bounded_write_stops_at_the_capacity(cfg1_ref):
    """a capacity below the frame: the bytes up to it, nothing past it, and the full length reported"""
    for m in cfg1_ref["ms"][:8]:
        full, n, _ = TL.frame(m)
        for cap in (0, 1, 5, n - 1):
            part, n2, counted = TL.frame(m, cap=cap)
            assert n2 == counted == n and part == full[:cap]


def test_create_time():
    L = TL.lib()
    assert L.trace_host_create_time(4, 1536517089, 3, 7) == 1000 * (1536517089 + 21)
    for code in (1, 2, 3):
        assert L.trace_host_create_time(code, 1536517089, 3, 7) == 0


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_emitter_program_under_asan_ubsan(cfg1_ref):
    """the stand-alone program (its own main, run directly): every frame of the cfg1 log into a heap buffer of
    exactly the counted length, and into one half as long"""
    exe = TL.build_san()
    ms = cfg1_ref["ms"]
    frames = [cfg1_ref["stream"][int(cfg1_ref["off"][k]):int(cfg1_ref["off"][k + 1])] for k in range(len(ms))]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=TL.san_input(ms, frames), capture_output=True, env=env, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.decode().strip() == f"ok {len(ms)} frames {len(cfg1_ref['stream'])} bytes"
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound():
    """the C ABI of the trace is exported and refuses a null handle"""
    from bftsim import runtime, trace
    L = runtime.lib()
    assert L.bftsim_set_trace_keep(None, 1) == -1
    assert L.bftsim_trace_sizes(None, 0, None, None) == -1
    assert L.bftsim_export_trace(None, 0, 0, None, 0, None, 0, None, None) == -1
    assert callable(trace.audit) and hasattr(runtime.Simulator, "export_trace")


def test_trace_columns():
    from bftsim.trace import Trace
    meta = np.array([[7, 2 | (3 << 8) | (70 << 16), 9, 1]], np.uint32)
    t = Trace(np.arange(10, dtype=np.uint8), np.array([0, 10], np.uint64), meta, np.array([0, 0, 1], np.uint64))
    assert (int(t.tick[0]), int(t.phase[0]), int(t.code[0]), int(t.sender[0]), int(t.flags[0])) == (7, 2, 3, 70, 9)
    assert t.frames(0) == [] and t.frames(1) == [bytes(range(10))] and len(t) == 1
