"""CPU: the chronicler (SPEC.md §11h). The Python reference alone (tests/timeline_ref.py) first, on a hand-made stream
with one instance per rule and on the simulated traces, whose premises it asserts; then the host build of the walk and
the rows (consensus-rs_amd/csrc/bft_timeline.h, tests/emu/timeline_host.cpp) against that reference array for array;
the same code as a stand-alone program under ASan + UBSan; the C ABI's bindings and argument checks."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import timeline_cases as TC     # first: it puts oracle/ on the path
import timeline_lib as TLL
import timeline_ref as TL
import audit_ref as AR

HERE = os.path.dirname(__file__)
PIN = json.load(open(os.path.join(HERE, "golden", "timeline_n4.json")))


def _host(c, want_key="want", **kw):
    """the host build over a case, asserted equal to the reference under the same cap"""
    got = TLL.timeline(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"], **kw)
    TL.assert_same({k: got[k] for k in TL.ARRAYS + ("report",)}, c[want_key])
    AR.assert_same({k: got["obs"][k] for k in AR.ARRAYS + ("report",)}, c["want"]["audit"])
    return got


def test_reference_on_the_handmade_rules():
    TC.check_handmade(TC.handmade())


def test_reference_on_the_lossy_n4_trace_is_the_pinned_one():
    """what the reference shows on "n4" (N = 4, 10 % drops, a forged validator), asserted as found and pinned"""
    w = TC.twins("n4")["want"]
    for k in TL.ARRAYS:
        assert w[k].tolist() == PIN[k], k
    assert w["report"] == PIN["report"]


def test_premises_of_the_simulated_cases():
    """between them the simulated cases hold a row with a round-change quorum, a row with PREPARED_FIRST, and a row with
    a commit certificate without PREPARED_FIRST (CERT_UNPREPARED, or a late prepare quorum); on the reference alone"""
    rc = first = cert_not_first = 0
    for case, plain in TC.SIMULATED:
        w = TC.twins(case, plain)["want"]
        cert = np.asarray(w["audit"]["cert_round"]) != 0xffff
        rc += int((w["rc_quorums"] > 0).sum())
        first += int(((w["flags"] & TL.PREPARED_FIRST) != 0).sum())
        cert_not_first += int((cert & ((w["flags"] & TL.PREPARED_FIRST) == 0)).sum())
        assert not (w["flags"][~cert] & (TL.PREPARED_FIRST | TL.CERT_UNPREPARED)).any()
        assert not (w["flags"][cert] & TL.LOCKED_OPEN).any()
    assert rc > 0 and first > 0 and cert_not_first > 0, (rc, first, cert_not_first)


@pytest.mark.parametrize("case,plain", TC.SIMULATED)
def test_host_build_equals_reference_on_simulated(case, plain):
    _host(TC.twins(case, plain))


def test_host_build_equals_reference_on_the_handmade_rules():
    c = TC.handmade()
    _host(c)
    _host(c, "want_cap2", tl_cap=2)


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_program_under_asan_ubsan():
    """the stand-alone program (its own main, run directly): the same walk and rows over every case, from and into heap
    buffers of exactly the counted sizes (the key table too), compared there with the reference"""
    exe = TLL.build_san()
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    hm = TC.handmade()
    obs = TLL.timeline(hm["stream"], hm["off"], hm["f0"], hm["cfg"], hm["heights"])
    runs = [("handmade", hm, obs, "want", 0), ("tl_cap 2", hm, obs, "want_cap2", 2)]
    for case, plain in TC.SIMULATED:
        c = TC.twins(case, plain)
        runs.append((f"{case} plain={plain}", c, TLL.timeline(c["stream"], c["off"], c["f0"], c["cfg"], c["heights"]), "want", 0))
    for name, c, got, key, tl_cap in runs:
        r = subprocess.run([exe], input=TLL.san_input(got, c["f0"], c["cfg"].n, tl_cap, c["heights"], c[key]),
                           capture_output=True, env=env, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        rows = (len(c["f0"]) - 1) * c["heights"]
        assert r.stdout.decode().strip() == f"ok {len(c['off']) - 1} frames {rows} rows", name
        assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound_and_check_arguments():
    """bound; a null handle, out or report refused, and the observer's argument errors are this call's, all before any
    device work and with nothing written (this runs without a GPU)"""
    from bftsim import _abi, runtime, trace
    from bftsim.configs import cfg1 as mk
    L = runtime.lib()
    rep, arep = _abi.CTimelineReport(), _abi.CAuditReport()
    o, arrs = _abi.alloc_timeline(1, 6)
    assert L.bftsim_timeline_trace(None, None, 0, None, 0, None, 0, 1, 0, 0, ctypes.byref(o), None, None, ctypes.byref(rep)) == -1
    assert L.bftsim_timeline_last_trace(None, 0, 0, 0, 0, ctypes.byref(o), None, None, ctypes.byref(rep)) == -1
    assert L.bftsim_timeline_last_ms(None, None, None, None, None) == -1
    for name in ("timeline_trace", "timeline_last_trace", "timeline_ms"):
        assert callable(getattr(runtime.Simulator, name))
    for name in ("row", "open_height", "rounds_walked", "stalled"):
        assert callable(getattr(trace.Timeline, name))
    c, keep = _abi.to_cconfig(mk(True, heights=6))
    h = ctypes.c_void_p()
    L.bftsim_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert h.value
    stream = np.zeros(16, np.uint8)
    for a in arrs.values():
        a.view(np.uint8)[...] = 7
    rep.prepared, arep.frames = 77, 78

    def call(off, f0, frames=2, inst=1, heights=6, out=o, rep=rep, nbytes=16):
        off, f0 = np.array(off, np.uint64), np.array(f0, np.uint64)
        return L.bftsim_timeline_trace(h, stream.ctypes.data, nbytes, off.ctypes.data, frames, f0.ctypes.data, inst, heights, 0,
                                       0, ctypes.byref(out) if out is not None else None, None, ctypes.byref(arep),
                                       ctypes.byref(rep) if rep is not None else None)

    assert call([0, 8, 16], [0, 2], rep=None) == -1                     # null report
    assert call([0, 8, 16], [0, 2], out=None) == -1                     # null out
    assert call([0, 9, 8], [0, 2], nbytes=8) == -1                      # the observer's: frame_off decreases
    assert call([0, 8, 15], [0, 2]) == -1
    assert call([0, 8, 16], [1, 2]) == -1
    assert call([0, 8, 16], [0, 2, 1, 2], inst=3) == -1
    assert call([0, 8, 16], [0, 2], heights=0) == -1
    assert call([0, 8, 16], [0, 2], frames=1 << 32) == -1
    assert L.bftsim_timeline_last_trace(h, 0, 1, 0, 0, ctypes.byref(o), None, ctypes.byref(arep), ctypes.byref(rep)) == -1   # no kept trace
    assert len(L.bftsim_last_error(h)) > 0 and rep.prepared == 77 and arep.frames == 78      # nothing written
    assert all((a.view(np.uint8) == 7).all() for a in arrs.values())
    del keep


def test_new_structs_bound_in_integration_md():
    """bftsim_timeline_report / _out: INTEGRATION.md's #[repr(C)] structs against the header, by the checker of
    test_integration_binding (field names, types, offsets and sizes as gcc lays them out); the ctypes mirrors too"""
    import re
    import test_integration_binding as B
    from bftsim import _abi
    txt = re.sub(r"struct (bftsim_timeline_\w+) \{(.*?)\};\s*typedef struct \1 \1;", r"typedef struct \1 {\2} \1;",
                 B.header_text(), flags=re.S)
    decls = {k: v for k, v in B.c_struct_decls(txt).items() if k.startswith("bftsim_timeline_")}
    assert set(decls) == {"bftsim_timeline_report", "bftsim_timeline_out"}
    src = B.strip_rust_comments(B.rust_blocks())
    rs, consts = B.rust_structs(src), B.rust_consts(src)
    lay = B.gcc_layout({k: [f for f, _ in v] for k, v in decls.items()})
    for name, fields in decls.items():
        assert [f for f, _ in rs[name]] == [f for f, _ in fields], name
        assert [B.canon_rust(B.parse_rust_type(t), consts) for _, t in rs[name]] == [t for _, t in fields], name
        size, _, offs = B.struct_layout(name, rs, consts, {})
        assert size == lay[(name, "sizeof")]
        for f, o in offs.items():
            assert o == lay[(name, f)], (name, f)
    for name, cls in (("bftsim_timeline_report", _abi.CTimelineReport), ("bftsim_timeline_out", _abi.CTimelineOut)):
        assert ctypes.sizeof(cls) == lay[(name, "sizeof")]
        assert [f for f, _ in cls._fields_] == [f for f, _ in decls[name]]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[(name, f)], (name, f)
    for k, v in (("KEY_OVERFLOW", 1), ("PREPARED_FIRST", 1), ("CERT_UNPREPARED", 2), ("LOCKED_OPEN", 4)):
        assert consts["BFTSIM_TIMELINE_" + k].strip() == str(v)
