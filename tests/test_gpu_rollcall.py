"""GPU: the roll call (include/bftsim.h bftsim_rollcall_trace / bftsim_rollcall_last_trace, SPEC.md §11i): per validator
what it signed, and per view the wire proves started its proposer and whether that proposer's PrePrepare is there, found
on the device. The cases of tests/test_rollcall_cpu.py equal the independent Python roll call (tests/rollcall_ref.py)
array for array; the kept trace equals its export; a proposer-crash run is closed against the CRASH draws of SPEC.md §5;
a larger Byzantine run is checked, with the library's own statuses, signers and certificates, against the Python rule."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import rollcall_cases as RC     # first: it puts oracle/ on the path
import rollcall_ref as RR
import timeline_ref as TL
import audit_ref as AR
import ledger_ref as LR
import trace_ref as TRC
import twins_ref as TW
from bftsim.configs import BftConfig

pytestmark = pytest.mark.gpu
RESULT = ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash")
STREAMS = RC.stream_cases()


def _tr(stream, off, f0):
    return SimpleNamespace(stream=np.frombuffer(bytes(stream), np.uint8), frame_off=np.asarray(off, np.uint64),
                           inst_frame0=np.asarray(f0, np.uint64))


def _same_audit(a, b):
    for k in AR.ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.report == b.report


def _same_timeline(a, b):
    for k in TL.ROWS + ("inst_flags", "open_heights"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.report == b.report


def _same_rollcall(a, b):
    for k in RR.ARRAYS:
        assert np.array_equal(a.arrays[k], b.arrays[k]), k
    assert np.array_equal(a.records, b.records) and a.report == b.report
    _same_audit(a.audit, b.audit)
    _same_timeline(a.timeline, b.timeline)


def _own_audit(got):
    """the library's own statuses, signers and certificates, for the Python rule"""
    return {k: getattr(got.audit, k) for k in ("frame_status", "frame_signer", "cert_round", "cert_digest", "cert_frame")}


@pytest.mark.parametrize("tl_cap", [0, 2])
@pytest.mark.parametrize("name", list(STREAMS))
def test_stream_equals_reference(name, tl_cap):
    """the library's arrays, records and report equal the Python roll call's under the same cap; the audit and timeline
    outputs passed through are bftsim_audit_trace's and bftsim_timeline_trace's"""
    from bftsim.runtime import Simulator
    c = STREAMS[name]()
    if tl_cap == 0:
        want = c["want"]
    elif "want_cap2" in c:
        want = c["want_cap2"]
    else:
        want = RR.rollcall(c["stream"], c["off"], c["f0"], c["cfg"].addresses, c["cfg"].seed_byte_order == 1, c["genesis"],
                           c["heights"], tl_cap=tl_cap, audit=c["want"]["audit"])
    sim = Simulator(c["cfg"])                 # no secrets, no set_crypto: the roll call needs neither
    try:
        tr = _tr(c["stream"], c["off"], c["f0"])
        got = sim.rollcall_trace(tr, max_heights=c["heights"], tl_cap=tl_cap)
        ms = sim.rollcall_ms()
        audit = sim.audit_trace(tr, max_heights=c["heights"])
        tl = sim.timeline_trace(tr, max_heights=c["heights"], tl_cap=tl_cap)
    finally:
        sim.close()
    RR.assert_same(got, want)
    AR.assert_same(got.audit, c["want"]["audit"])
    _same_audit(got.audit, audit)
    _same_timeline(got.timeline, tl)
    TL.assert_same(got.timeline, want["timeline"])
    for i in range(got.n):
        assert got.missed(i) == RR.missed_of(want, i) and got.silent(i) == RR.silent_of(want, i), i
        assert [tuple(int(r[k]) for k in ("height", "round")) for r in got.views(i)] == [v[:2] for v in RR.views_of(want, i)]
        for v in range(c["cfg"].n):
            r = got.row(i, v)
            assert r["frames"] == want["frames"][i, v].tolist() and r["missed"] == int(want["missed"][i, v])
    assert all(x >= 0 for x in ms) and ms[0] > 0
    if name in ("crash", "cfg1") and tl_cap == 0:
        RC.check_against_run(got, c["cfg"], c["ref"]["res"], c["ref"]["first"])


def test_family_shares_the_observer_and_each_call_keeps_its_own_ms():
    """audit, archive, accuse, timeline and roll call in that order on one Simulator over "cfg1" (the fewest frames of
    STREAMS: 71, one instance, 6 heights): every continuation's audit outputs are the plain audit's and the roll call's
    timeline is timeline_trace's. The roll call runs the chronicler's passes but is no timeline call: timeline_ms(),
    archive_ms() and accuse_ms() read the same stored floats after it as before, while audit_ms() now describes the
    roll call's observer passes (its first three sum, in float, to rollcall_ms()[0] as they did to timeline_ms()[0])"""
    from bftsim.runtime import Simulator
    c = STREAMS["cfg1"]()
    f32 = lambda ms: np.float32(ms[0]) + np.float32(ms[1]) + np.float32(ms[2])
    sim = Simulator(c["cfg"])
    try:
        tr, H = _tr(c["stream"], c["off"], c["f0"]), c["heights"]
        audit = sim.audit_trace(tr, max_heights=H)
        _, archive = sim.archive_trace(tr, max_heights=H)
        accuse = sim.accuse_trace(tr, max_heights=H)
        tl = sim.timeline_trace(tr, max_heights=H)
        before = sim.timeline_ms(), sim.archive_ms(), sim.accuse_ms()
        audit_before = sim.audit_ms()
        roll = sim.rollcall_trace(tr, max_heights=H)
        after = sim.timeline_ms(), sim.archive_ms(), sim.accuse_ms()
        audit_after, roll_ms = sim.audit_ms(), sim.rollcall_ms()
    finally:
        sim.close()
    for got in (archive, accuse, tl, roll):
        _same_audit(got.audit, audit)
    _same_timeline(roll.timeline, tl)
    print("ms", before, after, audit_before, audit_after, roll_ms)
    assert after == before
    assert len(roll_ms) == 6 and len(before[0]) == 4
    assert f32(audit_before) == np.float32(before[0][0]) and f32(audit_after) == np.float32(roll_ms[0])
    assert audit_after != audit_before


def test_last_trace_equals_exported_and_leaves_the_run_alone():
    """rollcall_last_trace equals rollcall_trace(export_trace()) for a launch and for a sub-range, and the Python roll
    call on the reference trace; fetch() and the crypto_verify report are bit-identical before and after"""
    ref = TW.reference("n7")
    from bftsim.runtime import BftsimError, Simulator
    sim = Simulator(ref["cfg"])
    sim.set_crypto(ref["secrets"], ref["forged"], 1024)
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    res = sim.run(ref["first"], ref["n"])
    sim.crypto_verify()
    try:
        before, stats = sim.fetch(), sim.stats()
        whole, part = sim.rollcall_last_trace(), sim.rollcall_last_trace(1, 2)
        via, via_part = sim.rollcall_trace(sim.export_trace()), sim.rollcall_trace(sim.export_trace(1, 2))
        after, stats_after = sim.fetch(), sim.stats()
        with pytest.raises(BftsimError):
            sim.rollcall_last_trace(2, 2)                               # past the launch
    finally:
        sim.close()
    _same_rollcall(whole, via)
    _same_rollcall(part, via_part)
    RR.assert_same(whole, RC.twins("n7")["want"])                       # the run's frames are the reference trace's
    assert np.array_equal(part.frames, whole.frames[1:]) and np.array_equal(part.inst_views, whole.inst_views[1:])
    assert stats == stats_after
    for k in RESULT:
        assert np.array_equal(before[k], res[k]) and np.array_equal(after[k], res[k]), k


def test_crash_run_closes_against_the_crash_draws():
    """N = 10, 6 heights, proposer_crash_ppm 300,000, 8 instances, lossless, on the GPU: the MISSED views are exactly
    the started views whose CRASH draw fell, and every committed height has one WON view, the run's"""
    from bftsim.runtime import Simulator
    cfg, sec = LR.keyed(RC.crash_config(n=10, heights=6, seed=4), 5)
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), 65536)
    sim.set_trace_keep(True)
    try:
        res = sim.run(0, 8)
        sim.crypto_verify()
        tr = sim.export_trace()
        got = sim.rollcall_last_trace()
    finally:
        sim.close()
    want = RR.rollcall(tr.stream.tobytes(), tr.frame_off, tr.inst_frame0, cfg.addresses, cfg.seed_byte_order == 1,
                       TRC.genesis_hash(cfg), cfg.heights, audit=_own_audit(got))
    RR.assert_same(got, want)
    RC.check_against_run(got, cfg, res, 0)
    print("crash", "frames", len(tr), got.report, [got.missed(i) for i in range(8)])
    assert got.report["by_outcome"][1] > 0 and got.report["won"] == int(res["committed_height"].sum())


def test_n65_byzantine_lossy_run_equals_the_rule():
    """N = 65 with 21 Byzantine validators and 5 % drops, 4 instances x 3 heights, twins on: the outputs equal the Python
    rule applied to the library's own statuses, signers and certificates. No Python signing at this size. Validator 64
    has the one row past lane 63"""
    from bftsim.runtime import Simulator
    cfg, sec = LR.keyed(BftConfig(n=65, heights=3, seed=9, byz_count=21, drop_ppm=50_000), 4)
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), 65536)
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    try:
        sim.run(0, 4)
        sim.crypto_verify()
        tr = sim.export_trace()
        got = sim.rollcall_last_trace()
    finally:
        sim.close()
    want = RR.rollcall(tr.stream.tobytes(), tr.frame_off, tr.inst_frame0, cfg.addresses, cfg.seed_byte_order == 1,
                       TRC.genesis_hash(cfg), cfg.heights, audit=_own_audit(got))
    RR.assert_same(got, want)
    print("n65", "frames", len(tr), got.report)
    assert got.frames[:, 64].any() and got.report["views"] >= 4


def test_hostile_streams_are_no_error():
    """audit_ref.truncations of a frame, an empty stream, and a RoundChange quorum at round 2^60: no error; the views
    are (1, 0) alone, or that one more view"""
    from bftsim.runtime import Simulator
    c = RC.handmade()
    cfg, sec = TW._keyed(BftConfig(n=RC.N, heights=RC.H, seed=5), 7)
    k = int(c["f0"][c["index"]["round 0 after certificate"]])
    cut = AR.truncations(c["stream"], c["off"], [k, k + 1])
    far = RC._sign_all({"far": [(v, 4, 1, 1 << 60, bytes(32)) for v in range(5)]}, sec, None)["far"]
    import accuse_ref as XR
    stream, off, f0 = XR.stream_of([far])
    sim = Simulator(cfg)
    try:
        got = sim.rollcall_trace(_tr(stream, off, f0))
        empty = sim.rollcall_trace(_tr(b"", np.zeros(1, np.uint64), np.zeros(1, np.uint64)))
        torn = sim.rollcall_trace(_tr(*AR.appended(b"", np.zeros(1, np.uint64), cut)))
    finally:
        sim.close()
    g0 = c["prop"]["g"]
    assert RR.views_of(got, 0) == [(1, 0, g0(0), RR.MISSED, RR.NONE, RR.NONE), (1, 1 << 60, g0(1 << 60), RR.MISSED, 4, RR.NONE)]
    assert RR.views_of(torn, 0) == [(1, 0, g0(0), RR.MISSED, RR.NONE, RR.NONE)] and torn.report["frames"] == 0
    assert torn.audit.report["undecodable"] == len(cut) and RR.silent_of(torn, 0) == list(range(RC.N))
    assert empty.n == 0 and empty.report["views"] == 0 and len(empty.records) == 0


def test_refused_calls_write_nothing_and_rec_cap_keeps_the_prefix():
    from bftsim import _abi, runtime
    c = RC.handmade()
    sim = runtime.Simulator(c["cfg"])
    try:
        L = runtime.lib()
        stream = np.frombuffer(c["stream"], np.uint8)
        off, f0 = c["off"], c["f0"]
        F, n = len(off) - 1, len(f0) - 1
        o, arrs = _abi.alloc_rollcall(n, c["cfg"].n, 7)
        ao, aarrs = _abi.alloc_audit(F, n, c["heights"])
        to, tarrs = _abi.alloc_timeline(n, c["heights"])
        rep, arep, trep = _abi.CRollCallReport(), _abi.CAuditReport(), _abi.CTimelineReport()
        rep.views, arep.frames, trep.prepared = 77, 78, 79
        every = list(arrs.values()) + list(aarrs.values()) + list(tarrs.values())
        for a in every:
            a.view(np.uint8)[...] = 7
        no_rec = _abi.CRollCallOut()
        no_rec.rec_cap = 3

        def call(out_p=ctypes.byref(o), rep_p=ctypes.byref(rep), heights=c["heights"], frames=F):
            return L.bftsim_rollcall_trace(sim.h, stream.ctypes.data, len(stream), off.ctypes.data, frames, f0.ctypes.data, n,
                                           heights, 0, 0, out_p, rep_p, ctypes.byref(ao), ctypes.byref(arep),
                                           ctypes.byref(to), ctypes.byref(trep))

        for rc in (call(out_p=None), call(rep_p=None), call(out_p=ctypes.byref(no_rec)), call(heights=0), call(frames=F - 1)):
            assert rc == -1
        assert L.bftsim_rollcall_last_trace(sim.h, 0, 1, 0, 0, ctypes.byref(o), ctypes.byref(rep), ctypes.byref(ao),
                                            ctypes.byref(arep), ctypes.byref(to), ctypes.byref(trep)) == -1   # no kept trace
        assert rep.views == 77 and arep.frames == 78 and trep.prepared == 79
        assert all((a.view(np.uint8) == 7).all() for a in every)
        assert call() == 0 and rep.views == len(c["want"]["records"]) and arep.frames == F
        assert np.array_equal(arrs["records"], c["want"]["records"][:7])           # rec_cap 7: the exact prefix
        assert np.array_equal(arrs["due"].reshape(n, -1), c["want"]["due"])
        kept = sim.rollcall_trace(_tr(c["stream"], off, f0), max_heights=c["heights"], rec_cap=7)
        RR.assert_same(kept, c["want"], rec_cap=7)
    finally:
        sim.close()
