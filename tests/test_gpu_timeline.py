"""GPU: the chronicler (include/bftsim.h bftsim_timeline_trace / bftsim_timeline_last_trace, SPEC.md §11h): per height
the first prepare certificate, the round-change quorums and the verdicts that join them to the observer's commit
certificate, tallied on the device. The cases of tests/test_timeline_cpu.py equal the independent Python chronicler
(tests/timeline_ref.py) array for array; the kept trace equals its export; a larger Byzantine run is checked, with the
library's own statuses, signers and certificates, against the Python rule."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import timeline_cases as TC     # first: it puts oracle/ on the path
import timeline_ref as TL
import audit_ref as AR
import ledger_ref as LR
import twins_ref as TW
from bftsim.configs import BftConfig

pytestmark = pytest.mark.gpu
RESULT = ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash")
EMPTY_REPORT = dict.fromkeys(TL.REPORT, 0)


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
    _same_audit(a.audit, b.audit)


def _own_audit(got):
    """the library's own statuses, signers and certificates, for the Python rule"""
    return {k: getattr(got.audit, k) for k in ("frame_status", "frame_signer", "cert_round", "cert_digest", "cert_frame")}


CASES = [("handmade", "want", {}), ("handmade", "want_cap2", dict(tl_cap=2))] + [
    (case + (" plain" if plain else ""), "want", {}) for case, plain in TC.SIMULATED]


@pytest.mark.parametrize("name,key,kw", CASES, ids=[f"{n}-{k}" for n, k, _ in CASES])
def test_stream_equals_reference(name, key, kw):
    """the library's arrays and report equal the Python chronicler's under the same cap; the audit outputs passed
    through are bftsim_audit_trace's"""
    from bftsim.runtime import Simulator
    c = TC.handmade() if name == "handmade" else TC.twins(name.split()[0], name.endswith("plain"))
    sim = Simulator(c["cfg"])                 # no secrets, no set_crypto: the chronicler needs neither
    try:
        tr = _tr(c["stream"], c["off"], c["f0"])
        got = sim.timeline_trace(tr, max_heights=c["heights"], **kw)
        ms = sim.timeline_ms()
        audit = sim.audit_trace(tr, max_heights=c["heights"])
    finally:
        sim.close()
    TL.assert_same(got, c[key])
    AR.assert_same(got.audit, c["want"]["audit"])
    _same_audit(got.audit, audit)
    w = c[key]
    for i in range(got.n):
        assert got.open_height(i) == int(w["open_height"][i]) and got.stalled(i) == TL.stalled(w, i), i
        for x in range(1, c["heights"] + 1):
            r = got.row(i, x)
            assert r["prep_voters"] == TC.voters_of(w, i, x) and r["flags"] == int(w["flags"][i, x - 1])
            assert got.rounds_walked(i, x) == (0 if w["rc_max_round"][i, x - 1] == 0xffff else int(w["rc_max_round"][i, x - 1]))
    assert all(x >= 0 for x in ms) and ms[0] > 0


@pytest.mark.parametrize("twins", [True, False])
def test_last_trace_equals_exported_and_leaves_the_run_alone(twins):
    """timeline_last_trace equals timeline_trace(export_trace()) for a launch and for a sub-range, and the Python
    chronicler on the reference trace; fetch() and stats() are the same before and after"""
    ref = TW.reference("n7")
    from bftsim.runtime import BftsimError, Simulator
    sim = Simulator(ref["cfg"])
    sim.set_crypto(ref["secrets"], ref["forged"], 1024)
    sim.set_trace_keep(True)
    sim.set_trace_twins(twins)
    res = sim.run(ref["first"], ref["n"])
    sim.crypto_verify()
    try:
        before, stats = sim.fetch(), sim.stats()
        whole, part = sim.timeline_last_trace(), sim.timeline_last_trace(1, 2)
        via, via_part = sim.timeline_trace(sim.export_trace()), sim.timeline_trace(sim.export_trace(1, 2))
        after, stats_after = sim.fetch(), sim.stats()
        with pytest.raises(BftsimError):
            sim.timeline_last_trace(2, 2)                               # past the launch
    finally:
        sim.close()
    _same_timeline(whole, via)
    _same_timeline(part, via_part)
    TL.assert_same(whole, TC.twins("n7", not twins)["want"])            # the run's frames are the reference trace's
    assert np.array_equal(part.flags, whole.flags[1:]) and np.array_equal(part.prep_frame, whole.prep_frame[1:])
    assert stats == stats_after
    for k in RESULT:
        assert np.array_equal(before[k], res[k]) and np.array_equal(after[k], res[k]), k


def test_n65_byzantine_lossy_run_equals_the_rule():
    """N = 65 with 21 Byzantine validators and 5 % drops, 2 instances x 3 heights: quorums of 44 voters. The outputs
    equal the Python rule applied to the library's own statuses, signers and certificates. No Python signing at this
    size. Validator 64, the only one of voter word 1, votes in the tables here but in no frozen certificate: a round's
    senders broadcast in index order, so it comes after the 44th voter (the CPU oracle's log shows it last in every
    round). Word 1 in the outputs is test_n100_second_voter_word_in_the_certificates"""
    from bftsim.runtime import Simulator
    cfg, sec = LR.keyed(BftConfig(n=65, heights=3, seed=9, byz_count=21, drop_ppm=50_000), 4)
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), 65536)
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    try:
        sim.run(0, 2)
        sim.crypto_verify()
        tr = sim.export_trace()
        got = sim.timeline_last_trace()
    finally:
        sim.close()
    want = TL.timeline(tr.stream.tobytes(), tr.frame_off, tr.inst_frame0, cfg.addresses, cfg.seed_byte_order == 1, cfg.heights,
                       audit=_own_audit(got))
    TL.assert_same(got, dict(want, audit=None))
    print("n65", "frames", len(tr), got.report)
    assert got.report["prepared"] > 0
    assert ((tr.sender == 64) & np.isin(tr.code, (2, 4))).any()                      # word 1 is written in the tables


def test_n100_second_voter_word_in_the_certificates():
    """N = 100, 2 heights, lossless, one instance: a quorum is 67 voters, so validators 64..66 stand in word 1 of every
    frozen prepare certificate; the outputs equal the Python rule over the library's own statuses, signers and
    certificates"""
    from bftsim.configs import cfg4
    from bftsim.runtime import Simulator
    cfg, sec = LR.keyed(cfg4(100, heights=2), 5)
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), 0)
    sim.set_trace_keep(True)
    try:
        sim.run(0, 1)
        sim.crypto_verify()
        tr = sim.export_trace()
        got = sim.timeline_last_trace()
    finally:
        sim.close()
    want = TL.timeline(tr.stream.tobytes(), tr.frame_off, tr.inst_frame0, cfg.addresses, cfg.seed_byte_order == 1, cfg.heights,
                       audit=_own_audit(got))
    TL.assert_same(got, dict(want, audit=None))
    assert got.prep_voters[0, :, 1].all() and all(len(got.row(0, x)["prep_voters"]) == 67 for x in (1, 2))
    assert got.report["prepared"] == got.report["prepared_first"] == 2


def test_lossless_n4_run_is_prepared_first_at_the_runs_round():
    """a lossless N = 4 launch of 3 heights: every committed height has its prepare quorum before its commit quorum, at
    the run's round, and no round-change quorum"""
    from bftsim.runtime import Simulator
    cfg, sec = LR.keyed(BftConfig(n=4, heights=3, seed=21), 7)
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), 4096)
    sim.set_trace_keep(True)
    try:
        res = sim.run(0, 3)
        sim.crypto_verify()
        got = sim.timeline_last_trace()
    finally:
        sim.close()
    for i in range(3):
        ch = int(res["committed_height"][i])
        assert ch == 3 and got.open_height(i) == 4 and not got.stalled(i)
        for x in range(1, ch + 1):
            r = got.row(i, x)
            assert r["prepared_first"] and not r["cert_unprepared"] and not r["locked_open"], (i, x, r)
            assert r["prep_round"] == int(res["round"][i, x - 1]) == int(got.audit.cert_round[i, x - 1])
            assert r["prep_digest"] == bytes(res["block_hash"][i, x - 1]) and r["prep_frame"] < int(got.audit.cert_frame[i, x - 1])
    assert got.report["rc_quorums"] == 0 and got.report["prepared"] == got.report["prepared_first"] == 9
    assert got.report["locked_open"] == got.report["cert_unprepared"] == 0


def test_hostile_and_empty_streams_have_empty_rows():
    """the observer test's random bytes, empty frames and 0xffffffff prefixes, and an empty stream: return 0, rows empty"""
    from bftsim.runtime import Simulator
    cfg = TC.handmade()["cfg"]
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 900, 200)]
    frames += [b""] * 70 + [b"\xff\xff\xff\xff" + bytes(40), b"\xff\xff\xff\xff", b"\x00\x00\x00\x00", bytes(3)]
    frames.append(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())
    big = bytearray(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())
    big[:4] = (len(big) - 4).to_bytes(4, "big")
    frames.append(bytes(big))
    stream, off, _ = AR.appended(b"", np.zeros(1, np.uint64), frames)
    f0 = np.array([0, 100, 100, len(frames)], np.uint64)                 # an empty instance too
    sim = Simulator(cfg)
    try:
        got = sim.timeline_trace(_tr(stream, off, f0))
        empty = sim.timeline_trace(_tr(b"", np.zeros(1, np.uint64), np.zeros(1, np.uint64)))
    finally:
        sim.close()
    for g in (got, empty):
        assert g.report == EMPTY_REPORT
        assert (g.prep_round == 0xffff).all() and (g.rc_max_round == 0xffff).all() and (g.rc_top_round == 0xffff).all()
        for k in ("prep_digest", "prep_voters", "prep_frame", "prep_quorums", "rc_quorums", "rc_max_frame", "rc_frames", "flags",
                  "inst_flags"):
            assert not getattr(g, k).any(), k
        assert (g.open_heights == 1).all()
    assert got.audit.report["undecodable"] == len(frames) and got.n == 3 and empty.n == 0


def test_refused_calls_write_nothing():
    from bftsim import _abi, runtime
    c = TC.handmade()
    sim = runtime.Simulator(c["cfg"])
    try:
        L = runtime.lib()
        stream = np.frombuffer(c["stream"], np.uint8)
        off, f0 = c["off"], c["f0"]
        F, n = len(off) - 1, len(f0) - 1
        o, arrs = _abi.alloc_timeline(n, c["heights"])
        ao, aarrs = _abi.alloc_audit(F, n, c["heights"])
        rep, arep = _abi.CTimelineReport(), _abi.CAuditReport()
        rep.prepared, arep.frames = 77, 78
        for a in list(arrs.values()) + list(aarrs.values()):
            a.view(np.uint8)[...] = 7

        def call(out_p=ctypes.byref(o), rep_p=ctypes.byref(rep), heights=c["heights"], frames=F):
            return L.bftsim_timeline_trace(sim.h, stream.ctypes.data, len(stream), off.ctypes.data, frames, f0.ctypes.data, n,
                                           heights, 0, 0, out_p, ctypes.byref(ao), ctypes.byref(arep), rep_p)

        for rc in (call(out_p=None), call(rep_p=None), call(heights=0), call(frames=F - 1)):
            assert rc == -1
        assert L.bftsim_timeline_last_trace(sim.h, 0, 1, 0, 0, ctypes.byref(o), ctypes.byref(ao), ctypes.byref(arep),
                                            ctypes.byref(rep)) == -1        # no kept trace
        assert rep.prepared == 77 and arep.frames == 78
        assert all((a.view(np.uint8) == 7).all() for a in list(arrs.values()) + list(aarrs.values()))
        assert call() == 0 and rep.prepared == 13 and arep.frames == F
        assert np.array_equal(arrs["flags"].reshape(n, -1), c["want"]["flags"])
    finally:
        sim.close()
