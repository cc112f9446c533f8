"""GPU: the accuser (include/bftsim.h bftsim_accuse_trace / bftsim_accuse_last_trace, SPEC.md §11g): the validators that
signed two digests for one (code, height, round), each with the two frames that prove it, found on the device. The
cases of tests/test_accuse_cpu.py equal the independent Python accuser (tests/accuse_ref.py) array for array; the kept
trace equals its export; larger Byzantine runs are checked against the seeded Byzantine set and, with the library's own
statuses and signers, against the Python rule; every record's two frames alone prove the fault again (closure)."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import accuse_cases as XC       # first: it puts oracle/ on the path
import accuse_ref as XR
import audit_ref as AR
import ledger_ref as LR
import twins_ref as TW
from bftsim.configs import BftConfig, cfg3

pytestmark = pytest.mark.gpu
RESULT = ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash")


def _tr(stream, off, f0):
    return SimpleNamespace(stream=np.frombuffer(bytes(stream), np.uint8), frame_off=np.asarray(off, np.uint64),
                           inst_frame0=np.asarray(f0, np.uint64))


def _same_audit(a, b):
    for k in AR.ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.report == b.report


def _same_accusation(a, b):
    for k in ("frame_pair", "inst_accused", "inst_flags"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.records.tolist() == b.records.tolist() and a.report == b.report
    _same_audit(a.audit, b.audit)


def _closure(sim, tr, acc, heights, accepted=(AR.ST_OK,)):
    """each record's two frames as a two-frame instance of a new stream: the observer gives both OK (the hand-made
    stream's foreign seal: SEAL_FOREIGN) with one signer, the accuser finds exactly one record, (0, 1), per instance"""
    proofs = [acc.proof(tr, k) for k in range(len(acc.records))]
    stream, off, f0 = XR.stream_of([list(p) for p in proofs])
    again = sim.accuse_trace(_tr(stream, off, f0), max_heights=heights)
    n = len(proofs)
    assert np.isin(again.audit.frame_status, accepted).all()
    sg = again.audit.frame_signer.reshape(n, 2)
    assert (sg[:, 0] == sg[:, 1]).all() and sg[:, 0].tolist() == acc.records["signer"].tolist()
    assert again.report["records"] == n == len(again.records)
    assert again.records["frame_a"].tolist() == list(range(0, 2 * n, 2))
    assert again.records["frame_b"].tolist() == list(range(1, 2 * n, 2))
    assert again.records["inst"].tolist() == list(range(n))
    for k in ("round", "height", "signer", "code"):
        assert again.records[k].tolist() == acc.records[k].tolist(), k


CASES = [("handmade", "want", {}), ("handmade", "want_cap2", dict(view_cap=2)), ("handmade", "want_rec1", dict(rec_cap=1)),
         ("n7", "want", {}), ("n7 plain", "want", {}), ("n4", "want", {})]


@pytest.mark.parametrize("name,key,kw", CASES, ids=[f"{n}-{k}" for n, k, _ in CASES])
def test_stream_equals_reference(name, key, kw):
    """the library's arrays, records and report equal the Python accuser's under the same caps; the audit outputs
    passed through are bftsim_audit_trace's; every record is a proof on its own"""
    from bftsim.runtime import Simulator
    c = XC.handmade() if name == "handmade" else XC.twins(name.split()[0], name.endswith("plain"))
    sim = Simulator(c["cfg"])                 # no secrets, no set_crypto: the accuser needs neither
    try:
        tr = _tr(c["stream"], c["off"], c["f0"])
        got = sim.accuse_trace(tr, max_heights=c["heights"], **kw)
        ms = sim.accuse_ms()
        audit = sim.audit_trace(tr, max_heights=c["heights"])
        if key == "want" and len(got.records):
            _closure(sim, SimpleNamespace(frame=lambda k: bytes(tr.stream[int(tr.frame_off[k]):int(tr.frame_off[k + 1])])),
                     got, c["heights"], (AR.ST_OK, AR.ST_SEAL_FOREIGN) if name == "handmade" else (AR.ST_OK,))
    finally:
        sim.close()
    XR.assert_same(got, c[key])
    AR.assert_same(got.audit, c["want"]["audit"])
    _same_audit(got.audit, audit)
    assert [got.accused(i) for i in range(got.n)] == [XR.accused(c[key], i) for i in range(got.n)]
    assert all(x >= 0 for x in ms) and ms[0] > 0


@pytest.mark.parametrize("twins", [True, False])
def test_last_trace_equals_exported_and_leaves_the_run_alone(twins):
    """accuse_last_trace equals accuse_trace(export_trace()) for a launch and for a sub-range, and the Python accuser on
    the reference trace; fetch() and stats() are the same before and after"""
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
        whole, part = sim.accuse_last_trace(), sim.accuse_last_trace(1, 2)
        tr = sim.export_trace()
        via, via_part = sim.accuse_trace(tr), sim.accuse_trace(sim.export_trace(1, 2))
        after, stats_after = sim.fetch(), sim.stats()
        with pytest.raises(BftsimError):
            sim.accuse_last_trace(2, 2)                                 # past the launch
    finally:
        sim.close()
    _same_accusation(whole, via)
    _same_accusation(part, via_part)
    XR.assert_same(whole, XC.twins("n7", not twins)["want"])            # the run's frames are the reference trace's
    assert whole.report["records"] == (15 if twins else 0)
    first_of_1 = int(tr.inst_frame0[1])
    tail = whole.records[whole.records["inst"] >= 1]
    assert part.records["frame_b"].tolist() == (tail["frame_b"] - first_of_1).tolist()
    assert part.records["inst"].tolist() == (tail["inst"] - 1).tolist()
    if twins:
        a, b = whole.proof(tr, 0)
        assert a == tr.frame(30) and b == tr.frame(31) and a != b
    assert stats == stats_after
    for k in RESULT:
        assert np.array_equal(before[k], res[k]) and np.array_equal(after[k], res[k]), k


@pytest.mark.parametrize("name", ["cfg3", "n65"])
def test_byzantine_runs(name):
    """cfg3's shape at instances 10..13 x 3 heights (N = 64, 21 Byzantine: 387 twins among 1,935 frames) and N = 65 with
    21 Byzantine (the second bitmap word, first rows past 64): the accused are within the seeded Byzantine set, every
    twin's sender is accused, the outputs equal the Python rule over the library's own statuses and signers, and every
    record proves its fault alone. No Python signing at this size"""
    from bftsim.runtime import Simulator
    if name == "cfg3":
        cfg, sec = LR.keyed(cfg3(heights=3), 3)
        first, n, cap = 10, 4, 16384
    else:
        cfg, sec = LR.keyed(BftConfig(n=65, heights=2, seed=9, byz_count=21), 4)
        first, n, cap = 0, 2, 16384
    sim = Simulator(cfg)
    sim.set_crypto(sec, (), cap)
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    try:
        sim.run(first, n)
        sim.crypto_verify()
        tr = sim.export_trace()
        got = sim.accuse_last_trace()
        _closure(sim, tr, got, cfg.heights)
    finally:
        sim.close()
    tw = tr.twin
    if name == "cfg3":
        assert (len(tr), int(tw.sum())) == (1935, 387)
    assert (got.audit.frame_status == AR.ST_OK).all() and int(tw.sum()) > 0
    for i in range(n):
        assert set(got.accused(i)) <= XC.seeded_byz(cfg, first + i), i
        assert {int(v) for v in tr.sender[tw & (tr.instance == i)]} <= set(got.accused(i)), i
    assert got.report["records"] == len(got.records) <= int(tw.sum()) and got.report["view_overflows"] == 0
    assert got.report["accused"] == sum(len(got.accused(i)) for i in range(n))
    want = XR.accuse(tr.stream.tobytes(), tr.frame_off, tr.inst_frame0, cfg.addresses, cfg.seed_byte_order == 1, cfg.heights,
                     audit=dict(frame_status=got.audit.frame_status, frame_signer=got.audit.frame_signer))
    XR.assert_same(got, dict(want, audit=None))
    print(name, "frames", len(tr), "twins", int(tw.sum()), got.report, "accused", [got.accused(i) for i in range(n)])


def test_hostile_stream_has_no_records():
    """the observer test's random bytes, empty frames and 0xffffffff prefixes: return 0, nothing accused"""
    from bftsim.runtime import Simulator
    cfg = XC.handmade()["cfg"]
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
        got = sim.accuse_trace(_tr(stream, off, f0))
        empty = sim.accuse_trace(_tr(b"", np.zeros(1, np.uint64), np.zeros(1, np.uint64)))
    finally:
        sim.close()
    for g in (got, empty):
        assert g.report == dict(records=0, by_code=[0, 0, 0], accused=0, accused_instances=0, view_overflows=0)
        assert (g.frame_pair == 0xffffffff).all() and not g.inst_accused.any() and not g.inst_flags.any() and len(g.records) == 0
    assert got.audit.report["undecodable"] == len(frames)


def test_refused_calls_write_nothing():
    from bftsim import _abi, runtime
    c = XC.handmade()
    sim = runtime.Simulator(c["cfg"])
    try:
        L = runtime.lib()
        stream = np.frombuffer(c["stream"], np.uint8)
        off, f0 = c["off"], c["f0"]
        F, n = len(off) - 1, len(f0) - 1
        o, arrs = _abi.alloc_accuse(F, n)
        ao, aarrs = _abi.alloc_audit(F, n, c["heights"])
        rep, arep = _abi.CAccuseReport(), _abi.CAuditReport()
        rep.records, arep.frames = 77, 78
        for a in list(arrs.values()) + list(aarrs.values()):
            a.view(np.uint8)[...] = 7
        no_recs = _abi.CAccuseOut()
        no_recs.frame_pair, no_recs.rec_cap = arrs["frame_pair"].ctypes.data, 4

        def call(out_p=ctypes.byref(o), rep_p=ctypes.byref(rep), heights=c["heights"], frames=F):
            return L.bftsim_accuse_trace(sim.h, stream.ctypes.data, len(stream), off.ctypes.data, frames, f0.ctypes.data, n,
                                         heights, 0, 0, out_p, ctypes.byref(ao), ctypes.byref(arep), rep_p)

        for rc in (call(out_p=None), call(rep_p=None), call(out_p=ctypes.byref(no_recs)), call(heights=0), call(frames=F - 1)):
            assert rc == -1
        assert L.bftsim_accuse_last_trace(sim.h, 0, 1, 0, 0, ctypes.byref(o), ctypes.byref(ao), ctypes.byref(arep),
                                          ctypes.byref(rep)) == -1          # no kept trace
        assert rep.records == 77 and arep.frames == 78
        assert all((a.view(np.uint8) == 7).all() for a in list(arrs.values()) + list(aarrs.values()))
        assert call() == 0 and rep.records == 8 and arep.frames == F
        assert arrs["records"][:8].tolist() == c["want"]["records"].tolist()
        assert np.array_equal(arrs["frame_pair"], c["want"]["frame_pair"])
        assert (arrs["records"][8:].view(np.uint8) == 7).all()              # only the records found are written
    finally:
        sim.close()
