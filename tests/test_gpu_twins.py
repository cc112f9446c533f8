"""GPU: trace twins (include/bftsim.h bftsim_set_trace_twins / bftsim_trace_twin_counts, SPEC.md §11f): an equivocator's
second frames in the kept trace. Small shapes equal the Python reference (tests/twins_ref.py) byte for byte, and their
archive and import equal the Python chain (archive_ref, ledger_ref) array for array; cfg3's shape is checked against
the oracle's log, by the observer and against the run."""
import ctypes

import numpy as np
import pytest

import twins_ref as TW          # first: it puts oracle/ on the path
import archive_ref as ARC
import audit_ref as AR
import ledger_ref as LR
import oracle_lib as O
import trace_ref as TR
from bftsim.configs import BftConfig, cfg3

pytestmark = pytest.mark.gpu
RESULT = ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash")


def _sim(ref_or_cfg, secrets=None, forged=(), log_cap=1024, twins=True):
    from bftsim.runtime import Simulator
    if isinstance(ref_or_cfg, dict):
        ref_or_cfg, secrets, forged = ref_or_cfg["cfg"], ref_or_cfg["secrets"], ref_or_cfg["forged"]
    sim = Simulator(ref_or_cfg)
    sim.set_crypto(secrets, forged, log_cap)
    sim.set_trace_keep(True)
    sim.set_trace_twins(twins)
    return sim


def _same(tr, want):
    stream, off, meta, f0 = want
    assert np.array_equal(tr.frame_off, off)
    assert tr.stream.tobytes() == stream
    assert np.array_equal(tr.meta, meta)
    assert np.array_equal(tr.inst_frame0, f0)


def test_pinned_n7_equals_reference():
    """N = 7, byz_count 2, instances 2..4: the twinned export equals the reference's stream, offsets, meta and
    inst_frame0; a sub-range is the matching slice; the counts are the reference's; with twins off (a second verify of
    the same launch) the trace is today's"""
    ref = TW.reference("n7")
    sim = _sim(ref)
    try:
        sim.run(ref["first"], ref["n"])
        sim.crypto_verify()
        fr, by = sim.trace_sizes()
        counts = sim.trace_twin_counts()
        whole, part, last = sim.export_trace(), sim.export_trace(1, 2), sim.export_trace(2)
        sim.set_trace_twins(False)
        sim.crypto_verify()
        off_counts, plain = sim.trace_twin_counts(), sim.export_trace()
    finally:
        sim.close()
    _same(whole, TW.joined(ref))
    _same(part, TW.joined(ref, 1, 2))
    _same(last, TW.joined(ref, 2, 1))
    assert counts == ref["counts"] == (3, 12) and int(whole.twin.sum()) == 15
    assert fr.tolist() == [len(t[3]) for t in ref["inst"]] and by.tolist() == [len(t[0]) for t in ref["inst"]]
    assert off_counts == (0, 0) and not plain.twin.any()
    _same(plain, TW.joined(ref, plain=True))          # trace_ref's own frames (test_twins_cpu pins that on the CPU)


def test_lossy_forged_equals_reference():
    """N = 4, byz_count 1, drops 10 %, the forged validator Byzantine in two of the three instances: its twins are signed
    with the forged key and audit NOT_VALIDATOR; vote twins exist; the stream is the reference's"""
    ref = TW.reference("n4")
    f = ref["forged"][0]
    assert any(f in TW.byzantine_senders(TW.log_of(ref["res"], i)) for i in range(ref["n"]))
    sim = _sim(ref)
    try:
        sim.run(ref["first"], ref["n"])
        sim.crypto_verify()
        counts = sim.trace_twin_counts()
        tr = sim.export_trace()
        audit = sim.audit_last_trace()
    finally:
        sim.close()
    _same(tr, TW.joined(ref))
    assert counts == ref["counts"] and counts[1] > 0 and counts[0] > 0
    forged_twins = tr.twin & (tr.sender == f)
    assert forged_twins.any() and ((tr.flags[forged_twins] & 1) == 1).all()
    assert (audit.frame_status[forged_twins] == AR.ST_NOT_VALIDATOR).all()
    honest_twins = tr.twin & (tr.sender != f)
    assert (audit.frame_status[honest_twins] == AR.ST_OK).all()
    assert np.array_equal(audit.frame_signer[honest_twins], tr.sender[honest_twins].astype(np.int32))


def test_twins_change_nothing_the_run_reports():
    """twins are not log entries: the verify report, the checksums, fetch(), export_ledger() and stats() are the same
    with twins on and off"""
    ref = TW.reference("n7")
    got = {}
    for twins in (False, True):
        sim = _sim(ref, twins=twins)
        try:
            res = sim.run(ref["first"], ref["n"])
            rep = sim.crypto_verify()
            got[twins] = dict(res=res, rep=rep, fetch=sim.fetch(), ledger=sim.export_ledger(), stats=sim.stats(),
                              frames=int(sim.trace_sizes()[0].sum()))
        finally:
            sim.close()
    a, b = got[False], got[True]
    assert b["frames"] == a["frames"] + 15 == int(ref["res"]["mlog_n"].sum()) + 15
    assert set(a["rep"]) == set(b["rep"])
    for k, v in a["rep"].items():
        assert np.array_equal(v, b["rep"][k]), k
    for k in RESULT:
        assert np.array_equal(a["fetch"][k], b["fetch"][k]) and np.array_equal(b["fetch"][k], ref["res"][k]), k
        assert np.array_equal(a["res"][k], b["res"][k]), k
    assert a["ledger"] == b["ledger"] and a["stats"] == b["stats"]


def _want(ref, plain):
    stream, off, _, f0 = TW.joined(ref, plain=plain)
    cfg = ref["cfg"]
    arc = ARC.archive(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, cfg.heights, 0)
    return arc


def test_end_to_end_on_the_device():
    """archive_last_trace then verify_ledger, with twins on and off, against the Python observer, archiver and
    importer array for array: off, the variant-1 heights are NONE / NO_PROPOSAL and the header above a gap NO_PARENT;
    on, every height is OK and verified_height is committed_height. audit_last_trace equals audit_trace(export_trace())"""
    ref = TW.reference("n7")
    cfg, res = ref["cfg"], ref["res"]
    out = {}
    sim = _sim(ref)
    try:
        sim.run(ref["first"], ref["n"])
        for twins in (True, False):
            sim.set_trace_twins(twins)
            sim.crypto_verify()
            ledger, got = sim.archive_last_trace()
            verdict = sim.verify_ledger(ledger)
            out[twins] = (ledger, got, verdict, sim.audit_last_trace(), sim.audit_trace(sim.export_trace()))
    finally:
        sim.close()
    for twins in (True, False):
        ledger, got, verdict, a1, a2 = out[twins]
        want = _want(ref, plain=not twins)
        ARC.assert_same((ledger, got), want)
        AR.assert_same(got.audit, want["audit"])
        for k in AR.ARRAYS:
            assert np.array_equal(getattr(a1, k), getattr(a2, k)) and np.array_equal(getattr(a1, k), getattr(got.audit, k)), k
        assert a1.report == a2.report
        hdr, lens, slot, H = ledger
        LR.assert_same(verdict, LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
    _, got, verdict, _, _ = out[True]
    assert (got.status == ARC.OK).all() and (verdict.status == LR.OK).all() and not got.audit.inst_flags.any()
    assert np.array_equal(verdict.verified_height, res["committed_height"].astype(np.uint64))
    assert np.array_equal(verdict.block_hash, res["block_hash"]) and got.audit.report["conflicts"] == 0
    _, got, verdict, _, _ = out[False]
    assert got.status.tolist() == [[0, 0, 1, 0, 0, 2], [0] * 6, [0, 0, 0, 0, 1, 0]]
    assert verdict.status.tolist() == [[LR.OK, LR.OK, LR.ABSENT, LR.NO_PARENT, LR.OK, LR.ABSENT], [LR.OK] * 6,
                                       [LR.OK, LR.OK, LR.OK, LR.OK, LR.ABSENT, LR.NO_PARENT]]
    assert verdict.verified_height.tolist() == [2, 6, 4]


@pytest.mark.parametrize("name", ["cfg3", "n65"])
def test_byzantine_runs_certify_whole(name):
    """cfg3's shape (N = 64, 21 Byzantine, 4 instances x 3 heights: the 64-lane paths; instances 10..13, because with
    cfg3's big-endian seeds the round-0 proposer is validator 0 at every height, so an instance equivocates only where
    the seeded subset holds validator 0: 11, 12 and 13 do, 10 does not) and N = 65 with 21 Byzantine (the general
    kernel): the twin counts are those of the oracle's log by the reference's rule, every twin follows a
    flagged original and audits OK with its sender as the signer, and every committed height is certified with the
    run's hash. No Python signing at this size"""
    from bftsim.trace import compare
    if name == "cfg3":
        cfg, sec = LR.keyed(cfg3(heights=3), 3)
        first, n, cap = 10, 4, 16384
    else:
        cfg, sec = LR.keyed(BftConfig(n=65, heights=2, seed=9, byz_count=21), 4)
        first, n, cap = 0, 2, 16384
    assert cfg.byz_count == 21
    orc = O.run_crypto(cfg, first, n, cap=cap)
    kinds = []
    for i in range(n):
        log = TW.log_of(orc, i)
        byz = TW.byzantine_senders(log)
        kinds += [TW.needs_twin(e, byz) for e in log]
    sim = _sim(cfg, sec, (), cap, twins=False)
    try:
        res = sim.run(first, n)
        sim.crypto_verify()
        plain = sim.export_trace()
        sim.set_trace_twins(True)
        sim.crypto_verify()
        counts = sim.trace_twin_counts()
        tr = sim.export_trace()
        audit = sim.audit_last_trace()
    finally:
        sim.close()
    assert len(plain) == len(kinds) == int(orc["mlog_n"].sum()) and not plain.twin.any()
    assert counts == (kinds.count(1), kinds.count(2)) and counts[0] > 0 and counts[1] > 0
    tw = tr.twin
    assert int(tw.sum()) == sum(counts) and len(tr) == len(plain) + sum(counts)
    # the originals, in order, are the plain trace; each twin sits behind a flagged original of the same sender and code
    assert np.array_equal(tr.meta[~tw], plain.meta)
    k = np.nonzero(tw)[0]
    assert not tw[k - 1].any() and np.array_equal(tr.meta[k][:, [0, 1, 3]], tr.meta[k - 1][:, [0, 1, 3]])
    assert np.array_equal(tr.flags[k], tr.flags[k - 1] | np.uint32(1 << 16))
    want_flag = np.where(tr.code[k - 1] == 1, 4, 2)
    assert ((tr.flags[k - 1] & want_flag) != 0).all() and np.isin(tr.code[k], (1, 2, 3)).all()
    assert np.array_equal(np.nonzero(tw)[0] - np.arange(1, len(k) + 1), np.nonzero(np.array(kinds) != 0)[0])
    # the equivocating PrePrepares of the plain meta all have a twin
    assert int(((plain.code == 1) & ((plain.flags & 4) != 0)).sum()) == counts[0]
    assert (audit.frame_status == AR.ST_OK).all()
    assert np.array_equal(audit.frame_signer[tw], tr.sender[tw].astype(np.int32))
    cmp = compare(audit, res)
    assert np.array_equal(cmp["certified"], res["committed_height"]) and not cmp["missing"].any() and not cmp["different"].any()
    assert (res["committed_height"] == cfg.heights).all() and (res["variant"] == 1).any()
    for k in RESULT:
        assert np.array_equal(res[k], orc[k]), k
    print(name, "frames", len(tr), "twins", counts, "certified", cmp["certified"].tolist(), "variant", res["variant"].tolist())


def test_refused_calls_write_nothing():
    """set_trace_twins(2) is refused and changes nothing; trace_twin_counts with keep off, or before a verify, is
    refused with the outputs unwritten"""
    from bftsim import runtime
    ref = TW.reference("n7")
    L = runtime.lib()
    sim = _sim(ref)
    try:
        a, b = ctypes.c_uint64(77), ctypes.c_uint64(78)
        for bad in (2, -1, 256):
            assert L.bftsim_set_trace_twins(sim.h, bad) == -1
        with pytest.raises(runtime.BftsimError):
            sim.set_trace_twins(2)
        sim.run(ref["first"], 1)
        assert L.bftsim_trace_twin_counts(sim.h, ctypes.byref(a), ctypes.byref(b)) == -1      # no verify yet
        sim.crypto_verify()
        assert sim.trace_twin_counts() == ref["inst"][0][4]                                   # still on after the refusals
        sim.set_trace_keep(False)
        assert L.bftsim_trace_twin_counts(sim.h, ctypes.byref(a), ctypes.byref(b)) == -1      # keep off
        assert (a.value, b.value) == (77, 78)
        sim.set_trace_keep(True)
        assert L.bftsim_trace_twin_counts(sim.h, ctypes.byref(a), ctypes.byref(b)) == -1      # the kept trace is gone
        assert (a.value, b.value) == (77, 78)
    finally:
        sim.close()
