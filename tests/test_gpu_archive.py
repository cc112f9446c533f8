"""GPU: the archiver (include/bftsim.h bftsim_archive_trace / bftsim_archive_last_trace, SPEC.md §11e): the ledger of a
frame stream's certified heights, assembled on the device from the bytes alone. Small shapes equal the independent
Python archiver (tests/archive_ref.py) array for array and slot for slot, hostile variants included; every archived
ledger goes through the library's importer, whose verdict equals the Python importer's (tests/ledger_ref.py); larger
ones, from real runs, are checked by structure plus the importer."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

import archive_cases as AC      # first: it puts oracle/ on the path
import archive_ref as ARC
import audit_ref as AR
import ledger_ref as LR
import trace_ref as TR
from bftsim.configs import BftConfig, cfg3, cfg4

pytestmark = pytest.mark.gpu


def _tr(stream, off, f0):
    return SimpleNamespace(stream=np.frombuffer(bytes(stream), np.uint8), frame_off=np.asarray(off, np.uint64),
                           inst_frame0=np.asarray(f0, np.uint64))


def _same_audit(a, b):
    for k in AR.ARRAYS:
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    assert a.report == b.report


def _import(sim, cfg, ledger):
    """the library's verdict on an archived ledger, asserted equal to the Python importer's"""
    hdr, lens, slot, H = ledger
    got = sim.verify_ledger(ledger)
    LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
    return got


@pytest.mark.parametrize("name", AC.NAMES)
def test_stream_equals_reference(name):
    """the library's ledger, arrays and report equal the Python archiver's; its audit outputs are bftsim_audit_trace's;
    the importer's verdict on the ledger is the Python importer's, and shows what the case was built to show"""
    from bftsim.runtime import Simulator
    c = AC.case(name)
    cfg, want = c["cfg"], c["want"]
    sim = Simulator(cfg)                      # no secrets, no set_crypto: the archiver needs neither
    try:
        tr = _tr(c["stream"], c["off"], c["f0"])
        ledger, got = sim.archive_trace(tr, max_heights=c["heights"], key_cap=c["key_cap"])
        ms = sim.archive_ms()
        audit = sim.audit_trace(tr, max_heights=c["heights"], key_cap=c["key_cap"])
        verdict = _import(sim, cfg, ledger)
    finally:
        sim.close()
    ARC.assert_same((ledger, got), want)
    AR.assert_same(got.audit, want["audit"])
    _same_audit(got.audit, audit)
    AC.check_expectations(c, got.status, verdict)
    assert all(x >= 0 for x in ms) and ms[0] > 0


def _run(cfg, secrets, first, n, log_cap=0, votes=None):
    from bftsim.runtime import Simulator
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), log_cap)
    sim.set_trace_keep(True)
    if votes is not None:
        sim.set_ledger_votes(votes)
    res = sim.run(first, n)
    rep = sim.crypto_verify()
    return sim, res, rep


def _structure(cfg, ledger, got, verdict, res, n):
    """a real run's archive: OK exactly where the observer certified, Q + 1 seals each, the run's block hashes; every
    written header verifies, or fails only for a gap below it"""
    from bftsim.ledger import AR_NONE, AR_OK
    Q = (2 * cfg.n) // 3
    cert = got.audit.cert_round != 0xffff
    assert np.array_equal(got.status == AR_OK, cert) and np.array_equal(got.status == AR_NONE, ~cert)
    assert (got.n_votes[cert] == Q + 1).all() and got.report["votes"] == (Q + 1) * int(cert.sum()) > 0
    assert got.report["headers"] == int(cert.sum()) and got.report["by_status"][2] == 0
    assert (np.asarray(ledger[1]).reshape(got.status.shape)[~cert] == 0).all()
    allowed = {LR.OK, LR.NO_PARENT, LR.BAD_PARENT}
    for i in range(n):
        assert int(got.archived_height[i]) == int(np.argmin(np.append(cert[i], False)))
        for x in range(cfg.heights):
            if not cert[i, x]:
                assert verdict.status[i, x] == LR.ABSENT
                continue
            assert np.array_equal(verdict.block_hash[i, x], res["block_hash"][i, x]), (i, x)
            assert int(verdict.status[i, x]) in allowed, (i, x, verdict.names(i))
            if verdict.status[i, x] in (LR.NO_PARENT, LR.BAD_PARENT):
                assert not cert[i, :x].all(), (i, x)
            assert sorted(verdict.voter_list(i, x + 1)) == verdict.voter_list(i, x + 1)
    print("archive", got.report, "import", verdict.report)


@pytest.mark.parametrize("name", ["n65-lossy", "n100", "cfg3"])
def test_real_runs_archive_and_verify(name):
    """N = 65 at 5 % drops (44 votes), N = 100 at 2 heights (67 votes: two lane rounds), cfg3's shape at 4 instances x 3
    heights with 21 Byzantine validators (heights without a byte-level certificate are NONE)"""
    if name == "n65-lossy":
        cfg, sec = LR.keyed(BftConfig(n=65, heights=2, seed=9, drop_ppm=50_000), 4)
        n, cap = 2, 0
    elif name == "n100":
        cfg, sec = LR.keyed(cfg4(100, heights=2), 5)
        n, cap = 1, 0
    else:
        cfg, sec = LR.keyed(cfg3(heights=3), 3)
        n, cap = 4, 16384
    sim, res, rep = _run(cfg, sec, 0, n, log_cap=cap)
    try:
        ledger, got = sim.archive_last_trace()
        verdict = _import(sim, cfg, ledger)
    finally:
        sim.close()
    assert got.audit.report["frames"] == rep["messages"]
    _structure(cfg, ledger, got, verdict, res, n)
    if name != "cfg3":
        assert got.report["foreign_seals"] == 0 and (verdict.status[got.status == 0] == LR.OK).all()
        assert np.array_equal(got.archived_height, res["committed_height"].astype(np.uint64))
        assert np.array_equal(verdict.verified_height, got.archived_height)


def test_last_trace_equals_exported_and_leaves_the_run_alone():
    """archive_last_trace equals archive_trace(export_trace()) for a launch and a sub-range, byte for byte; fetch() is
    the same before and after"""
    ref = TR.reference("n4")
    from bftsim.runtime import Simulator
    sim = Simulator(ref["cfg"])
    sim.set_crypto(ref["secrets"], ref["forged"], 1024)
    sim.set_trace_keep(True)
    res = sim.run(ref["first"], 3)
    sim.crypto_verify()
    try:
        before = sim.fetch()
        whole, part = sim.archive_last_trace(), sim.archive_last_trace(1, 2)
        via, via_part = sim.archive_trace(sim.export_trace()), sim.archive_trace(sim.export_trace(1, 2))
        after = sim.fetch()
        from bftsim.runtime import BftsimError
        with pytest.raises(BftsimError):
            sim.archive_last_trace(2, 2)                                # past the launch
    finally:
        sim.close()
    for (la, a), (lb, b) in ((whole, via), (part, via_part)):
        assert la[2:] == lb[2:] and np.array_equal(la[0], lb[0]) and np.array_equal(la[1], lb[1])
        for k in ARC.ARRAYS:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.report == b.report
        _same_audit(a.audit, b.audit)
    assert np.array_equal(part[1].status, whole[1].status[1:]) and whole[1].report["headers"] == 15
    ARC.assert_same(whole, AC.case("n4")["want"])                       # the run's frames are the reference trace's
    for k in ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash"):
        assert np.array_equal(before[k], res[k]) and np.array_equal(after[k], res[k]), k


def test_against_the_exported_ledger_with_seals():
    """a lossless run without Byzantine validators (N = 4, 3 heights): the archive and export_ledger() under "seals" hold
    the same blocks, and a validator that votes in both carries the same 65 bytes (RFC 6979); the voter sets may differ,
    the observer hears the log in sender order and a Core in its own"""
    cfg, sec = LR.keyed(BftConfig(n=4, heights=3, seed=21), 7)
    sim, res, _ = _run(cfg, sec, 0, 2, votes="seals")
    try:
        exported = sim.export_ledger()
        ledger, got = sim.archive_last_trace()
        va, ve = _import(sim, cfg, ledger), sim.verify_ledger(exported)
    finally:
        sim.close()
    from bftsim.ledger import unpack
    archived = unpack(ledger)
    assert (got.status == 0).all() and (va.status == LR.OK).all() and (ve.status == LR.OK).all()
    assert np.array_equal(va.block_hash, ve.block_hash) and np.array_equal(va.block_hash, res["block_hash"])
    both = 0
    for i in range(2):
        for x in range(3):
            a = dict(zip(va.voter_list(i, x + 1), LR.decode(archived[i][x])["votes"]))
            e = dict(zip(ve.voter_list(i, x + 1), LR.decode(exported[i][x])["votes"]))
            assert len(a) == 3 and len(e) >= 3
            for v in set(a) & set(e):
                assert a[v] == e[v], (i, x, v)
                both += 1
    assert both >= 2 * 3 * 2                                            # two sets of 3 among 4 share 2 at least


def test_hostile_stream_is_none_not_errors():
    """the observer test's random bytes, empty frames and 0xffffffff prefixes: nothing certified, all NONE, return 0"""
    from bftsim.runtime import Simulator
    cfg = AC.case("cfg1")["cfg"]
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
        ledger, got = sim.archive_trace(_tr(stream, off, f0))
    finally:
        sim.close()
    assert (got.status == 1).all() and (got.pp_frame == 0xffffffff).all() and not got.n_votes.any()
    assert not ledger[0].any() and not ledger[1].any() and not got.archived_height.any()
    assert got.report == dict(headers=0, by_status=[0, 18, 0], votes=0, foreign_seals=0, archived_instances=3)
    assert got.audit.report["undecodable"] == len(frames)


def test_refused_calls_write_nothing():
    from bftsim import _abi, runtime
    c = AC.case("cfg1")
    cfg = c["cfg"]
    sim = runtime.Simulator(cfg)
    try:
        L = runtime.lib()
        slot = L.bftsim_ledger_slot_bytes(cfg.n)
        stream = np.frombuffer(c["stream"], np.uint8)
        off, f0 = c["off"], c["f0"]
        hdr, lens, o, arrs = _abi.alloc_archive(1, 6, slot)
        ao, aarrs = _abi.alloc_audit(len(off) - 1, 1, 6)
        rep, arep = _abi.CArchiveReport(), _abi.CAuditReport()
        rep.headers, arep.frames = 77, 78
        hdr[...], lens[...] = 7, 7
        for a in list(arrs.values()) + list(aarrs.values()):
            a[...] = 7

        def call(hdr_p=hdr.ctypes.data, slot_b=slot, len_p=lens.ctypes.data, rep_p=ctypes.byref(rep)):
            return L.bftsim_archive_trace(sim.h, stream.ctypes.data, len(stream), off.ctypes.data, len(off) - 1, f0.ctypes.data,
                                          1, 6, 0, hdr_p, slot_b, len_p, ctypes.byref(o), ctypes.byref(ao), ctypes.byref(arep),
                                          rep_p)

        for rc in (call(hdr_p=None), call(len_p=None), call(rep_p=None), call(slot_b=slot - 8)):
            assert rc == -1
        assert rep.headers == 77 and arep.frames == 78 and (hdr == 7).all() and (lens == 7).all()
        assert all((a == 7).all() for a in list(arrs.values()) + list(aarrs.values()))
        assert call() == 0 and rep.headers == 6 and arep.frames == 71 and (arrs["status"] == 0).all()
        ARC.assert_same(((hdr, lens, slot, 6), SimpleNamespace(report={k: (list(getattr(rep, k)) if k == "by_status" else
                                                                       int(getattr(rep, k))) for k, _ in rep._fields_},
                                                               status=arrs["status"].reshape(1, 6),
                                                               pp_frame=arrs["pp_frame"].reshape(1, 6),
                                                               n_votes=arrs["n_votes"].reshape(1, 6),
                                                               archived_height=arrs["archived_height"])), c["want"])
    finally:
        sim.close()


def test_wider_slot_is_written_up_to_the_ledger_slot_only():
    """slot_bytes above bftsim_ledger_slot_bytes(n): each header at its slot's start, the library's part of the slot
    zero behind it, the caller's bytes beyond that part untouched; the importer reads the wider layout as it is"""
    from bftsim import _abi, runtime
    c = AC.case("n4")
    cfg, want = c["cfg"], c["want"]
    sim = runtime.Simulator(cfg)
    try:
        L = runtime.lib()
        own = L.bftsim_ledger_slot_bytes(cfg.n)
        slot = own + 24
        stream = np.frombuffer(c["stream"], np.uint8)
        off, f0 = c["off"], c["f0"]
        hdr, lens, o, arrs = _abi.alloc_archive(3, 6, slot)
        hdr[...] = 7
        rep = _abi.CArchiveReport()
        rc = L.bftsim_archive_trace(sim.h, stream.ctypes.data, len(stream), off.ctypes.data, len(off) - 1, f0.ctypes.data, 3, 6,
                                    0, hdr.ctypes.data, slot, lens.ctypes.data, ctypes.byref(o), None, None, ctypes.byref(rep))
        assert rc == 0 and rep.headers == 15
        verdict = _import(sim, cfg, (hdr, lens, slot, 6))
    finally:
        sim.close()
    rows = hdr.reshape(18, slot)
    assert (rows[:, own:] == 7).all()
    flat = [h for row in want["headers"] for h in row]
    for i, h in enumerate(flat):
        assert int(lens[i]) == len(h) and rows[i, :len(h)].tobytes() == h and not rows[i, len(h):own].any(), i
    assert np.array_equal(arrs["status"].reshape(3, 6), want["status"]) and (verdict.status[want["status"] == 0] == LR.OK).all()
