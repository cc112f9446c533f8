"""CPU: trace twins (SPEC.md §11f). The Python reference alone (tests/twins_ref.py) shows what the twins are for: the
plain trace of the pinned N = 7 case has no certificate, or no proposal, at the heights that commit a variant-1 block,
and the twinned trace archives and imports whole. Then the host build of the mark and merge steps
(consensus-rs_amd/csrc/bft_twins.h, tests/emu/twins_host.cpp) and of the frame emitter against that reference, the
golden pin, and the steps as a stand-alone program under ASan + UBSan."""
import ctypes
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import twins_ref as TW          # first: it puts oracle/ on the path
import archive_ref as ARC
import ledger_ref as LR
import oracle_lib as O
import trace_lib as TL
import trace_ref as TR
import twins_lib as TWL

HERE = os.path.dirname(__file__)
PIN = json.load(open(os.path.join(HERE, "golden", "trace_twins_n7.json")))


@pytest.fixture(scope="module")
def n7():
    return TW.reference("n7")


def seeded_byz(cfg, inst) -> set:
    """the oracle's draw of SPEC.md §5"""
    c, keep = O.to_orc(cfg)
    out = (ctypes.c_uint64 * 4)()
    O.lib().orc_byz_mask(ctypes.byref(c), ctypes.c_uint32(inst), out)
    del keep
    return {v for v in range(cfg.n) if (out[v >> 6] >> (v & 63)) & 1}


def expected_index(mlog, mlog_n, byz_of):
    """the merged frame index by the reference's rule: fmap [frames], if0 [n + 1], kinds [messages]"""
    fmap, if0, kinds, m = [], [0], [], 0
    for i in range(len(mlog_n)):
        for e in mlog[i, :int(mlog_n[i])]:
            k = TW.needs_twin(e, byz_of(i))
            kinds.append(k)
            fmap.append(m)
            if k:
                fmap.append(m | TWL.F_TWIN)
            m += 1
        if0.append(len(fmap))
    return np.array(fmap, np.uint64), np.array(if0, np.uint64), kinds


def test_reference_pinned_to_golden(n7):
    """the Python reference alone: frame count, bytes and Keccak-256 of the twinned stream of instances 2..4"""
    stream, off, meta, f0 = TW.joined(n7)
    assert len(off) - 1 == PIN["frames"] and len(stream) == PIN["bytes"]
    assert O.keccak256(stream).hex() == PIN["keccak256"]
    assert list(n7["counts"]) == PIN["twins"] and sum(PIN["twins"]) == int((meta[:, 2] & TW.TWIN != 0).sum())
    plain = TW.joined(n7, plain=True)
    assert len(plain[1]) - 1 == PIN["frames"] - sum(PIN["twins"]) and O.keccak256(plain[0]).hex() == PIN["plain_keccak256"]
    # the plain trace inside the twinned reference is trace_ref's own
    for i in range(n7["n"]):
        assert plain_instance(n7, i) == n7["plain"][i][0]


def plain_instance(ref, i) -> bytes:
    return TR.instance_trace(ref["cfg"], ref["first"], ref["res"], i, ref["secrets"], ref["forged"])[0]


def test_reference_verdicts_plain_and_twinned(n7):
    """what the issue derived, observed: the plain trace is not OK at the variant-1 heights (no certificate at (2, 3)
    and (4, 5), a certificate without a proposal at (2, 6)); with twins every committed height is certified with the
    run's hash, nothing conflicts, the archiver and the importer say OK throughout"""
    cfg, res = n7["cfg"], n7["res"]
    assert res["variant"].tolist() == [[0, 0, 1, 0, 0, 1], [0] * 6, [0, 0, 0, 0, 1, 0]] and (res["committed_height"] == 6).all()
    v1 = res["variant"] == 1
    p = TW.verdicts(cfg, res, *[TW.joined(n7, plain=True)[k] for k in (0, 1, 3)])
    assert (p["archive"]["status"][v1] != ARC.OK).all() and (p["archive"]["status"][~v1] == ARC.OK).all()
    assert p["archive"]["status"].tolist() == [[0, 0, 1, 0, 0, 2], [0] * 6, [0, 0, 0, 0, 1, 0]]
    assert p["certified"].astype(int).tolist() == [[1, 1, 0, 1, 1, 1], [1] * 6, [1, 1, 1, 1, 0, 1]]
    assert p["ledger"]["status"].tolist() == [[LR.OK, LR.OK, LR.ABSENT, LR.NO_PARENT, LR.OK, LR.ABSENT], [LR.OK] * 6,
                                              [LR.OK, LR.OK, LR.OK, LR.OK, LR.ABSENT, LR.NO_PARENT]]
    assert p["ledger"]["verified_height"].tolist() == [2, 6, 4]
    t = TW.verdicts(cfg, res, *[TW.joined(n7)[k] for k in (0, 1, 3)])
    assert t["certified"].all() and not t["archive"]["audit"]["inst_flags"].any()
    assert t["archive"]["audit"]["report"]["conflicts"] == 0 and t["archive"]["audit"]["report"]["ok"] == PIN["frames"]
    assert (t["archive"]["status"] == ARC.OK).all() and (t["ledger"]["status"] == LR.OK).all()
    assert np.array_equal(t["ledger"]["verified_height"], res["committed_height"].astype(np.uint64))
    assert np.array_equal(t["ledger"]["block_hash"], res["block_hash"])


def test_log_rule_equals_the_seeded_subset(n7):
    """the reference's Byzantine set (senders of flagged entries) against the draw of SPEC.md §5: never outside it, and
    the same for every validator that ever proposes, so both mark the same entries"""
    cfg, res = n7["cfg"], n7["res"]
    for i in range(n7["n"]):
        log = TW.log_of(res, i)
        by_log, seeded = TW.byzantine_senders(log), seeded_byz(cfg, n7["first"] + i)
        assert by_log <= seeded and len(seeded) == cfg.byz_count
        proposers = {(int(e[4]) >> 24) & 0xff | ((int(e[5]) & 1) << 8) for e in log if (int(e[1]) >> 8) & 0xff == 1}
        assert proposers & by_log == proposers & seeded
        assert [TW.needs_twin(e, by_log) for e in log] == [TW.needs_twin(e, seeded) for e in log]


def test_host_mark_and_merge_equal_reference(n7):
    """the host build of bft_twins.h over the oracle's log: the Byzantine sets, the marks, the counts, the merged frame
    order, each instance's first frame, and the meta the merged index implies"""
    cfg, res = n7["cfg"], n7["res"]
    got = TWL.index(res["mlog"], res["mlog_n"], cfg.seed, n7["first"], cfg.n, cfg.byz_count)
    fmap, if0, kinds = expected_index(res["mlog"], res["mlog_n"], lambda i: TW.byzantine_senders(TW.log_of(res, i)))
    for i in range(n7["n"]):
        assert {v for v in range(cfg.n) if (int(got["byz"][i, v >> 6]) >> (v & 63)) & 1} == seeded_byz(cfg, n7["first"] + i)
    assert got["kind"].tolist() == kinds and got["counts"] == n7["counts"] == (kinds.count(1), kinds.count(2))
    assert np.array_equal(got["fmap"], fmap) and np.array_equal(got["if0"], if0)
    _, _, meta, f0 = TW.joined(n7)
    assert np.array_equal(got["if0"], f0)
    dense = np.concatenate([TW.log_of(res, i) for i in range(n7["n"])])
    inst = np.concatenate([np.full(int(res["mlog_n"][i]), i) for i in range(n7["n"])])
    m = (got["fmap"] & np.uint64(TWL.F_TWIN - 1)).astype(np.int64)
    tw = (got["fmap"] >> np.uint64(63)).astype(np.uint32)
    mine = np.stack([dense[m, 0], dense[m, 1], dense[m, 6] | (tw << np.uint32(16)), inst[m].astype(np.uint32)], axis=1)
    assert np.array_equal(mine.astype(np.uint32), meta)


def test_emitter_equals_reference_on_twins(n7):
    """the host build of the frame emitter over the reference's twin messages, byte for byte"""
    seen = set()
    for stream, off, meta, ms, _ in n7["inst"]:
        for k, m in enumerate(ms):
            if not m["twin"]:
                continue
            want = stream[int(off[k]):int(off[k + 1])]
            got, n, counted = TL.frame(m)
            assert counted == n == len(want) and got == want, (k, m["code"])
            assert ms[k - 1]["meta"][:2] == m["meta"][:2] and ms[k - 1]["meta"][2] | TW.TWIN == m["meta"][2]
            assert ms[k - 1]["digest"] != m["digest"] and ms[k - 1]["sig"] != m["sig"] and ms[k - 1]["key"] == m["key"]
            seen.add(m["code"])
    assert seen == {1, 2, 3}


def _variants(n7):
    cfg, res = n7["cfg"], n7["res"]
    n, cap = res["mlog"].shape[0], 128
    log = np.ascontiguousarray(res["mlog"][:, :cap])
    assert int(res["mlog_n"].max()) <= cap
    yield "case", log, res["mlog_n"], cfg.byz_count, lambda i: seeded_byz(cfg, n7["first"] + i)
    full = log.copy()
    code = (full[:, :, 1] >> 8) & 0xff
    full[:, :, 6] |= np.where(code == 1, 4, 2).astype(np.uint32)          # every PrePrepare equivocates, every vote is wild
    yield "every entry flagged", full, res["mlog_n"], cfg.n, lambda i: set(range(cfg.n))
    none = log.copy()
    none[:, :, 6] &= np.uint32(~6 & 0xffffffff)
    yield "no entry flagged", none, res["mlog_n"], cfg.byz_count, lambda i: seeded_byz(cfg, n7["first"] + i)
    yield "zero messages", log, np.zeros(n, np.uint32), cfg.byz_count, lambda i: set()


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_index_program_under_asan_ubsan(n7):
    """the stand-alone program (its own main, run directly): the case's log, every entry flagged, none flagged and no
    messages at all, each into heap buffers of exactly the counted sizes"""
    exe = TWL.build_san()
    cfg = n7["cfg"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    for name, log, cnt, byz_count, byz_of in _variants(n7):
        fmap, if0, kinds = expected_index(log, cnt, byz_of)
        M = int(np.asarray(cnt).sum())
        if name == "every entry flagged":
            assert len(fmap) == 2 * M
        elif name != "case":
            assert len(fmap) == M
        r = subprocess.run([exe], input=TWL.san_input(log, cnt, cfg.seed, n7["first"], cfg.n, byz_count, fmap, if0),
                           capture_output=True, env=env, timeout=120)
        assert r.returncode == 0, (name, r.returncode, r.stdout[-2000:], r.stderr[-4000:])
        assert r.stdout.decode().strip() == f"ok {M} messages {kinds.count(1)} pp twins {kinds.count(2)} vote twins", name
        assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_argument_errors_without_a_gpu():
    """the C ABI of the twins is exported and refuses a null handle, writing nothing"""
    from bftsim import runtime
    L = runtime.lib()
    a, b = ctypes.c_uint64(77), ctypes.c_uint64(78)
    assert L.bftsim_set_trace_twins(None, 1) == -1 and L.bftsim_set_trace_twins(None, 2) == -1
    assert L.bftsim_trace_twin_counts(None, ctypes.byref(a), ctypes.byref(b)) == -1 and (a.value, b.value) == (77, 78)
    assert L.bftsim_trace_twins_last_ms(None, None, None, None) == -1
    for name in ("set_trace_twins", "trace_twin_counts"):
        assert callable(getattr(runtime.Simulator, name))


def test_trace_twin_column():
    from bftsim.trace import FLAG_TWIN, Trace
    meta = np.array([[7, 2 | (3 << 8) | (5 << 16), 2, 0], [7, 2 | (3 << 8) | (5 << 16), 2 | FLAG_TWIN, 0]], np.uint32)
    t = Trace(np.zeros(2, np.uint8), np.array([0, 1, 2], np.uint64), meta, np.array([0, 2], np.uint64))
    assert FLAG_TWIN == 1 << 16 and t.twin.tolist() == [False, True] and t.twin.dtype == bool
    assert t.flags.tolist() == [2, 2 | FLAG_TWIN] and t.sender.tolist() == [5, 5]
