"""GPU: the importer (include/bftsim.h bftsim_verify_ledger, SPEC.md §11d): a ledger verified from its bytes on the
device. Ledgers of real runs kept with commit seals (bftsim_set_ledger_votes) verify, header for header, and are tied to
the run and to its exported trace; constructed and tampered ledgers equal the independent Python verifier
(tests/ledger_ref.py) array for array."""
import ctypes

import numpy as np
import pytest

import ledger_ref as LR         # first: it puts oracle/ on the path
import trace_ref as TR
import wire_ref as R
from bftsim.configs import BftConfig, cfg3
from bftsim.ledger import compare, pack

pytestmark = pytest.mark.gpu
(OK, ABSENT, UNDECODABLE, BAD_HEIGHT, NO_PARENT, BAD_PARENT, BAD_TIME, LACK_VOTES, BAD_VOTE, BAD_PROPOSER) = range(10)


def _gpu_vs_ref(cfg, ledger, heights=None, sim=None):
    """the library's verdict on a ledger (lists of header bytes, or packed arrays), asserted equal to the Python
    verifier's in every array and counter"""
    from bftsim.runtime import Simulator
    packed = ledger if isinstance(ledger, tuple) else pack(ledger, heights=cfg.heights if heights is None else heights)
    own = sim is None
    if own:
        sim = Simulator(cfg)                  # no secrets, no set_crypto: the importer needs neither
    try:
        got = sim.verify_ledger(packed)
    finally:
        if own:
            sim.close()
    hdr, lens, slot, H = packed
    LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
    return got


def _run(cfg, secrets, first, n, votes="seals", log_cap=0):
    from bftsim.runtime import Simulator
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), log_cap)
    sim.set_trace_keep(True)
    if votes is not None:
        sim.set_ledger_votes(votes)
    res = sim.run(first, n)
    sim.crypto_verify()
    return sim, res


def _shape(name):
    if name == "cfg1":
        ref = TR.reference("cfg1")
        return ref["cfg"], ref["secrets"], 0, 1
    if name == "n4-lossy":
        cfg, sec = LR.keyed(BftConfig(n=4, heights=15, seed=21, drop_ppm=100_000), 7)
        return cfg, sec, 3, 3
    if name == "n65-lossy":
        cfg, sec = LR.keyed(BftConfig(n=65, heights=6, seed=9, drop_ppm=50_000), 4)
        return cfg, sec, 0, 2
    cfg, sec = LR.keyed(BftConfig(n=100, heights=4, seed=5), 5)
    return cfg, sec, 0, 1


@pytest.mark.parametrize("name", ["cfg1", "n4-lossy", "n65-lossy", "n100"])
def test_sealed_ledger_of_a_run_verifies(name):
    """byz_count = 0: every header OK, verified_height = committed_height, the block hashes the run's, every voter's
    seal the seal of one of its Commit frames on the wire, and the verdict the Python verifier's"""
    cfg, secrets, first, n = _shape(name)
    sim, res = _run(cfg, secrets, first, n, log_cap=4096 if name == "n4-lossy" else 0)   # 15 heights with drops: rounds up to 8
    try:
        ledger = sim.export_ledger()
        got = _gpu_vs_ref(cfg, ledger, sim=sim)
        trace = sim.export_trace()
        fetched = sim.fetch()
    finally:
        sim.close()
    ch = res["committed_height"]
    assert ch.sum() > 0 and [len(r) for r in ledger] == [int(c) for c in ch]
    c = compare(got, res)
    assert np.array_equal(c["ok"], ch.astype(np.uint32)) and np.array_equal(c["same_hash"], c["ok"]) and c["verified_as_run"].all()
    assert np.array_equal(got.verified_height, ch.astype(np.uint64))
    assert got.report["by_status"][OK] == int(ch.sum()) and got.report["by_status"][ABSENT] == n * cfg.heights - int(ch.sum())
    assert got.report["duplicate_votes"] == 0 and got.report["verified_instances"] == n
    for k in ("committed_height", "flags", "round", "block_hash"):          # the run state is untouched
        assert np.array_equal(fetched[k], res[k]), k
    # the seals on the wire: per (instance, sender) those of its Commit frames
    wire = {}
    off, meta = trace.frame_off, trace.meta
    for k in np.nonzero(((meta[:, 1] >> 8) & 0xff) == 3)[0]:
        d = R.decode(trace.frame(int(k)))
        wire.setdefault((int(meta[k, 3]), int(meta[k, 1]) >> 16), set()).add(bytes(d["commit_seal"]))
    checked = 0
    for i in range(n):
        for x in range(1, int(ch[i]) + 1):
            votes = LR.decode(ledger[i][x - 1])["votes"]
            voters = got.voter_list(i, x)
            assert len(votes) == len(voters) == int(got.n_votes[i, x - 1]) > (2 * cfg.n) // 3
            for v, s in zip(voters, votes):                                 # ascending validator order
                assert s in wire[(i, v)], (i, x, v)
                checked += 1
    assert checked == got.report["votes"] == got.report["recoveries"]
    print(name, "votes per header", int(got.n_votes[got.n_votes > 0].min()), "..", int(got.n_votes.max()),
          "second voter word", bool(got.voters[:, :, 1].any()))
    if name in ("n65-lossy", "n100"):
        assert got.voters[:, :, 1].any()                                   # the second voter word
    if name == "n100":
        assert got.n_votes.max() > 64                                      # several rounds of a wave (N = 65: Q + 1 = 44)


def test_default_ledger_keeps_signatures_which_cannot_be_verified():
    """the reference's own votes (the Commit messages' signatures, core.rs:402-413) recover to nothing in the set over
    keccak(0x03 || block hash): every header BAD_VOTE. And the default export is byte-identical with and without an
    explicit set_ledger_votes("signatures")"""
    cfg, secrets, first, n = _shape("cfg1")
    sim, res = _run(cfg, secrets, first, n, votes=None)
    try:
        plain = sim.export_ledger()
        got = _gpu_vs_ref(cfg, plain, sim=sim)
    finally:
        sim.close()
    assert (got.status == BAD_VOTE).all() and got.report["by_status"][BAD_VOTE] == 6 and (got.verified_height == 0).all()
    assert np.array_equal(got.block_hash, res["block_hash"])
    sim, _ = _run(cfg, secrets, first, n, votes="signatures")
    try:
        named = sim.export_ledger()
        sim.set_ledger_votes("seals")                                       # read by the next crypto_verify only
        same = sim.export_ledger()
        from bftsim.runtime import BftsimError
        with pytest.raises(BftsimError):
            sim.set_ledger_votes("votes")
    finally:
        sim.close()
    assert named == plain and same == plain
    sealed, _ = _run(cfg, secrets, first, n, votes="seals")
    try:
        other = sealed.export_ledger()
    finally:
        sealed.close()
    assert other != plain
    assert [LR.encode(LR.decode(h), "nil") for h in other[0]] == [LR.encode(LR.decode(h), "nil") for h in plain[0]]


def test_cfg3_byzantine_equals_reference():
    """cfg3 x 4 heights x 4 instances (21 Byzantine): a wildcard voter's seal is over its own logged block (SPEC.md §11),
    so not every header verifies; the verdict is the Python verifier's and no status is outside OK / LACK_VOTES / BAD_VOTE"""
    cfg, secrets = LR.keyed(cfg3(heights=4), 3)
    sim, res = _run(cfg, secrets, 0, 4, log_cap=16384)
    try:
        got = _gpu_vs_ref(cfg, sim.export_ledger(), sim=sim)
    finally:
        sim.close()
    assert set(np.unique(got.status[got.status != ABSENT])) <= {OK, LACK_VOTES, BAD_VOTE} and got.report["headers"] == int(res["committed_height"].sum())
    assert np.array_equal(compare(got, res)["same_hash"], res["committed_height"].astype(np.uint32))


def test_constructed_and_tampered_ledgers():
    from bftsim.runtime import Simulator
    for case, ok in (("n256_171", True), ("n256_170", False)):
        ref = LR.reference(case)
        got = _gpu_vs_ref(ref["cfg"], ref["ledger"])
        assert (got.status == (OK if ok else LACK_VOTES)).all() and got.voter_list(0, 2) == ref["voters"]
        assert got.verified_height[0] == (2 if ok else 0) and (got.n_votes == len(ref["voters"])).all()
    sims = {}
    try:
        for name, ref, ledger, heights, want in LR.tamper_cases():
            sim = sims.setdefault(ref["cfg"].n, Simulator(ref["cfg"]))
            got = _gpu_vs_ref(ref["cfg"], ledger, heights=heights, sim=sim)
            for (i, x), st in want.items():
                assert got.status[i, x - 1] == st, (name, i, x, got.status.tolist())
    finally:
        for s in sims.values():
            s.close()


def test_hostile_buffer_is_statuses_not_errors():
    ref = LR.reference("cfg1")
    rng = np.random.default_rng(11)
    slot, H, n = 1024, 5, 40
    hdr = rng.integers(0, 256, n * H * slot, dtype=np.uint8)
    lens = rng.integers(0, slot + 1, n * H).astype(np.uint32)
    lens[::7] = slot + 1 + rng.integers(0, 1 << 31, len(lens[::7]))          # lengths above the slot: nothing is read
    lens[3::11], lens[5::13] = 1, 0
    good = ref["ledger"][0][0]
    hdr[:len(good)] = np.frombuffer(good, np.uint8)                          # one real header among them
    lens[0] = len(good)
    got = _gpu_vs_ref(ref["cfg"], (hdr, lens, slot, H))
    assert got.status[0, 0] == OK and got.verified_height[0] == 1 and (got.verified_height[1:] == 0).all()
    assert set(np.unique(got.status.reshape(-1)[1:])) <= {ABSENT, UNDECODABLE} and got.report["by_status"][UNDECODABLE] > 100
    assert got.report["votes"] == 4 and not got.block_hash.reshape(-1, 32)[1:].any()


def test_refused_calls_write_nothing_and_the_run_state_stays():
    from bftsim import _abi, runtime
    ref = LR.reference("n4")
    cfg = ref["cfg"]
    sim = runtime.Simulator(cfg)
    try:
        res = sim.run(ref["first"], ref["n"])
        hdr, lens, slot, H = pack(ref["ledger"], heights=cfg.heights)
        o, arrs = _abi.alloc_ledger(ref["n"], H)
        for a in arrs.values():
            a[...] = 7
        rep = _abi.CLedgerReport()
        rep.headers = 77
        L = runtime.lib()

        def call(hdr_p=hdr.ctypes.data, slot_b=slot, len_p=lens.ctypes.data, inst=ref["n"], heights=H, rep_p=ctypes.byref(rep)):
            return L.bftsim_verify_ledger(sim.h, hdr_p, slot_b, len_p, inst, heights, ctypes.byref(o), rep_p)

        for rc in (call(hdr_p=None), call(len_p=None), call(rep_p=None), call(slot_b=0), call(heights=0), call(heights=65536),
                   call(inst=1 << 31)):
            assert rc == -1
        assert rep.headers == 77 and all((a == 7).all() for a in arrs.values())
        assert call() == 0 and rep.headers == 12 and rep.by_status[OK] == 12 and (arrs["status"] == OK).all()
        got = sim.verify_ledger(ref["ledger"])
        ms = sim.ledger_ms()
        after = sim.fetch()
    finally:
        sim.close()
    assert (got.status == OK).all() and all(x >= 0 for x in ms) and ms[1] > 0
    for k in ("committed_height", "flags", "ticks", "views", "round", "proposer", "variant", "time_tick", "block_hash"):
        assert np.array_equal(after[k], res[k]), k


@pytest.mark.parametrize("mapping", [1, 2])
def test_both_tally_mappings_on_both_extremes(monkeypatch, mapping):
    """the A/B switch of scripts/ledger_bench.py (BFTSIM_TESTING=1 + BFTSIM_LEDGER_TALLY: 1 a lane per header, 2 a wave
    per header): either mapping gives the Python verifier's verdict on 3-vote headers and on 171-vote headers alike"""
    monkeypatch.setenv("BFTSIM_TESTING", "1")
    monkeypatch.setenv("BFTSIM_LEDGER_TALLY", str(mapping))
    for case in ("n4", "n256_171"):
        ref = LR.reference(case)
        got = _gpu_vs_ref(ref["cfg"], ref["ledger"])
        assert (got.status[got.status != ABSENT] == OK).all() and got.report["by_status"][OK] == sum(len(r) for r in ref["ledger"])
    name, ref, ledger, heights, want = [c for c in LR.tamper_cases() if c[0] == "duplicate"][0]
    got = _gpu_vs_ref(ref["cfg"], ledger, heights=heights)
    assert got.status[0, 0] == LACK_VOTES and got.report["duplicate_votes"] == 1
