"""GPU: every header-hash path at every MessagePack width of the header's `time` field (1, 2, 3, 5 and 9 bytes) and
across a change of width inside a chain (tests/time_cases.py). Every other GPU test runs at the default genesis time
and block period, where `time` is the 5-byte 0xce form at every height; each width moves everything behind it in the
suffix, the splice offset and the Keccak pad byte. The oracle these runs are compared with is pinned to the msgpack
package at the same widths by tests/test_oracle_kat.py, and every case first asserts on the oracle's result that it has
the sizes it is there for.

a. plain runs of every kernel (general, segment, FAST + canonical_run, resume, full kernel alone, both seed byte orders)
b. windowed streams
c. the pipelined chain kernels (wave, pair, predicted pair, lane in all its modes, little-endian predictions)
d. the ledger export's header bytes
e. real-crypto mode: the trace, its audit and archive, the sealed ledger through the importer

Not here: 3-block headers. With a 9-byte time and a 5-byte height a header is 248 bytes on average (sd 4) and needs 273
for a third rate block, about 1e-9 per header, and it cannot be forced through the ABI since the parent is always a real
Keccak output. The host-side emu_splice_check / emu_wave_chain_check (tests/test_emu_parity.py) keep that case."""
import ctypes

import numpy as np
import pytest

import oracle_lib as O
import time_cases as T
from bftsim.distributed import stats_from_result
from parity_util import FIELDS, assert_same

pytestmark = pytest.mark.gpu


def _sim(cfg):
    from bftsim.runtime import Simulator
    return Simulator(cfg)


def _check_stats(st, cfg, first, n, ref, what):
    want = stats_from_result(ref)
    for k in ("instances", "committed_heights", "views", "ticks", "flagged", "round_hist"):
        assert st[k] == want[k], (what, k, st[k], want[k])
    lat = O.run_stream(cfg, first, n, threads=8)["latency_hist"]
    assert st["latency_hist"] == [int(x) for x in lat], (what, "latency_hist")


def _run_check(cfg, first, n, ref, fast=True):
    sim = _sim(cfg)
    try:
        if not fast:
            sim.set_fast(False)
        got = sim.run(first, n)
        st = sim.stats()
    finally:
        sim.close()
    assert_same(ref, got, cfg.name)
    assert all(np.array_equal(ref[k], got[k]) for k in FIELDS)
    _check_stats(st, cfg, first, n, ref, cfg.name)


# ---- a. plain runs
@pytest.mark.parametrize("shape", list(T.PLAIN))
@pytest.mark.parametrize("case", T.SHORT_IDS)
def test_plain_run(case, shape):
    _run_check(*T.reference("PLAIN", shape, case))


@pytest.mark.parametrize("case", T.SHORT_IDS)
def test_full_kernel_alone_n64(case):
    _run_check(*T.reference("NO_FAST", "n64-byz21", case), fast=False)


@pytest.mark.parametrize("shape", list(T.LONG))
def test_time_and_height_change_width_together(shape):
    """t-0: `height` and `time` go from 1 to 2 to 3 bytes, at the same blocks on a lossless chain"""
    cfg, first, n, ref = T.reference("LONG", shape, "t-0")
    assert (ref["committed_height"] >= 260).all()
    _run_check(cfg, first, n, ref)


def test_height_crosses_65536():
    """N = 4, 2 instances, 65,600 lossless heights at t-0: the 5-byte form of `height` (and of `time`) on the device.
    The oracle's run of it takes 0.55 s on one CPU thread."""
    from bftsim.configs import BftConfig
    cfg = T.with_time(BftConfig(n=4, heights=65_600, seed=2, name="n4-65600"), "t-0")
    ref = O.run(cfg, 0, 2)
    T.assert_case("t-0", cfg, ref)
    assert (ref["committed_height"] == 65_600).all() and 5 in T.time_sizes(cfg, ref)[0]
    _run_check(cfg, 0, 2, ref)


# ---- b. windowed streams
@pytest.mark.parametrize("case", T.STREAM_IDS)
def test_windowed_stream(case):
    mk, first, n, window = T.STREAM
    cfg = T.with_time(mk(), case)
    T.assert_case(case, cfg, O.run(cfg, first, n, threads=8))
    sim = _sim(cfg)
    try:
        got = sim.run_stream(first, n, window=window)
    finally:
        sim.close()
    ref = O.run_stream(cfg, first, n, threads=8)
    for k in ("committed_height", "flags", "ticks", "views", "tip_hash", "round_hist", "latency_hist"):
        assert np.array_equal(ref[k], got[k]), (cfg.name, k)
    assert not (got["flags"] & 64).any()


# ---- c. pipelined chain kernels: 5 launches over distinct ranges, the last one compared (the ring wraps at depth 3
# only; the depth-6 modes reuse no set, time_cases.CHAIN_MODES)
def _chain(mode, case, monkeypatch):
    _, _, depth, batch, env = T.CHAIN_MODES[mode]
    monkeypatch.setenv("BFTSIM_TESTING", "1")
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cfg, first, n, ref = T.reference("CHAIN", mode, case)
    sim = _sim(cfg)
    try:
        sim.set_pipeline(True, depth)
        if batch:
            sim.set_hash_batch(batch)
        sim.prepare(n)
        for k in range(T.LAUNCHES):
            sim.launch(k * n)
        sim.sync()
        got = sim.fetch()
        st = sim.stats()
    finally:
        sim.close()
    assert_same(ref, got, f"{mode} {case}")
    _check_stats(st, cfg, first, n, ref, f"{mode} {case}")


@pytest.mark.parametrize("mode", T.CHAIN_MODE_IDS)
@pytest.mark.parametrize("case", T.CHAIN_IDS)
def test_chain_kernels(case, mode, monkeypatch):
    _chain(mode, case, monkeypatch)


@pytest.mark.parametrize("case", T.CHAIN_REST)
def test_inline_predicted_lane_chain_remaining_rows(case, monkeypatch):
    _chain(T.TIGHTEST + "-260" if case == "t-0" else T.TIGHTEST, case, monkeypatch)


# ---- d. ledger export
def _expected_header(cfg, inst, x, prop, var, tick, prev):
    L = O.lib()
    u32, u64, cp = ctypes.c_uint32, ctypes.c_uint64, ctypes.c_char_p
    L.orc_tx_hash.argtypes = [u64, u32, u32, u32, u32, ctypes.c_void_p]
    tx = (ctypes.c_uint8 * 32)()
    L.orc_tx_hash(cfg.seed, inst, x, prop, var, tx)
    extra = b"Coinse base"
    buf = (ctypes.c_uint8 * 512)()
    time = cfg.genesis_time + cfg.block_period * (tick + 1)
    n = L.orc_encode_header(buf, prev, bytes(cfg.addresses[prop]), bytes(tx), x, 0, 0, time, extra, len(extra))
    return bytes(buf[:n])


@pytest.mark.parametrize("shape", list(T.LEDGER))
@pytest.mark.parametrize("case", T.LEDGER_IDS)
def test_exported_headers(case, shape):
    """the header bytes the GPU exports equal the oracle's encoder's, hash to the run's block hashes, and have the
    lengths the case's sizes of `time` give"""
    import trace_ref as TR
    cfg, first, n, ref = T.reference("LEDGER", shape, case)
    sim = _sim(cfg)
    try:
        res = sim.run(first, n)
        hdrs = sim.export_headers(n)
    finally:
        sim.close()
    assert_same(ref, res, cfg.name)
    genesis = TR.genesis_hash(cfg)
    lengths = set()
    for i in range(n):
        ch = int(ref["committed_height"][i])
        prev = genesis
        for x in range(1, cfg.heights + 1):
            h = hdrs[i][x - 1]
            if x > ch:
                assert h == b""
                continue
            want = _expected_header(cfg, first + i, x, int(ref["proposer"][i, x - 1]), int(ref["variant"][i, x - 1]),
                                    int(ref["time_tick"][i, x - 1]), prev)
            assert h == want, (cfg.name, i, x)
            prev = O.keccak256(h)
            assert prev == bytes(ref["block_hash"][i, x - 1]), (cfg.name, i, x)
            lengths.add(len(h))
    assert len(lengths) > 1


# ---- e. real-crypto mode
def _same_trace(tr, want):
    stream, off, meta, f0 = want
    assert np.array_equal(tr.frame_off, off)
    assert tr.stream.tobytes() == stream
    assert np.array_equal(tr.meta, meta)
    assert np.array_equal(tr.inst_frame0, f0)


def _crypto_run(ref, twins=False):
    """a run in real-crypto mode with the trace and the commit seals kept -> everything group e compares"""
    from bftsim.runtime import Simulator
    cfg = ref["cfg"]
    sim = Simulator(cfg)
    try:
        sim.set_crypto(ref["secrets"], (), 4096)
        sim.set_trace_keep(True)
        sim.set_trace_twins(twins)
        sim.set_ledger_votes("seals")
        res = sim.run(ref["first"], ref["n"])
        sim.crypto_verify()
        out = dict(res=res, trace=sim.export_trace(), audit=sim.audit_last_trace())
        out["archive"] = sim.archive_last_trace()
        out["archive_verdict"] = sim.verify_ledger(out["archive"][0])
        out["exported"] = sim.export_ledger()
        out["exported_verdict"] = sim.verify_ledger(out["exported"])
    finally:
        sim.close()
    return out


def _check_crypto(ref, got, joined, whole=True):
    """the trace byte for byte; its audit and archive against the Python observer and archiver; the archive and the
    exported sealed ledger through the importer, every committed header OK and the verdicts the Python importer's"""
    import archive_ref as ARC
    import audit_ref as AR
    import ledger_ref as LR
    import trace_ref as TR
    from bftsim.ledger import pack
    cfg, res, want = ref["cfg"], ref["res"], ref["want"]
    for k in FIELDS:
        assert np.array_equal(got["res"][k], res[k]), k
    _same_trace(got["trace"], joined)
    AR.assert_same(got["audit"], want["archive"]["audit"])
    ARC.assert_same(got["archive"], want["archive"])
    LR.assert_same(got["archive_verdict"], want["ledger"])
    hdr, lens, slot, H = pack(got["exported"], heights=cfg.heights)
    LR.assert_same(got["exported_verdict"], LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
    ch = res["committed_height"]
    assert ch.min() >= 3
    # whole: every committed header is OK. With equivocators (twins) the references decide which heights certify; what
    # they do certify carries the run's block hashes, and the exported headers its times, whatever the equivocators do
    certified = 0
    for verdict in (got["archive_verdict"], got["exported_verdict"]):
        if whole:
            assert np.array_equal(verdict.verified_height, ch.astype(np.uint64))
        for i in range(ref["n"]):
            ok = verdict.status[i, :int(ch[i])] == LR.OK
            assert ok.all() or not whole, verdict.names(i)
            assert np.array_equal(verdict.block_hash[i, :int(ch[i])][ok], res["block_hash"][i, :int(ch[i])][ok])
            certified += int(ok.sum())
    assert certified > 0
    times = {LR.decode(h)["time"] for row in got["exported"] for h in row if h}
    assert {T.uint_size(t) for t in times} == ref["time_sizes"]


@pytest.mark.parametrize("shape", T.CRYPTO_SHAPES)
@pytest.mark.parametrize("case", T.CRYPTO_IDS)
def test_real_crypto(case, shape):
    import trace_ref as TR
    ref = T.crypto_reference(case, shape)
    T.assert_crypto_case(case, shape, ref)
    _check_crypto(ref, _crypto_run(ref), TR.joined(ref))


def test_real_crypto_n65_lossy_at_the_5_to_9_byte_change():
    """N = 65 with drops, 6 heights, once: several lane rounds per wave and 44 seals per header, with RoundChange frames
    and a header time that goes from 5 to 9 bytes"""
    import trace_ref as TR
    ref = T.crypto_reference(*T.CRYPTO_ONCE)
    T.assert_crypto_case(*T.CRYPTO_ONCE, ref)
    _check_crypto(ref, _crypto_run(ref), TR.joined(ref))


def test_twins_at_the_5_to_9_byte_change():
    """set_trace_twins on, N = 7 with 2 equivocators (cfg3's kind of run) at c-5-9: the twinned trace equals the Python
    reference's; its audit, archive and import equal the Python observer's, archiver's and importer's"""
    import twins_ref as TW
    ref = T.twins_reference()
    assert {5, 9} <= ref["time_sizes"] and sum(ref["counts"]) > 0
    _check_crypto(ref, _crypto_run(ref, twins=True), TW.joined(ref), whole=False)


def test_timestamp_rule_across_2_32():
    """constructed ledgers: a time of exactly parent + block_period is OK and one less BAD_TIME, at a parent time of
    2^32 - 1 (the sum needs more than 32 bits)"""
    import ledger_ref as LR
    import trace_ref as TR
    from bftsim.ledger import pack
    from bftsim.runtime import Simulator
    for name, ref, ledger, heights, want in T.boundary_ledgers():
        cfg = ref["cfg"]
        packed = pack(ledger, heights=heights)
        sim = Simulator(cfg)
        try:
            got = sim.verify_ledger(packed)
        finally:
            sim.close()
        hdr, lens, slot, H = packed
        LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
        for (i, x), st in want.items():
            assert got.status[i, x - 1] == st, (name, i, x, got.status.tolist())
