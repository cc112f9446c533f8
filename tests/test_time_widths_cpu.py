"""CPU: the host builds of the device's header and frame code at every MessagePack width of `time` and `create_time`
(tests/time_cases.py), against the oracle and the independent Python references:
- the importer's canonical re-encoding (bft_ledger.h, tests/emu/ledger_host.cpp) over the grid of heights and times of
  tests/test_oracle_kat.py, against the oracle's encoder (pinned there to the msgpack package);
- every case of tests/test_gpu_time_widths.py on the oracle alone: it has the sizes of `time` it is there for;
- real-crypto runs at four genesis times: the frame emitter (bft_trace.h) against tests/trace_ref.py byte for byte, the
  observer, the archiver and the importer (bft_audit.h, bft_archive.h, bft_ledger.h) against their Python references;
- the importer's timestamp rule across the 32-bit boundary."""
import ctypes

import numpy as np
import pytest

import ledger_ref as LR         # first: it puts oracle/ on the path
import archive_lib as ARL
import archive_ref as ARC
import audit_lib as AL
import audit_ref as AR
import ledger_lib as LL
import oracle_lib as O
import time_cases as T
import trace_lib as TL
import trace_ref as TR
from bftsim.configs import string_to_address
from bftsim.ledger import pack
from time_cases import GRID_HASHES, GRID_HEIGHTS, GRID_TIMES


def test_importer_reencodes_every_width_as_the_oracle():
    """a header of every (height, time) of the grid, with all-high and all-low parent and tx hashes, decoded and hashed
    by the host build of the importer: the block hash is Keccak of the oracle's encoding, and the verdict (BAD_HEIGHT:
    no height of the grid is 1) is the Python importer's"""
    ref = LR.reference("cfg1")
    cfg = ref["cfg"]
    prop = string_to_address("0x72d5c75fd6703414aa87f79b3e4797dd09cd9251")
    extra = b"Coinse base"
    L = O.lib()
    headers = []
    for height in GRID_HEIGHTS:
        for time in GRID_TIMES:
            for prev, tx in zip(GRID_HASHES, GRID_HASHES):
                buf = (ctypes.c_uint8 * 512)()
                n = L.orc_encode_header(buf, prev, prop, tx, height, 0, 0, time, extra, len(extra))
                headers.append(bytes(buf[:n]))
    assert len({len(h) for h in headers}) == 2 * 11               # 11 sums of a height's and a time's width, 2 hash lengths
    hdr, lens, slot, H = pack([[h] for h in headers], heights=1)
    got = LL.verify(hdr, lens, slot, H, cfg, ref["genesis"])
    LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, ref["genesis"]))
    for i, h in enumerate(headers):
        assert bytes(got["block_hash"][i, 0]) == O.keccak256(h), i
        assert LR.decode(h)["time"] in GRID_TIMES
    assert (got["status"] == LR.BAD_HEIGHT).all()                 # no height of the grid is the slot's


def test_gpu_cases_show_their_sizes_on_the_oracle():
    """every case of tests/test_gpu_time_widths.py on the oracle alone (time_cases.reference asserts assert_case)"""
    for case in T.SHORT_IDS:
        for shape in list(T.PLAIN) + list(T.NO_FAST):
            T.reference("PLAIN" if shape in T.PLAIN else "NO_FAST", shape, case)
    for shape in T.LONG:
        T.reference("LONG", shape, "t-0")
    for case in T.LEDGER_IDS:
        for shape in T.LEDGER:
            T.reference("LEDGER", shape, case)
    for mode in T.CHAIN_MODE_IDS:
        for case in T.CHAIN_IDS:
            T.reference("CHAIN", mode, case)
    for case in T.CHAIN_REST:
        T.reference("CHAIN", T.TIGHTEST + "-260" if case == "t-0" else T.TIGHTEST, case)
    mk, first, n, _ = T.STREAM
    for case in T.STREAM_IDS:
        cfg = T.with_time(mk(), case)
        T.assert_case(case, cfg, O.run(cfg, first, n, threads=8))


@pytest.mark.parametrize("case,shape", [(c, s) for c in T.CRYPTO_IDS for s in T.CRYPTO_SHAPES] + [T.CRYPTO_ONCE])
def test_real_crypto_host_builds_equal_references(case, shape):
    ref = T.crypto_reference(case, shape)
    T.assert_crypto_case(case, shape, ref)
    cfg, res, want = ref["cfg"], ref["res"], ref["want"]
    # the frame emitter, frame for frame, and create_time as the device computes it
    for stream, off, meta, ms in ref["inst"]:
        for k, m in enumerate(ms):
            frame = stream[int(off[k]):int(off[k + 1])]
            got, n, counted = TL.frame(m)
            assert counted == n == len(frame) and got == frame, (k, m["code"])
            assert TL.lib().trace_host_create_time(m["code"], cfg.genesis_time, cfg.block_period, m["meta"][0]) == m["ctime"]
    # the observer and the archiver over the stream, the importer over the archive
    stream, off, _, f0 = TR.joined(ref)
    AR.assert_same(AL.observe(stream, off, f0, cfg, cfg.heights), want["archive"]["audit"])
    got = ARL.archive(stream, off, f0, cfg, cfg.heights)
    assert got["errors"] == 0
    ARC.assert_same(got, want["archive"])
    verdict = LL.verify(got["hdr"], got["hdr_len"], got["slot_bytes"], cfg.heights, cfg, TR.genesis_hash(cfg))
    LR.assert_same(verdict, want["ledger"])
    ch = int(res["committed_height"][0])
    assert ch >= 3 and want["certified"][0, :ch].all()
    assert (verdict["status"][0, :ch] == LR.OK).all() and int(verdict["verified_height"][0]) == ch
    assert np.array_equal(verdict["block_hash"][0, :ch], res["block_hash"][0, :ch])
    # the sealed ledger of the same run (headers by the oracle's encoder, seals of Q + 1 validators)
    ledger, res2, _ = LR.build(cfg, ref["secrets"], ref["first"], 1, lambda i, x: list(range((2 * cfg.n) // 3 + 1)))
    hdr, lens, slot, H = pack(ledger, heights=cfg.heights)
    sealed = LL.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg))
    LR.assert_same(sealed, LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg)))
    assert (sealed["status"][0, :ch] == LR.OK).all() and np.array_equal(res2["block_hash"], res["block_hash"])


def test_timestamp_rule_across_2_32():
    for name, ref, ledger, heights, want in T.boundary_ledgers():
        cfg = ref["cfg"]
        hdr, lens, slot, H = pack(ledger, heights=heights)
        got = LL.verify(hdr, lens, slot, H, cfg, ref["genesis"])
        LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, ref["genesis"]))
        for (i, x), st in want.items():
            assert got["status"][i, x - 1] == st, (name, i, x, got["status"].tolist())
