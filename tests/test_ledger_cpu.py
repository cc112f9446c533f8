"""CPU: the importer's decode, scatter, tally and link steps (consensus-rs_amd/csrc/bft_ledger.h, host build
tests/emu/ledger_host.cpp, recoveries from the C oracle) against the independent Python verifier (tests/ledger_ref.py),
array for array, over ledgers built from oracle runs and tampered variants of them; the decoder as a stand-alone program
under ASan + UBSan; the C ABI's bindings and argument checks."""
import ctypes
import os
import shutil
import subprocess

import msgpack
import numpy as np
import pytest

import ledger_ref as LR         # first: it puts oracle/ on the path
import ledger_lib as LL
import oracle_lib as O
from bftsim.ledger import pack

(OK, ABSENT, UNDECODABLE, BAD_HEIGHT, NO_PARENT, BAD_PARENT, BAD_TIME, LACK_VOTES, BAD_VOTE, BAD_PROPOSER) = range(10)


def _both(ref, ledger, heights=None, slot_bytes=None):
    """(host build, Python reference) over one ledger, asserted equal"""
    cfg = ref["cfg"]
    hdr, lens, slot, H = pack(ledger, slot_bytes=slot_bytes, heights=cfg.heights if heights is None else heights)
    got = LL.verify(hdr, lens, slot, H, cfg, ref["genesis"])
    LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg, ref["genesis"]))
    return got


def _voters(got, i, x):
    w = got["voters"][i, x - 1]
    return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]


@pytest.fixture(scope="module")
def cfg1():
    return LR.reference("cfg1")


@pytest.fixture(scope="module")
def n4():
    return LR.reference("n4")


def test_cfg1_verifies(cfg1):
    got = _both(cfg1, cfg1["ledger"])
    assert (got["status"] == OK).all() and got["verified_height"][0] == 6 == int(cfg1["res"]["committed_height"][0])
    assert np.array_equal(got["block_hash"][0], cfg1["res"]["block_hash"][0])
    assert all(_voters(got, 0, x) == [0, 1, 2, 3] for x in range(1, 7)) and (got["n_votes"] == 4).all()
    assert got["report"] == dict(headers=6, by_status=[6] + [0] * 9, votes=24, recoveries=24, duplicate_votes=0,
                                 verified_instances=1)


def test_n4_quorum_boundary(n4):
    """Q = 2: three distinct seals verify, two are LACK_VOTES"""
    got = _both(n4, n4["ledger"])
    assert (got["status"] == OK).all() and (got["verified_height"] == 6).all() and got["report"]["verified_instances"] == 2
    led = [list(r) for r in n4["ledger"]]
    led[1][3] = LR.reseal(led[1][3], n4["secrets"], [1, 3])
    got = _both(n4, led)
    assert got["status"][1, 3] == LACK_VOTES and _voters(got, 1, 4) == [1, 3]
    assert (np.delete(got["status"].reshape(-1), 9) == OK).all()          # the block hash ignores votes: height 5 links on
    assert list(got["verified_height"]) == [6, 3] and got["report"]["verified_instances"] == 1


@pytest.mark.parametrize("case,ok", [("n100_67", True), ("n100_68", True), ("n256_171", True), ("n256_170", False)])
def test_wide_sets(case, ok):
    """N = 100 (Q = 66) with 67 and 68 seals, N = 256 (Q = 170) with 171 and 170: the 0xdc array form, every voter word"""
    ref = LR.reference(case)
    got = _both(ref, ref["ledger"])
    assert (got["status"] == (OK if ok else LACK_VOTES)).all()
    assert _voters(got, 0, 1) == ref["voters"] and got["n_votes"][0, 0] == len(ref["voters"])
    assert got["verified_height"][0] == (2 if ok else 0)


def _status_cases(cfg1):
    """one header for each status 1..9, each in a ledger of its own: [(ledger, instance, height, status)]"""
    L, sec = cfg1["ledger"][0], cfg1["secrets"]
    rs = lambda h, **f: LR.reseal(LR.replace_field(h, **f), sec, [0, 1, 2, 3])
    out = [([L[:3]], 0, 4, ABSENT),
           ([L[:2] + [L[2][:-5]] + L[3:]], 0, 3, UNDECODABLE),
           ([L[:2] + [rs(L[2], height=7)] + L[3:]], 0, 3, BAD_HEIGHT),
           ([L[:2] + [b""] + L[3:]], 0, 4, NO_PARENT),
           ([L[:2] + [rs(L[2], prev_hash=bytes(32))] + L[3:]], 0, 3, BAD_PARENT),
           ([L[:2] + [rs(L[2], time=LR.decode(L[1])["time"] + cfg1["cfg"].block_period - 1)] + L[3:]], 0, 3, BAD_TIME),
           ([L[:2] + [LR.encode(LR.decode(L[2]), "nil")] + L[3:]], 0, 3, LACK_VOTES),
           ([L[:2] + [LR.reseal(L[2], [O.keccak256(b"stranger")] * 5, [0, 1, 2, 4])] + L[3:]], 0, 3, BAD_VOTE),
           ([L[:2] + [rs(L[2], proposer=bytes(range(20)))] + L[3:]], 0, 3, BAD_PROPOSER)]
    return out


def test_one_header_of_each_status(cfg1):
    for ledger, i, x, want in _status_cases(cfg1):
        got = _both(cfg1, ledger)
        assert got["status"][i, x - 1] == want, (want, got["status"].tolist())
        assert got["report"]["by_status"][want] >= 1
    # a time of exactly parent.time + block_period passes; 11- and 12-field headers are LACK_VOTES
    L, sec = cfg1["ledger"][0], cfg1["secrets"]
    t = LR.decode(L[1])["time"] + cfg1["cfg"].block_period
    got = _both(cfg1, [L[:2] + [LR.reseal(LR.replace_field(L[2], time=t), sec, [0, 1, 2, 3])]])
    assert got["status"][0, 2] == OK
    nil = cfg1["nil"][0][0]
    twelve = bytes([0x9c]) + nil[1:-1]
    eleven = bytes([0x9b]) + nil[1:-1 - len(msgpack.packb(list(b"Coinse base")))]
    got = _both(cfg1, [[twelve], [eleven]])
    assert list(got["status"][:, 0]) == [LACK_VOTES, LACK_VOTES] and (got["block_hash"][0, 0] != got["block_hash"][1, 0]).any()
    assert np.array_equal(got["block_hash"][0, 0], cfg1["res"]["block_hash"][0, 0])


def test_distinct_voters_count(n4):
    """exactly Q distinct voters is LACK_VOTES, Q + 1 is OK; Q + 1 votes of which two are one validator's is LACK_VOTES
    with duplicate_votes = 1 (the reference's votes.len() would accept it)"""
    sec, h = n4["secrets"], n4["ledger"][0][0]
    for voters, want, dup in (([0, 1], LACK_VOTES, 0), ([0, 1, 3], OK, 0), ([0, 1, 1], LACK_VOTES, 1), ([2, 2, 2, 2], LACK_VOTES, 3)):
        got = _both(n4, [[LR.reseal(h, sec, voters)]])
        assert got["status"][0, 0] == want and got["report"]["duplicate_votes"] == dup, voters
        assert _voters(got, 0, 1) == sorted(set(voters)) and got["n_votes"][0, 0] == len(voters)


def test_bad_votes(n4):
    sec, h = n4["secrets"], n4["ledger"][0][0]
    d = LR.decode(h)
    flipped = bytearray(d["votes"][1])
    flipped[40] ^= 0x01
    got = _both(n4, [[LR.with_votes(LR.encode(d, "nil"), [d["votes"][0], bytes(flipped), d["votes"][2]])]])
    assert got["status"][0, 0] == BAD_VOTE                                  # a flipped seal byte
    outsider = LR.seal(O.keccak256(b"not a validator"), LR.block_hash(d))
    got = _both(n4, [[LR.with_votes(LR.encode(d, "nil"), list(d["votes"]) + [outsider])]])
    assert got["status"][0, 0] == BAD_VOTE and _voters(got, 0, 1) == [0, 1, 2]   # a seal by a key outside the set
    got = _both(n4, [[LR.with_votes(LR.encode(d, "nil"), [outsider])]])
    assert got["status"][0, 0] == BAD_VOTE                                  # BAD_VOTE together with too few votes
    got = _both(n4, [[LR.with_votes(LR.encode(d, "nil"), [bytes(65)] * 3)]])
    assert got["status"][0, 0] == BAD_VOTE and got["report"]["recoveries"] == 3   # seals that do not recover


def test_tampered_tx_hash_breaks_the_chain(cfg1):
    L = list(cfg1["ledger"][0])
    L[2] = LR.replace_field(L[2], tx_hash=O.keccak256(b"another body"))
    got = _both(cfg1, [L])
    assert list(got["status"][0]) == [OK, OK, BAD_VOTE, BAD_PARENT, OK, OK] and got["verified_height"][0] == 2
    assert got["report"]["verified_instances"] == 0
    assert not np.array_equal(got["block_hash"][0, 2], cfg1["res"]["block_hash"][0, 2])


def test_swapped_slots(cfg1):
    L = list(cfg1["ledger"][0])
    L[1], L[2] = L[2], L[1]
    got = _both(cfg1, [L])
    assert list(got["status"][0]) == [OK, BAD_HEIGHT, BAD_HEIGHT, BAD_PARENT, OK, OK] and got["verified_height"][0] == 1


def test_non_canonical_encodings_hash_as_the_canonical_header(cfg1):
    """integers in wider forms than they need, the array headers too, an upper-case address: the same block hash"""
    h = cfg1["ledger"][0][1]
    d = LR.decode(h)
    wide = lambda v: b"\xcf" + v.to_bytes(8, "big")
    lst = lambda b: b"\xdd" + len(b).to_bytes(4, "big") + b"".join(b"\xcd\x00" + bytes([c]) for c in b)
    raw = b"\xdc\x00\x0d" + lst(d["prev_hash"]) + b"\xda\x00\x2a0X" + d["proposer"].hex().upper().encode() + \
        lst(d["root"]) + lst(d["tx_hash"]) + lst(d["receipt_hash"]) + \
        b"".join(wide(d[k]) for k in ("bloom", "difficulty", "height", "gas_limit", "gas_used", "time")) + \
        lst(d["extra"]) + b"\xdd" + len(d["votes"]).to_bytes(4, "big") + b"".join(b"\xdd\x00\x00\x00\x41" + b"".join(
            b"\xcc" + bytes([c]) for c in v) for v in d["votes"])
    assert raw != h and LR.decode(raw) == d
    L = list(cfg1["ledger"][0])
    L[1] = raw
    got = _both(cfg1, [L])
    assert (got["status"] == OK).all() and np.array_equal(got["block_hash"][0], cfg1["res"]["block_hash"][0])


def test_undecodable_shapes(cfg1):
    h = cfg1["ledger"][0][0]
    d = LR.decode(h)
    nil = LR.encode(d, "nil")
    cases = [h + b"\x00",                                                               # trailing bytes
             LR.with_votes(nil, [d["votes"][0][:64]]),                                  # a vote of 64 bytes
             nil[:-1] + msgpack.packb([list(d["votes"][0])] * 257),                     # more than 256 votes
             LR.encode(dict(d, extra=bytes(33)), "own"),                                # extra above 32 bytes
             bytes([0x9e]) + h[1:] + b"\xc0", bytes([0x9a]) + h[1:],                     # 14 and 10 fields
             h[:4] + b"\xd0\x05" + h[(5 if h[4] < 0x80 else 6):]]                       # a signed integer
    got = _both(cfg1, [[c] for c in cases] + [[LR.with_votes(nil, [d["votes"][0]] * 256)]], heights=1)
    assert (got["status"][:-1, 0] == UNDECODABLE).all() and not got["block_hash"][:-1].any()
    assert got["status"][-1, 0] == LACK_VOTES and got["report"]["duplicate_votes"] == 255
    # a length above the slot is undecodable unread
    hdr, lens, slot, H = pack([[h]], heights=1)
    lens[0] = slot + 1
    got = LL.verify(hdr, lens, slot, H, cfg1["cfg"], cfg1["genesis"])
    LR.assert_same(got, LR.verify(hdr, lens, slot, H, cfg1["cfg"], cfg1["genesis"]))
    assert got["status"][0, 0] == UNDECODABLE


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_decoder_program_under_asan_ubsan(n4):
    """the stand-alone program (its own main, run directly): every truncation and every single-byte flip of one N = 4
    header, decoded (and its votes scattered) from heap buffers of exactly the header's length"""
    exe = LL.build_san()
    h = n4["ledger"][0][0]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=LL.san_input([h]), capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.decode().strip() == f"ok 1 headers {4 * len(h) - 1} cases"
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound_and_check_arguments():
    """bound, and argument errors are BFTSIM_EINVAL before any device work, with nothing written (this runs without a
    GPU: the handle of a create that could not reach a device still checks arguments)"""
    from bftsim import _abi, runtime, ledger
    from bftsim.configs import cfg1 as mk
    L = runtime.lib()
    rep = _abi.CLedgerReport()
    buf, lens = np.zeros(64, np.uint8), np.zeros(2, np.uint32)
    assert L.bftsim_verify_ledger(None, buf.ctypes.data, 32, lens.ctypes.data, 1, 2, None, ctypes.byref(rep)) == -1
    assert L.bftsim_set_ledger_votes(None, 0) == -1 and L.bftsim_ledger_last_ms(None, None, None, None, None) == -1
    for k in ("set_ledger_votes", "verify_ledger", "ledger_ms"):
        assert hasattr(runtime.Simulator, k)
    assert callable(ledger.compare) and hasattr(ledger.Verdict, "voter_list")
    c, keep = _abi.to_cconfig(mk(True, heights=6))
    h = ctypes.c_void_p()
    L.bftsim_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert h.value
    o, arrs = _abi.alloc_ledger(1, 2)
    for a in arrs.values():
        a[...] = 7
    rep.headers = 77

    def call(hdr=buf.ctypes.data, slot=32, ln=lens.ctypes.data, inst=1, heights=2, rep=rep):
        return L.bftsim_verify_ledger(h, hdr, slot, ln, inst, heights, ctypes.byref(o), ctypes.byref(rep) if rep is not None else None)

    assert call(rep=None) == -1 and call(hdr=None) == -1 and call(ln=None) == -1
    assert call(heights=0) == -1 and call(heights=65536) == -1 and call(slot=0) == -1 and call(inst=1 << 31) == -1
    assert len(L.bftsim_last_error(h)) > 0 and rep.headers == 77 and all((a == 7).all() for a in arrs.values())
    assert L.bftsim_set_ledger_votes(h, 2) == -1 and L.bftsim_set_ledger_votes(h, 1) == 0 and L.bftsim_set_ledger_votes(h, 0) == 0
    ms = [ctypes.c_float(-1) for _ in range(4)]
    assert L.bftsim_ledger_last_ms(h, *[ctypes.byref(x) for x in ms]) == 0 and all(x.value == 0 for x in ms)
    del keep


def test_new_structs_bound_in_integration_md():
    """bftsim_ledger_report / bftsim_ledger_out: INTEGRATION.md's #[repr(C)] structs against the header, by the checker of
    test_integration_binding (field names, types, offsets and sizes as gcc lays them out); the ctypes mirrors too"""
    import re
    import test_integration_binding as B
    from bftsim import _abi
    txt = re.sub(r"struct (bftsim_ledger_\w+) \{(.*?)\};\s*typedef struct \1 \1;", r"typedef struct \1 {\2} \1;",
                 B.header_text(), flags=re.S)
    decls = {k: v for k, v in B.c_struct_decls(txt).items() if k.startswith("bftsim_ledger_")}
    assert set(decls) == {"bftsim_ledger_report", "bftsim_ledger_out"}
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
    for name, cls in (("bftsim_ledger_report", _abi.CLedgerReport), ("bftsim_ledger_out", _abi.CLedgerOut)):
        assert ctypes.sizeof(cls) == lay[(name, "sizeof")]
        assert [f for f, _ in cls._fields_] == [f for f, _ in decls[name]]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[(name, f)], (name, f)
    for k in ("BFTSIM_VOTES_SIGNATURES", "BFTSIM_VOTES_SEALS", "BFTSIM_LEDGER_OK", "BFTSIM_LEDGER_BAD_PROPOSER"):
        assert k in consts


def test_shared_tamper_set():
    """the tampered ledgers the GPU test sends through bftsim_verify_ledger, here through the host build"""
    for name, ref, ledger, heights, want in LR.tamper_cases():
        got = _both(ref, ledger, heights=heights)
        for (i, x), st in want.items():
            assert got["status"][i, x - 1] == st, (name, i, x, got["status"].tolist())


def test_committed_times_increase_strictly():
    """the timestamp rule on the runs themselves (the C oracle): committed time_ticks increase strictly, so a real
    run's header is never BAD_TIME (time = genesis_time + block_period * (tick + 1), SPEC.md §4)"""
    from bftsim.configs import BftConfig, cfg1 as mk1, cfg4
    shapes = [(mk1(True, heights=6), 0, 1), (BftConfig(n=4, heights=15, seed=21, drop_ppm=100_000), 3, 3),
              (BftConfig(n=65, heights=6, seed=9, drop_ppm=50_000), 0, 2), (BftConfig(n=100, heights=4, seed=5), 0, 1),
              (cfg4(7, heights=10), 3, 8), (cfg4(64, heights=6), 0, 4), (BftConfig(n=256, heights=2, seed=5), 0, 1)]
    for cfg, first, n in shapes:
        res = O.run(cfg, first, n)
        assert res["committed_height"].sum() > 0
        for i in range(n):
            t = res["time_tick"][i, :int(res["committed_height"][i])].astype(np.int64)
            assert (np.diff(t) > 0).all() and (len(t) == 0 or t[0] >= 0), (cfg.n, i, t.tolist())
