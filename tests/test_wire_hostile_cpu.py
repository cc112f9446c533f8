"""Hostile frames by grammar, on the CPU: the catalogue of tests/wire_mutations.py (every case one broken or bent rule of
SPEC.md §9's decoder grammar) through the host builds of every decoder, against the strict reference
(oracle/wire_strict.py). The catalogue is first checked against the reference alone; the reference is checked against
the msgpack-based decoders it replaces on every well-formed frame of the existing generators."""
import ctypes
import os
import random
import shutil
import subprocess

import numpy as np
import pytest

import wire_mutations as WM     # first: it puts oracle/ on the path
import audit_lib as AL
import audit_ref as AR
import ledger_lib as LL
import ledger_ref as LR
import trace_ref as TR
import twins_ref as TW
import wire_lib as W
import wire_ref as R
import wire_strict as WS
from test_gpu_wire import make_batch, oracle_msg
from test_wire_block_cpu import EDGE, host_blocks_decode, host_pp_decode, rand_block, rand_pp

H = 6
SAN_ENV = dict(ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")


@pytest.fixture(scope="module")
def cat():
    return WM.catalogue()


@pytest.fixture(scope="module")
def ref():
    return WM.reference()


def test_catalogue_checks_itself():
    """before anything is compared: every class is non-empty and the strict reference alone gives every case the verdict
    its class declares, at its own entry point, at the three others (rejected) and at the observer"""
    counts = WM.self_check()
    assert set(counts) == set(WM.CLASSES) and sum(counts.values()) == len(WM.catalogue()["cases"]) > 5000
    hc = WM.header_catalogue()["cases"]
    assert len(hc) > 500
    for c in hc:
        assert (LR.decode(c["frame"]) is not None) == c["accept"], (c["cls"], c["name"])


def test_catalogue_is_deterministic(cat):
    WM.catalogue.cache_clear()
    again = WM.catalogue()
    assert [c["frame"] for c in again["cases"]] == [c["frame"] for c in cat["cases"]]
    assert [(c["cls"], c["name"]) for c in again["cases"]] == [(c["cls"], c["name"]) for c in cat["cases"]]


def test_strict_equals_loose_on_well_formed_frames():
    """the strict decoders equal the msgpack-based ones they replace on every well-formed frame of the existing
    generators: make_batch, rand_pp, rand_block, the Sync edges and the pinned traces"""
    b = make_batch(300, 5)
    for i in range(300):
        m = oracle_msg(b, i)
        for peer in (None, bytes(range(34))):
            f = R.encode(dict(m, peer_id=peer))[0]
            want = R.loose_decode(f)
            assert want is not None and WS.decode(f) == want, i
            assert WS.decode_preprepare(f) is None and WS.decode_blocks(f) is None and WS.decode_sync(f) is None
    rng = random.Random(3)
    for _ in range(60):
        f = R.preprepare_frame(rand_pp(rng))[0]
        want = R.loose_decode_preprepare(f)
        assert want is not None and WS.decode_preprepare(f) == want and WS.decode(f) is None
    rng = random.Random(4)
    for k in range(30):
        blocks = [rand_block(rng) for _ in range(rng.randrange(4))]
        f = R.blocks_frame(blocks, 10, 1000 + k)
        assert WS.decode_blocks(f) == R.loose_decode_blocks(f) == blocks and WS.decode_blocks(f, len(blocks)) == blocks
        assert (WS.decode_blocks(f, len(blocks) - 1) is None) and WS.decode_sync(f) is None
    for h in EDGE:
        f = R.sync_frame(h, 10, 7)
        assert WS.decode_sync(f) == R.loose_decode_sync(f) == h and WS.decode_blocks(f) is None
    frames = 0
    for stream, off, _, _ in (TR.joined(TR.reference("cfg1")), TR.joined(TR.reference("n4")), TW.joined(TW.reference("n7"))):
        for k in range(len(off) - 1):
            fr = bytes(stream[int(off[k]):int(off[k + 1])])
            want = AR.parse_loose(fr)
            assert want is not None and AR.parse(fr) == want, k
            frames += 1
    assert frames > 500
    for row in LR.reference("n4")["ledger"] + LR.reference("cfg1")["ledger"]:
        for h in row:
            d = LR.decode(h)
            assert d is not None and LR.encode(d, "own") == h


def _host(kind, f):
    if kind == "subject":
        return W.decode(f)
    if kind == "preprepare":
        return host_pp_decode(f)
    if kind == "blocks":
        return host_blocks_decode(f, WM.MAX_PER_FRAME)
    v = ctypes.c_uint64()
    return v.value if W.lib().wire_host_sync_decode(f, len(f), ctypes.byref(v)) == 1 else None


@pytest.mark.parametrize("kind", WM.KINDS)
def test_host_decoder_equals_strict_reference(cat, ref, kind):
    """wire_host_decode / _pp_decode / _blocks_decode / _sync_decode over the whole catalogue: the verdict and every
    field are the strict reference's"""
    accepted = 0
    for i, c in enumerate(cat["cases"]):
        got, want = _host(kind, c["frame"]), ref[kind][i]
        assert got == want, (i, c["cls"], c["name"], kind)
        accepted += want is not None
    assert accepted == sum(1 for c in cat["cases"] if c["kind"] == kind and c["accept"]) > 0


def test_observer_decode_pass_equals_strict_reference(cat, ref):
    """audit_host's decode pass: decodable exactly where the strict observer parses; an accepted case's record (code,
    height, round, digest, sign digest, signature, pp_want) is its canonical base frame's, a rejected one's is zero"""
    cases = cat["cases"]
    rec = AL.records([c["frame"] for c in cases], cat["cfg"], H)
    seals = 0
    for i, c in enumerate(cases):
        want = ref["observe"][i]
        assert (rec["st"][i] == AR.ST_OK) == (want is not None) == bool(c["observe"]), (i, c["cls"], c["name"])
        b = c["base"]
        for k in ("code", "hx", "round", "digest", "sdig", "sig", "pp_want"):
            if want is not None:
                assert np.array_equal(rec[k][i], rec[k][b]), (i, c["cls"], c["name"], k)
            else:
                assert np.array_equal(rec[k][i], np.full_like(rec[k][i], 0xffffffff if k == "pp_want" else 0)), (i, c["name"], k)
        if want is not None:
            assert rec["code"][i] == want["code"] and int(rec["round"][i]) == want["round"] and rec["hx"][i] == want["height"]
            assert bytes(rec["sig"][i]) == want["sig"]
            if want["code"] != 1:
                assert bytes(rec["digest"][i]) == want["digest"]
        if want is not None and want["code"] == 3:
            assert rec["seal_k"][i] == seals and bytes(rec["seal"][seals]) == want["seal"]
            seals += 1
        else:
            assert rec["seal_k"][i] == 0xffffffff
    assert rec["n_seals"] == seals > 0


def test_observer_statuses_of_the_signed_cases(cat, ref):
    """the host observer end to end over the Subject and Preprepare cases: every accepted case is OK with the signer of
    its base frame, every other one UNDECODABLE with signer -1, as the Python observer says"""
    ix = [i for i, c in enumerate(cat["cases"]) if c["kind"] in ("subject", "preprepare")]
    frames = [cat["cases"][i]["frame"] for i in ix]
    stream, off = WM.stream_of(frames)
    f0 = np.array([0, len(frames)], np.uint64)
    cfg = cat["cfg"]
    got = AL.observe(stream, off.astype(np.uint64), f0, cfg, H)
    AR.assert_same(got, AR.observe(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, H))
    for k, i in enumerate(ix):
        c = cat["cases"][i]
        want = (AR.ST_OK, cat["signer"][c["base"]]) if c["observe"] else (AR.ST_UNDECODABLE, -1)
        assert (int(got["frame_status"][k]), int(got["frame_signer"][k])) == want, (i, c["cls"], c["name"])


def test_observer_stream_through_the_host_continuations():
    """the stream the GPU tests audit (the catalogue, then a quorum of Commits in canonical and in five non-canonical
    encodings) through the host builds of the observer, archiver, accuser, chronicler and roll call: each equals its
    Python reference, which stands on the strict parser; the two quorums certify alike and archive to the same bytes"""
    import accuse_lib as XL
    import accuse_ref as XR
    import archive_lib as ARL
    import archive_ref as ARC
    import rollcall_lib as RL
    import rollcall_ref as RR
    import timeline_lib as TLL
    import timeline_ref as TL
    c = WM.observer_stream()
    cfg, le, args = c["cfg"], c["cfg"].seed_byte_order == 1, (c["stream"], c["off"], c["f0"])
    want = ARC.archive(*args, cfg.addresses, le, H)
    obs = want["audit"]
    got = ARL.archive(*args, cfg, H, 0)
    AR.assert_same(got["audit"], obs)
    ARC.assert_same(got, want)
    assert obs["report"]["certified"] == 2 and want["headers"][1] == want["headers"][2] and want["headers"][1][4]
    for k in ("cert_round", "cert_digest", "cert_voters", "cert_frame", "cert_flags"):
        assert np.array_equal(obs[k][1], obs[k][2]), k
    g = XL.accuse(*args, cfg, H)
    XR.assert_same({k: g[k] for k in XR.ARRAYS + ("report",)}, XR.accuse(*args, cfg.addresses, le, H, audit=obs))
    g = TLL.timeline(*args, cfg, H)
    TL.assert_same({k: g[k] for k in TL.ARRAYS + ("report",)}, TL.timeline(*args, cfg.addresses, le, H, audit=obs))
    RR.assert_same(RL.rollcall(*args, cfg, c["genesis"], H), RR.rollcall(*args, cfg.addresses, le, c["genesis"], H, audit=obs))


def test_importer_on_the_header_classes():
    """ledger_host over the classes that apply to a bare header, one instance of one height each: UNDECODABLE exactly
    where the grammar rejects, and every array and counter the Python importer's"""
    from bftsim.ledger import pack
    hc = WM.header_catalogue()
    ref, cases = hc["ref"], hc["cases"]
    hdr, lens, slot, Hh = pack([[c["frame"]] for c in cases], heights=1)
    got = LL.verify(hdr, lens, slot, Hh, ref["cfg"], ref["genesis"])
    LR.assert_same({k: got[k] for k in LR.ARRAYS + ("report",)}, LR.verify(hdr, lens, slot, Hh, ref["cfg"], ref["genesis"]))
    for i, c in enumerate(cases):
        assert (got["status"][i, 0] != LR.UNDECODABLE) == c["accept"], (i, c["cls"], c["name"])
        if c["cls"] in ("base", "accept.int_wider", "accept.array_wider", "accept.address"):
            assert got["status"][i, 0] == LR.OK, (i, c["cls"], c["name"])       # the same fields: the seals stand


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_wire_program_under_asan_ubsan(cat, ref):
    """the stand-alone program (its own main, run directly): the four decoders over the whole catalogue, each frame in a
    heap buffer of exactly its length, the verdicts compared with the strict reference's"""
    exe = W.build_san()
    cases = [(c["frame"], [ref[k][i] is not None for k in WM.KINDS]) for i, c in enumerate(cat["cases"])]
    r = subprocess.run([exe], input=W.san_input(WM.MAX_PER_FRAME, cases), capture_output=True,
                       env=dict(os.environ, **SAN_ENV), timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.decode().strip() == f"ok {len(cases)} cases"
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_observer_program_under_asan_ubsan(cat, ref):
    """audit_host's stand-alone program over the whole catalogue, after its own truncations and flips of one base frame"""
    exe = AL.build_san()
    cfg = cat["cfg"]
    base = cat["cases"][cat["bases"][0]]["frame"]
    cases = [(c["frame"], ref["observe"][i] is not None) for i, c in enumerate(cat["cases"])]
    r = subprocess.run([exe], input=AL.san_input(cfg.address_bytes(), cfg.n, [base], cases), capture_output=True,
                       env=dict(os.environ, **SAN_ENV), timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    assert r.stdout.decode().split("\n")[:2] == [f"ok 1 frames {4 * len(base)} cases", f"catalogue ok {len(cases)} cases"]
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]
