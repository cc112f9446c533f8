"""GPU: hostile frames by grammar. The catalogue of tests/wire_mutations.py (every case one broken or bent rule of
SPEC.md §9's decoder grammar) through the four decoders of libbftwire and through the observer with its continuations
(archiver, accuser, chronicler, roll call), against the strict reference (oracle/wire_strict.py) and the Python
references that stand on it. tests/test_wire_hostile_cpu.py checks the catalogue against the reference alone first."""
from types import SimpleNamespace

import numpy as np
import pytest

import wire_mutations as WM     # first: it puts oracle/ on the path
import accuse_ref as XR
import archive_ref as ARC
import audit_ref as AR
import rollcall_ref as RR
import timeline_ref as TL

pytestmark = pytest.mark.gpu
SENTINEL = 0xa5


@pytest.fixture(scope="module")
def codec():
    from bftsim.wire import Codec
    c = Codec(0)
    yield c
    c.close()


@pytest.fixture(scope="module")
def launches():
    """the three launch layouts as lists of case indices: the whole catalogue in its order; a fixed permutation of it
    (accepted and rejected frames share wavefronts) padded to 64 k + 1 frames, so the last block has one live lane; one
    frame alone, per kind an accepted one"""
    n = len(WM.catalogue()["cases"])
    perm = np.random.default_rng(1).permutation(n)
    pad = (1 - n) % 64
    padded = [int(i) for i in perm] + [int(i) for i in perm[:pad]]
    assert len(padded) % 64 == 1 and len(padded) > 64
    return dict(whole=list(range(n)), permuted=padded)


def _alone(kind):
    cs = WM.catalogue()["cases"]
    return [next(i for i, c in enumerate(cs) if c["kind"] == kind and c["cls"] == "accept.array_wider")]


def _stream(ix):
    return WM.stream_of([WM.catalogue()["cases"][i]["frame"] for i in ix])


def _layouts(launches, kind):
    return list(launches.items()) + [("alone", _alone(kind))]


def test_decode_equals_strict_reference(codec, launches):
    """bftwire_decode: the verdict and every field are the strict reference's; a rejected frame leaves zeros"""
    want, cs = WM.reference()["subject"], WM.catalogue()["cases"]
    for name, ix in _layouts(launches, "subject"):
        stream, off = _stream(ix)
        out, ok = codec.decode(np.frombuffer(stream, np.uint8), off)
        ok = ok.cpu().numpy()
        f = {k: v.cpu().numpy() for k, v in out.items()}
        assert len(ok) == len(ix)
        for k, i in enumerate(ix):
            w = want[i]
            assert ok[k] == (w is not None), (name, k, cs[i]["cls"], cs[i]["name"])
            got = dict(code=int(f["code"][k]), round=int(f["round"][k].view(np.uint64)), height=int(f["height"][k].view(np.uint64)),
                       create_time=int(f["create_time"][k].view(np.uint64)), ttl=int(f["ttl"][k].view(np.uint64)),
                       raw_time=int(f["raw_time"][k].view(np.uint64)), digest=bytes(f["digest"][k]),
                       signature=bytes(f["signature"][k]), commit_seal=bytes(f["commit_seal"][k]),
                       has_sig=int(f["has_sig"][k]), has_seal=int(f["has_seal"][k]))
            if w is None:
                exp = dict(code=0, round=0, height=0, create_time=0, ttl=0, raw_time=0, digest=bytes(32), signature=bytes(65),
                           commit_seal=bytes(65), has_sig=0, has_seal=0)
            else:
                exp = {k2: w[k2] for k2 in ("code", "round", "height", "create_time", "ttl", "raw_time", "digest")}
                exp.update(signature=w["signature"] or bytes(65), commit_seal=w["commit_seal"] or bytes(65),
                           has_sig=int(w["signature"] is not None), has_seal=int(w["commit_seal"] is not None))
            assert got == exp, (name, k, cs[i]["cls"], cs[i]["name"])
        assert ok.sum() == sum(want[i] is not None for i in ix) > 0


def test_decode_preprepare_equals_strict_reference(codec, launches):
    """bftwire_decode_preprepare: verdicts and every field; a rejected frame's record is all zero bytes"""
    from bftsim import wire
    want, cs = WM.reference()["preprepare"], WM.catalogue()["cases"]
    for name, ix in _layouts(launches, "preprepare"):
        stream, off = _stream(ix)
        arr, ok = codec.decode_preprepare(stream, off)
        raw = arr.view(np.uint8).reshape(len(ix), -1)
        for k, i in enumerate(ix):
            w = want[i]
            assert ok[k] == (w is not None), (name, k, cs[i]["cls"], cs[i]["name"])
            if w is None:
                assert not raw[k].any(), (name, k, cs[i]["cls"], cs[i]["name"])
            else:
                assert wire.array_to_preprepares(arr[k:k + 1])[0] == w, (name, k, cs[i]["cls"], cs[i]["name"])
        assert ok.sum() == sum(want[i] is not None for i in ix) > 0


def _decode_blocks_raw(codec, stream, off, maxpf):
    """bftwire_decode_blocks into sentinel-filled outputs, with a guard slot group on either side of `out`"""
    import torch
    from bftsim import wire
    t, dev = torch, codec.device
    n = len(off) - 1
    slot = wire.BLOCK_DTYPE.itemsize
    s = t.from_numpy(np.frombuffer(stream, np.uint8).copy()).to(dev)
    offs = t.from_numpy(np.asarray(off, np.int64)).to(dev)
    buf = t.full(((n + 2) * maxpf * slot,), SENTINEL, dtype=t.uint8, device=dev)
    cnt = t.full((n + 2,), 0x5a5a5a5a, dtype=t.int32, device=dev)
    ok = t.full((n + 2,), SENTINEL, dtype=t.uint8, device=dev)
    rc = wire.lib().bftwire_decode_blocks(codec.h, s.data_ptr(), offs.data_ptr(), n, maxpf, buf.data_ptr() + maxpf * slot,
                                          cnt.data_ptr() + 4, ok.data_ptr() + 1, None)
    assert rc == 0
    t.cuda.synchronize(dev)
    return buf.cpu().numpy().reshape(n + 2, maxpf, slot), cnt.cpu().numpy().view(np.uint32), ok.cpu().numpy()


def test_decode_blocks_equals_strict_reference(codec, launches):
    """bftwire_decode_blocks into a sentinel-filled `out`: verdicts, counts and blocks are the strict reference's;
    nothing outside a frame's own max_per_frame slots is written; an accepted frame's slots at or above its count are
    untouched; a rejected frame has count 0 and ok 0 (its slots are unspecified, include/bftwire.h)"""
    from bftsim import wire
    want, cs = WM.reference()["blocks"], WM.catalogue()["cases"]
    M = WM.MAX_PER_FRAME
    for name, ix in _layouts(launches, "blocks"):
        stream, off = _stream(ix)
        n = len(ix)
        buf, cnt, ok = _decode_blocks_raw(codec, stream, off, M)
        assert (buf[0] == SENTINEL).all() and (buf[n + 1] == SENTINEL).all()          # the guards around `out`
        assert cnt[0] == cnt[n + 1] == 0x5a5a5a5a and ok[0] == ok[n + 1] == SENTINEL
        for k, i in enumerate(ix):
            w, slots = want[i], buf[k + 1]
            assert ok[k + 1] == (w is not None) and cnt[k + 1] == (len(w) if w is not None else 0), (name, k, cs[i]["name"])
            if cs[i]["kind"] != "blocks":
                assert (slots == SENTINEL).all(), (name, k, cs[i]["cls"], cs[i]["name"])  # not a Block frame: nothing decoded
            if w is None:
                continue
            recs = slots[:len(w)].copy().view(wire.BLOCK_DTYPE).reshape(-1)
            assert [wire.rec_to_block(r) for r in recs] == w, (name, k, cs[i]["cls"], cs[i]["name"])
            assert (slots[len(w):] == SENTINEL).all(), (name, k, cs[i]["cls"], cs[i]["name"])
        assert ok[1:n + 1].sum() == sum(want[i] is not None for i in ix) > 0


def test_decode_sync_equals_strict_reference(codec, launches):
    want, cs = WM.reference()["sync"], WM.catalogue()["cases"]
    for name, ix in _layouts(launches, "sync"):
        stream, off = _stream(ix)
        h, ok = codec.decode_sync(stream, off)
        for k, i in enumerate(ix):
            assert ok[k] == (want[i] is not None) and int(h[k]) == (want[i] or 0), (name, k, cs[i]["cls"], cs[i]["name"])
        assert ok.sum() == sum(want[i] is not None for i in ix) > 0


# ---- the observer and its continuations
def _tr(c):
    return SimpleNamespace(stream=np.frombuffer(bytes(c["stream"]), np.uint8), frame_off=np.asarray(c["off"], np.uint64),
                           inst_frame0=np.asarray(c["f0"], np.uint64))


@pytest.fixture(scope="module")
def observed():
    """the stream of wire_mutations.observer_stream() through every trace entry point of one Simulator, and the Python
    references (each standing on the strict parser), computed once"""
    from bftsim.runtime import Simulator
    c = WM.observer_stream()
    cfg, H = c["cfg"], c["heights"]
    le = cfg.seed_byte_order == 1
    sim = Simulator(cfg)
    try:
        tr = _tr(c)
        got = dict(audit=sim.audit_trace(tr, max_heights=H), archive=sim.archive_trace(tr, max_heights=H),
                   accuse=sim.accuse_trace(tr, max_heights=H), timeline=sim.timeline_trace(tr, max_heights=H),
                   rollcall=sim.rollcall_trace(tr, max_heights=H))
    finally:
        sim.close()
    want = dict(archive=ARC.archive(c["stream"], c["off"], c["f0"], cfg.addresses, le, H))
    obs = want["audit"] = want["archive"]["audit"]
    want["accuse"] = XR.accuse(c["stream"], c["off"], c["f0"], cfg.addresses, le, H, audit=obs)
    want["timeline"] = TL.timeline(c["stream"], c["off"], c["f0"], cfg.addresses, le, H, audit=obs)
    want["rollcall"] = RR.rollcall(c["stream"], c["off"], c["f0"], cfg.addresses, le, c["genesis"], H, audit=obs)
    return dict(c=c, got=got, want=want)


def test_observer_statuses(observed):
    """bftsim_audit_trace over the catalogue (instance 0): statuses and signers are the strict-reference observer's;
    every case the grammar accepts is OK with the signer of its base frame, every other one UNDECODABLE with -1"""
    got, cat = observed["got"]["audit"], WM.catalogue()
    AR.assert_same(got, observed["want"]["audit"])
    n_ok = 0
    for i, c in enumerate(cat["cases"]):
        want = (AR.ST_OK, cat["signer"][c["base"]]) if c["observe"] else (AR.ST_UNDECODABLE, -1)
        assert (int(got.frame_status[i]), int(got.frame_signer[i])) == want, (i, c["cls"], c["name"])
        n_ok += bool(c["observe"])
    assert n_ok > 300 and got.report["ok"] == n_ok + 12 and got.report["undecodable"] == len(cat["cases"]) - n_ok


def test_observer_certifies_non_canonical_commits(observed):
    """five Commits, each in another valid encoding, certify their height as the canonical five do: the same
    certificate row, and byte-equal archived ledgers"""
    got, (ledger, arch) = observed["got"]["audit"], observed["got"]["archive"]
    assert (got.frame_status[-12:] == AR.ST_OK).all() and got.frame_signer[-12:].tolist() == [3, 0, 1, 2, 3, 4] * 2
    assert got.cert_round[1].tolist() == [0xffff] * 4 + [0, 0xffff] and got.report["certified"] == 2
    for k in ("cert_round", "cert_digest", "cert_voters", "cert_frame", "cert_flags"):
        assert np.array_equal(getattr(got, k)[1], getattr(got, k)[2]), k
    assert got.cert_voters[2, 4].tolist() == [0b11111, 0, 0, 0] and got.cert_frame[2, 4] == 5
    ARC.assert_same((ledger, arch), observed["want"]["archive"])
    AR.assert_same(arch.audit, observed["want"]["audit"])
    hdr, lens, slot, H = ledger
    hdr, lens = np.asarray(hdr, np.uint8).reshape(3, H, slot), np.asarray(lens, np.uint32).reshape(3, H)
    assert lens[1, 4] > 0 and np.array_equal(lens[1], lens[2]) and np.array_equal(hdr[1], hdr[2])
    assert not lens[0].any() and arch.report["headers"] == 2


def test_continuations_equal_their_references(observed):
    """the accuser, the chronicler and the roll call over the same stream equal their Python references, and each
    passes the observer's outputs through unchanged"""
    got, want = observed["got"], observed["want"]
    XR.assert_same(got["accuse"], want["accuse"])
    TL.assert_same(got["timeline"], want["timeline"])
    RR.assert_same(got["rollcall"], want["rollcall"])
    for k in ("accuse", "timeline", "rollcall"):
        AR.assert_same(got[k].audit, want["audit"])
    TL.assert_same(got["rollcall"].timeline, want["timeline"])
    assert want["timeline"]["report"]["prepare_frames"] > 50 and want["rollcall"]["report"]["frames"] == got["audit"].report["ok"]
