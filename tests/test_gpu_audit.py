"""GPU: the observer (include/bftsim.h bftsim_audit_trace / bftsim_audit_last_trace, SPEC.md §11c): a frame stream
audited from its bytes on the device. Small shapes equal the independent Python observer (tests/audit_ref.py) array
for array, hostile variants included; larger ones are tied to the run that produced them (bftsim.trace.compare)."""
from types import SimpleNamespace

import numpy as np
import pytest

import trace_ref as TR          # first: it puts oracle/ on the path
import audit_ref as AR
import oracle_lib as O
import secp256k1_ref as S
import wire_ref as R
from bftsim.configs import BftConfig, cfg3, cfg4

pytestmark = pytest.mark.gpu
OK, UNDECODABLE, UNRECOVERABLE, NOT_VALIDATOR, SEAL_BAD, SEAL_FOREIGN = range(6)


def _tr(stream, off, f0):
    return SimpleNamespace(stream=np.frombuffer(bytes(stream), np.uint8), frame_off=np.asarray(off, np.uint64),
                           inst_frame0=np.asarray(f0, np.uint64))


def _gpu_vs_ref(cfg, stream, off, f0, key_cap=0, heights=None):
    """the library's audit of a stream, asserted equal to the Python observer's in every array and counter"""
    from bftsim.runtime import Simulator
    H = cfg.heights if heights is None else heights
    sim = Simulator(cfg)                      # no secrets, no set_crypto: the observer needs neither
    try:
        got = sim.audit_trace(_tr(stream, off, f0), max_heights=H, key_cap=key_cap)
    finally:
        sim.close()
    AR.assert_same(got, AR.observe(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, H, key_cap))
    return got


@pytest.fixture(scope="module")
def cfg1():
    ref = TR.reference("cfg1")
    stream, off, meta, f0 = TR.joined(ref)
    return dict(ref=ref, cfg=ref["cfg"], stream=stream, off=off, meta=meta, f0=f0, ms=ref["inst"][0][3])


def _keyed(cfg, seed):
    from bftsim.crypto import synthetic_secrets, keyed_config, gpu_addresses
    sec = synthetic_secrets(cfg.n, seed)
    return keyed_config(cfg, sec, gpu_addresses(sec))


def _run(cfg, secrets, first, n, forged=(), log_cap=0):
    from bftsim.runtime import Simulator
    sim = Simulator(cfg)
    sim.set_crypto(secrets, forged, log_cap)
    sim.set_trace_keep(True)
    res = sim.run(first, n)
    rep = sim.crypto_verify()
    return sim, res, rep


def test_cfg1_equals_reference(cfg1):
    got = _gpu_vs_ref(cfg1["cfg"], cfg1["stream"], cfg1["off"], cfg1["f0"])
    res = cfg1["ref"]["res"]
    assert (got.frame_status == OK).all() and got.report["certified"] == 6
    assert np.array_equal(got.cert_round[0], res["round"][0]) and np.array_equal(got.cert_digest[0], res["block_hash"][0])
    assert [c[3] for c in got.certificates(0)] == [[0, 1, 2, 3]] * 6 and all(c[4] and c[5] for c in got.certificates(0))


def test_n4_equals_reference_and_key_overflow():
    ref = TR.reference("n4")
    stream, off, meta, f0 = TR.joined(ref)
    got = _gpu_vs_ref(ref["cfg"], stream, off, f0)
    forged = (meta[:, 2] & 1) != 0
    assert (got.frame_status[forged] == NOT_VALIDATOR).all() and (got.frame_status[~forged] == OK).all()
    from bftsim.trace import compare
    c = compare(got, ref["res"])
    assert int(c["certified"].sum()) == int(ref["res"]["committed_height"].sum()) == 15
    assert not c["missing"].any() and not c["different"].any() and got.report["conflicts"] == 0
    small = _gpu_vs_ref(ref["cfg"], stream, off, f0, key_cap=4)
    assert (small.inst_flags & 1).all() and small.report["key_overflows"] == 3


def test_tampered_signature_and_seal(cfg1):
    ms = cfg1["ms"]
    k = [j for j, m in enumerate(ms) if m["code"] == 3 and m["height"] == 3][1]
    fr = cfg1["stream"][int(cfg1["off"][k]):int(cfg1["off"][k + 1])]
    sig = bytearray(R.decode(fr)["signature"])
    sig[7] ^= 0x40
    stream, off = AR.splice(cfg1["stream"], cfg1["off"], k, AR.reframe(fr, signature=bytes(sig)))
    got = _gpu_vs_ref(cfg1["cfg"], stream, off, cfg1["f0"])
    assert got.frame_status[k] in (UNRECOVERABLE, NOT_VALIDATOR) and got.cert_round[0, 2] == 0xffff
    assert got.report["certified"] == 5
    d = R.decode(fr)
    seal = bytearray(d["commit_seal"])
    seal[40] ^= 0x01
    d["commit_seal"] = bytes(seal)
    d["signature"] = S.sign(ms[k]["key"], O.keccak256(R.encode(d)[2]))
    stream, off = AR.splice(cfg1["stream"], cfg1["off"], k, R.encode(d)[0])
    got = _gpu_vs_ref(cfg1["cfg"], stream, off, cfg1["f0"])
    assert got.frame_status[k] in (SEAL_BAD, SEAL_FOREIGN) and got.frame_signer[k] == int(cfg1["meta"][k, 1]) >> 16


def test_truncations_and_conflict(cfg1):
    ms = cfg1["ms"]
    ks = [[j for j, m in enumerate(ms) if m["code"] == code][0] for code in (1, 2, 3, 4)]
    cuts = AR.truncations(cfg1["stream"], cfg1["off"], ks)
    got = _gpu_vs_ref(cfg1["cfg"], *AR.appended(cfg1["stream"], cfg1["off"], cuts, new_instance=True))
    assert (got.frame_status[:71] == OK).all() and (got.frame_status[71:] == UNDECODABLE).all() and len(cuts) > 1000
    assert got.report["certified"] == 6 and (got.cert_round[1] == 0xffff).all()
    other = AR.commit_frames(cfg1["ref"]["secrets"], 2, O.keccak256(b"another block at height 2"), range(4))
    got = _gpu_vs_ref(cfg1["cfg"], *AR.appended(cfg1["stream"], cfg1["off"], other))
    assert got.inst_flags[0] == 2 and got.report["conflicts"] == 1 and got.report["certified"] == 6
    got = _gpu_vs_ref(cfg1["cfg"], *AR.appended(cfg1["stream"], cfg1["off"], other[:3]))
    assert got.inst_flags[0] == 0 and got.report["conflicts"] == 0


def test_hostile_stream_is_statuses_not_errors(cfg1):
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in rng.integers(0, 900, 200)]
    frames += [b""] * 70 + [b"\xff\xff\xff\xff" + bytes(40), b"\xff\xff\xff\xff", b"\x00\x00\x00\x00", bytes(3)]
    frames.append(rng.integers(0, 256, 40000, dtype=np.uint8).tobytes())          # far above any real frame
    big = bytearray(rng.integers(0, 256, 70000, dtype=np.uint8).tobytes())
    big[:4] = (len(big) - 4).to_bytes(4, "big")                                   # a consistent size prefix, garbage inside
    frames.append(bytes(big))
    stream, off, f0 = AR.appended(b"", np.zeros(1, np.uint64), frames)
    f0 = np.array([0, 100, 100, len(frames)], np.uint64)                          # an empty instance too
    got = _gpu_vs_ref(cfg1["cfg"], stream, off, f0)
    assert (got.frame_status == UNDECODABLE).all() and (got.frame_signer == -1).all()
    assert got.report["undecodable"] == len(frames) and got.report["certified"] == 0 and not got.inst_flags.any()


def test_last_trace_equals_exported_and_leaves_the_run_alone():
    ref = TR.reference("n4")
    sim, res, rep = _run(ref["cfg"], ref["secrets"], ref["first"], 3, ref["forged"], 1024)
    try:
        before = sim.export_trace()
        whole, part = sim.audit_last_trace(), sim.audit_last_trace(1, 2)
        via, via_part = sim.audit_trace(before), sim.audit_trace(sim.export_trace(1, 2))
        after, fetched = sim.export_trace(), sim.fetch()
        ms = sim.audit_ms()
        from bftsim.runtime import BftsimError
        with pytest.raises(BftsimError):
            sim.audit_last_trace(2, 2)                                  # past the launch
        sim.set_trace_keep(False)
        with pytest.raises(BftsimError):
            sim.audit_last_trace()                                      # keep off: what the export refuses
    finally:
        sim.close()
    for a, b in ((whole, via), (part, via_part)):
        for k in AR.ARRAYS:
            assert np.array_equal(getattr(a, k), getattr(b, k)), k
        assert a.report == b.report
    stream, off, meta, f0 = TR.joined(ref)
    AR.assert_same(whole, AR.observe(stream, off, f0, ref["cfg"].addresses, False, ref["cfg"].heights))
    assert np.array_equal(part.cert_digest, whole.cert_digest[1:]) and whole.report["not_validator"] == rep["forged"]
    assert after.stream.tobytes() == before.stream.tobytes() and np.array_equal(after.frame_off, before.frame_off)
    for k in ("committed_height", "flags", "round", "block_hash"):
        assert np.array_equal(fetched[k], res[k]), k
    assert all(x >= 0 for x in ms) and ms[1] > 0


def _certified_as_run(got, res, n):
    from bftsim.trace import compare
    c = compare(got, res)
    assert np.array_equal(c["certified"], res["committed_height"][:n].astype(np.uint32)) and c["certified"].sum() > 0
    assert not c["missing"].any() and not c["different"].any()
    assert got.report["conflicts"] == 0 and not got.inst_flags.any()
    return c


def test_n100_second_voter_word():
    """N=100, 2 heights, lossless: voter bitmaps reach the second word; certificates are the run's, at its rounds"""
    cfg, secrets = _keyed(cfg4(100, heights=2), 5)
    sim, res, rep = _run(cfg, secrets, 0, 1)
    try:
        got = sim.audit_last_trace()
    finally:
        sim.close()
    assert got.report["frames"] == rep["messages"] and got.report["ok"] == rep["messages"]
    c = _certified_as_run(got, res, 1)
    assert np.array_equal(c["same_round"], c["certified"])
    assert got.cert_voters[0, :, 1].all() and all(len(v) == 67 for _, _, _, v, _, _ in got.certificates(0))
    assert all(p and r for *_, p, r in got.certificates(0))


def test_n65_lossy():
    """N=65 (a second voter word of one bit), 2 heights, 2 % drop, 2 instances"""
    cfg, secrets = _keyed(BftConfig(n=65, heights=2, seed=9, drop_ppm=20_000), 4)
    sim, res, rep = _run(cfg, secrets, 0, 2)
    try:
        got = sim.audit_last_trace()
    finally:
        sim.close()
    assert got.report["frames"] == rep["messages"] == got.report["ok"]
    c = _certified_as_run(got, res, 2)
    for i in range(2):
        for x in range(int(res["committed_height"][i])):
            assert int(got.cert_round[i, x]) <= int(res["round"][i, x])


def test_cfg3_byzantine_no_wrong_certificate():
    """cfg3 x 4 heights x 4 instances: wildcard votes are not on the wire, so some committed heights have no
    certificate (SPEC.md §11c); none has one for another block, and nothing conflicts"""
    from bftsim.trace import compare
    cfg, secrets = _keyed(cfg3(heights=4), 3)
    sim, res, rep = _run(cfg, secrets, 0, 4, log_cap=16384)
    try:
        got = sim.audit_last_trace()
    finally:
        sim.close()
    c = compare(got, res)
    assert got.report["frames"] == rep["messages"] and got.report["ok"] + got.report["seal_foreign"] == rep["messages"]
    assert not c["different"].any() and got.report["conflicts"] == 0 and c["certified"].sum() > 0
