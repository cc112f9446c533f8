"""CPU: the observer's per-frame parsing, classification and tally step (consensus-rs_amd/csrc/bft_audit.h, host
build tests/emu/audit_host.cpp, recoveries from the C oracle) against the independent Python observer
(tests/audit_ref.py) and the oracle's run, over the reference traces of tests/trace_ref.py and hostile variants of them;
the parser as a stand-alone program under ASan + UBSan; the C ABI's bindings and argument checks."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import trace_ref as TR          # first: it puts oracle/ on the path
import audit_lib as AL
import audit_ref as AR
import oracle_lib as O
import secp256k1_ref as S
import wire_ref as R

OK, UNDECODABLE, UNRECOVERABLE, NOT_VALIDATOR, SEAL_BAD, SEAL_FOREIGN = range(6)


def _both(ref, stream, off, f0, key_cap=0):
    """(host build, Python reference) over one stream, asserted equal"""
    cfg = ref["cfg"]
    got = AL.observe(stream, off, f0, cfg, cfg.heights, key_cap)
    want = AR.observe(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, cfg.heights, key_cap)
    AR.assert_same(got, want)
    return got


@pytest.fixture(scope="module")
def cfg1():
    ref = TR.reference("cfg1")
    stream, off, meta, f0 = TR.joined(ref)
    return dict(ref=ref, stream=stream, off=off, meta=meta, f0=f0, got=_both(ref, stream, off, f0))


@pytest.fixture(scope="module")
def n4():
    ref = TR.reference("n4")
    stream, off, meta, f0 = TR.joined(ref)
    return dict(ref=ref, stream=stream, off=off, meta=meta, f0=f0, got=_both(ref, stream, off, f0))


def _voters(got, i, x):
    w = got["cert_voters"][i, x - 1]
    return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]


def test_cfg1_statuses_signers_certificates(cfg1):
    """71 frames, N=5, 6 heights: every frame OK and signed by its sender; 6 certificates equal to the oracle's
    (round, block_hash), each by exactly the 4 running validators, proposed by the rightful proposer"""
    got, res, meta = cfg1["got"], cfg1["ref"]["res"], cfg1["meta"]
    assert len(meta) == 71 and got["report"]["frames"] == 71
    assert (got["frame_status"] == OK).all() and got["report"]["ok"] == 71
    assert np.array_equal(got["frame_signer"], (meta[:, 1] >> 16).astype(np.int32))
    assert int(res["committed_height"][0]) == 6 and got["report"]["certified"] == 6
    assert np.array_equal(got["cert_round"][0], res["round"][0])
    assert np.array_equal(got["cert_digest"][0], res["block_hash"][0])
    for x in range(1, 7):
        assert _voters(got, 0, x) == [0, 1, 2, 3]                       # c5 is silent
    assert (got["cert_flags"] == 3).all()
    assert got["inst_flags"][0] == 0 and got["report"]["conflicts"] == 0
    ms = cfg1["ref"]["inst"][0][3]                                      # the run goes on into height 7 before it stops
    assert got["report"]["out_of_range"] == sum(1 for m in ms if m["code"] in (1, 3) and not 1 <= m["height"] <= 6)
    codes = (meta[:, 1] >> 8) & 0xff
    assert got["report"]["by_code"] == [int((codes == c).sum()) for c in (1, 2, 3, 4)]
    assert got["report"]["recoveries"] == 71 + int((codes == 3).sum())
    # the certificate completes at the fourth Commit of its key
    cm = np.nonzero(codes == 3)[0]
    assert [int(k) for k in got["cert_frame"][0]] == [int(cm[4 * x + 3]) for x in range(6)]


def test_n4_forged_lossy(n4):
    """instances 3..5, 1,016 frames, 10 % drop, validator 2 forged: forged frames NOT_VALIDATOR, every committed
    height certified with the committed hash, no conflicts"""
    got, res, meta = n4["got"], n4["ref"]["res"], n4["meta"]
    forged = (meta[:, 2] & 1) != 0
    assert len(meta) == 1016 and forged.any()
    assert (got["frame_status"][forged] == NOT_VALIDATOR).all() and (got["frame_signer"][forged] == -1).all()
    assert (got["frame_status"][~forged] == OK).all()
    assert np.array_equal(got["frame_signer"][~forged], (meta[~forged, 1] >> 16).astype(np.int32))
    committed = 0
    for i in range(3):
        for x in range(int(res["committed_height"][i])):
            committed += 1
            assert got["cert_round"][i, x] != 0xffff, (i, x)
            assert np.array_equal(got["cert_digest"][i, x], res["block_hash"][i, x]), (i, x)
            assert int(got["cert_round"][i, x]) <= int(res["round"][i, x])
            assert 2 not in _voters(got, i, x + 1)
    assert committed == 15
    assert (got["inst_flags"] == 0).all() and got["report"]["conflicts"] == 0 and got["report"]["key_overflows"] == 0


def _commit_of_height(cfg1, x, nth=0):
    ms = cfg1["ref"]["inst"][0][3]
    return [k for k, m in enumerate(ms) if m["code"] == 3 and m["height"] == x][nth]


def test_flipped_signature_byte_loses_the_certificate(cfg1):
    k = _commit_of_height(cfg1, 3, 1)
    fr = cfg1["stream"][int(cfg1["off"][k]):int(cfg1["off"][k + 1])]
    sig = bytearray(R.decode(fr)["signature"])
    sig[7] ^= 0x40
    stream, off = AR.splice(cfg1["stream"], cfg1["off"], k, AR.reframe(fr, signature=bytes(sig)))
    got = _both(cfg1["ref"], stream, off, cfg1["f0"])
    assert got["frame_status"][k] in (UNRECOVERABLE, NOT_VALIDATOR) and got["frame_signer"][k] == -1
    assert (np.delete(got["frame_status"], k) == OK).all()
    assert got["cert_round"][0, 2] == 0xffff and not got["cert_digest"][0, 2].any()
    assert (np.delete(got["cert_round"][0], 2) != 0xffff).all() and got["report"]["certified"] == 5


def test_flipped_seal_byte(cfg1):
    k = _commit_of_height(cfg1, 2, 0)
    fr = cfg1["stream"][int(cfg1["off"][k]):int(cfg1["off"][k + 1])]
    seal = bytearray(R.decode(fr)["commit_seal"])
    seal[40] ^= 0x01
    stream, off = AR.splice(cfg1["stream"], cfg1["off"], k, AR.reframe(fr, commit_seal=bytes(seal)))
    got = _both(cfg1["ref"], stream, off, cfg1["f0"])
    # the seal is part of the sign payload: the frame's own signature no longer covers it either
    assert got["frame_status"][k] in (UNRECOVERABLE, NOT_VALIDATOR, SEAL_BAD, SEAL_FOREIGN)
    # a frame signed over the tampered seal: the signature recovers, the seal does not match
    m = cfg1["ref"]["inst"][0][3][k]
    d = R.decode(fr)
    d["commit_seal"] = bytes(seal)
    d["signature"] = S.sign(m["key"], O.keccak256(R.encode(d)[2]))
    stream, off = AR.splice(cfg1["stream"], cfg1["off"], k, R.encode(d)[0])
    got = _both(cfg1["ref"], stream, off, cfg1["f0"])
    assert got["frame_status"][k] in (SEAL_BAD, SEAL_FOREIGN)
    assert got["frame_signer"][k] == (int(cfg1["meta"][k, 1]) >> 16)
    assert got["report"]["seal_bad"] + got["report"]["seal_foreign"] == 1
    if got["frame_status"][k] == SEAL_BAD:                              # dropped: its height loses the certificate
        assert got["cert_round"][0, 1] == 0xffff
    else:                                                               # accepted and counted apart
        assert got["cert_round"][0, 1] != 0xffff


def test_every_truncation_is_undecodable(cfg1):
    """one frame of each kind cut at every length, each cut a frame of a second instance of the stream"""
    ms = cfg1["ref"]["inst"][0][3]
    stream, offs, n0 = cfg1["stream"], [int(x) for x in cfg1["off"]], len(ms)
    for code in (1, 2, 3, 4):
        k = [j for j, m in enumerate(ms) if m["code"] == code][0]
        fr = cfg1["stream"][offs[k]:offs[k + 1]]
        for cut in range(len(fr)):
            stream += fr[:cut]
            offs.append(len(stream))
    f0 = np.array([0, n0, len(offs) - 1], np.uint64)
    got = _both(cfg1["ref"], stream, np.array(offs, np.uint64), f0)
    assert (got["frame_status"][:n0] == OK).all()
    assert (got["frame_status"][n0:] == UNDECODABLE).all() and (got["frame_signer"][n0:] == -1).all()
    assert got["report"]["undecodable"] == len(offs) - 1 - n0 > 1000
    assert np.array_equal(got["cert_digest"][0], cfg1["got"]["cert_digest"][0]) and (got["cert_round"][1] == 0xffff).all()


def test_second_quorum_is_a_conflict(cfg1):
    """height 2 again: a quorum of Commits for another digest, signed here with the reference keys"""
    ref = cfg1["ref"]
    other = O.keccak256(b"another block at height 2")
    extra = b""
    offs = [int(x) for x in cfg1["off"]]
    stream = cfg1["stream"]
    for v in range(4):
        key = ref["secrets"][v]
        d = dict(code=3, create_time=0, round=0, height=2, digest=other)
        d["commit_seal"] = S.sign(key, O.keccak256(b"\x03" + other))
        d["signature"] = S.sign(key, O.keccak256(R.encode(d)[2]))
        stream += R.encode(d)[0]
        offs.append(len(stream))
    del extra
    f0 = np.array([0, len(offs) - 1], np.uint64)
    got = _both(ref, stream, np.array(offs, np.uint64), f0)
    assert (got["frame_status"] == OK).all()
    assert got["inst_flags"][0] == 2 and got["report"]["conflicts"] == 1 and got["report"]["certified"] == 6
    assert np.array_equal(got["cert_digest"], cfg1["got"]["cert_digest"])          # the certificate stays the first one
    # three of them are no quorum
    got = _both(ref, stream[:offs[-2]], np.array(offs[:-1], np.uint64), np.array([0, len(offs) - 2], np.uint64))
    assert got["inst_flags"][0] == 0 and got["report"]["conflicts"] == 0


def test_key_overflow_is_deterministic(n4):
    got = _both(n4["ref"], n4["stream"], n4["off"], n4["f0"], key_cap=4)
    assert (got["inst_flags"] & 1).all() and got["report"]["key_overflows"] == 3
    assert got["report"]["certified"] < n4["got"]["report"]["certified"]
    assert np.array_equal(got["frame_status"], n4["got"]["frame_status"])


def test_heights_out_of_range_are_counted_not_tallied(cfg1):
    cfg = cfg1["ref"]["cfg"]
    got = AL.observe(cfg1["stream"], cfg1["off"], cfg1["f0"], cfg, 4)
    want = AR.observe(cfg1["stream"], cfg1["off"], cfg1["f0"], cfg.addresses, False, 4)
    AR.assert_same(got, want)
    codes = (cfg1["meta"][:, 1] >> 8) & 0xff
    ms = cfg1["ref"]["inst"][0][3]
    assert got["report"]["out_of_range"] == sum(1 for m in ms if m["code"] in (1, 3) and m["height"] > 4) > 0
    assert got["report"]["certified"] == 4 and len(codes) == 71


@pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")
def test_parser_program_under_asan_ubsan(cfg1):
    """the stand-alone program (its own main, run directly): every truncation and every single-byte flip of one frame
    of each kind, parsed from heap buffers of exactly the frame's length"""
    exe = AL.build_san()
    ms = cfg1["ref"]["inst"][0][3]
    frames = []
    for code in (1, 2, 3, 4):
        k = [j for j, m in enumerate(ms) if m["code"] == code][0]
        frames.append(cfg1["stream"][int(cfg1["off"][k]):int(cfg1["off"][k + 1])])
    cfg = cfg1["ref"]["cfg"]
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0", UBSAN_OPTIONS="print_stacktrace=1:halt_on_error=1")
    r = subprocess.run([exe], input=AL.san_input(cfg.address_bytes(), cfg.n, frames), capture_output=True, env=env, timeout=300)
    assert r.returncode == 0, (r.returncode, r.stdout[-2000:], r.stderr[-4000:])
    cases = sum(len(f) for f in frames) * 4
    assert r.stdout.decode().strip() == f"ok 4 frames {cases} cases"
    assert b"runtime error" not in r.stderr and b"AddressSanitizer" not in r.stderr, r.stderr[-4000:]


def test_entry_points_are_bound_and_check_arguments():
    """bound, a null handle or report refused, and argument errors are BFTSIM_EINVAL before any device work (this
    runs without a GPU: the handle of a create that could not reach a device still checks arguments)"""
    from bftsim import _abi, runtime, trace
    from bftsim.configs import cfg1 as mk
    L = runtime.lib()
    rep = _abi.CAuditReport()
    assert L.bftsim_audit_trace(None, None, 0, None, 0, None, 0, 1, 0, None, ctypes.byref(rep)) == -1
    assert L.bftsim_audit_last_trace(None, 0, 0, 0, None, ctypes.byref(rep)) == -1
    assert L.bftsim_audit_last_ms(None, None, None, None, None) == -1
    assert hasattr(runtime.Simulator, "audit_trace") and hasattr(runtime.Simulator, "audit_last_trace")
    assert callable(trace.compare) and callable(trace.audit) and hasattr(trace.Audit, "certificates")
    c, keep = _abi.to_cconfig(mk(True, heights=6))
    h = ctypes.c_void_p()
    L.bftsim_create(ctypes.byref(c), 0, ctypes.byref(h))
    assert h.value
    stream = np.zeros(16, np.uint8)

    def call(off, f0, frames=2, inst=1, heights=6, rep=rep, nbytes=16):
        off, f0 = np.array(off, np.uint64), np.array(f0, np.uint64)
        return L.bftsim_audit_trace(h, stream.ctypes.data, nbytes, off.ctypes.data, frames, f0.ctypes.data, inst, heights, 0,
                                    None, ctypes.byref(rep) if rep is not None else None)

    rep.frames = 77
    assert call([0, 8, 16], [0, 2], rep=None) == -1                     # null report
    assert call([0, 9, 8], [0, 2], nbytes=8) == -1                      # frame_off decreases
    assert call([0, 8, 15], [0, 2]) == -1                               # does not end at stream_bytes
    assert call([0, 8, 16], [1, 2]) == -1                               # inst_frame0 does not start at 0
    assert call([0, 8, 16], [0, 1]) == -1                               # ... or end at frames
    assert call([0, 8, 16], [0, 2, 1, 2], inst=3) == -1                 # ... or decreases
    assert call([0, 8, 16], [0, 2], heights=0) == -1
    assert call([0, 8, 16], [0, 2], heights=65536) == -1
    assert call([0, 8, 16], [0, 2], frames=1 << 32) == -1
    assert len(L.bftsim_last_error(h)) > 0 and rep.frames == 77         # nothing written
    del keep


def test_new_structs_bound_in_integration_md():
    """bftsim_audit_report / bftsim_audit_out: INTEGRATION.md's #[repr(C)] structs against the header, by the checker of
    test_integration_binding (field names, types, offsets and sizes as gcc lays them out); the ctypes mirrors too"""
    import re
    import test_integration_binding as B
    from bftsim import _abi
    txt = re.sub(r"struct (bftsim_audit_\w+) \{(.*?)\};\s*typedef struct \1 \1;", r"typedef struct \1 {\2} \1;",
                 B.header_text(), flags=re.S)
    decls = {k: v for k, v in B.c_struct_decls(txt).items() if k.startswith("bftsim_audit_")}
    assert set(decls) == {"bftsim_audit_report", "bftsim_audit_out"}
    src = B.strip_rust_comments(B.rust_blocks())
    rs, consts = B.rust_structs(src), B.rust_consts(src)
    lay = B.gcc_layout({k: [f for f, _ in v] for k, v in decls.items()})
    for name, fields in decls.items():
        assert [f for f, _ in rs[name]] == [f for f, _ in fields], name
        assert [B.canon_rust(B.parse_rust_type(t), consts) for _, t in rs[name]] == \
            [t.replace("int32_t", "i32") for _, t in fields], name       # the checker's table has no int32_t
        size, _, offs = B.struct_layout(name, rs, consts, {})
        assert size == lay[(name, "sizeof")]
        for f, o in offs.items():
            assert o == lay[(name, f)], (name, f)
    for name, cls in (("bftsim_audit_report", _abi.CAuditReport), ("bftsim_audit_out", _abi.CAuditOut)):
        assert ctypes.sizeof(cls) == lay[(name, "sizeof")]
        assert [f for f, _ in cls._fields_] == [f for f, _ in decls[name]]
        for f, _ in cls._fields_:
            assert getattr(cls, f).offset == lay[(name, f)], (name, f)
    for k in ("BFTSIM_AUDIT_KEY_OVERFLOW", "BFTSIM_AUDIT_CONFLICT", "BFTSIM_AUDIT_SEAL_FOREIGN"):
        assert k in consts
