"""CPU reference of the observer (SPEC.md §11c), test infrastructure only: frame bytes -> statuses, signers, commit
certificates and the safety verdict, with the strict wire reference (oracle/wire_strict.py; the msgpack encoders of
oracle/wire_ref.py), the C oracle's secp256k1 recovery and Keccak-256. Independent of the code under test: no byte of it comes from csrc/."""
from __future__ import annotations

import os
import sys

import msgpack
import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import oracle_lib as O  # noqa: E402
import wire_ref as R  # noqa: E402
import wire_strict as WS  # noqa: E402

ST_OK, ST_UNDECODABLE, ST_UNRECOVERABLE, ST_NOT_VALIDATOR, ST_SEAL_BAD, ST_SEAL_FOREIGN = range(6)
KEY_OVERFLOW, CONFLICT = 1, 2
CERT_NONE, ROUND_MAX = 0xffff, 0xfffe


def _uint(x):
    if not isinstance(x, int) or isinstance(x, bool) or x < 0:
        raise ValueError
    return x


def parse(fr: bytes):
    """frame -> dict(code, round, height, digest, sign_payload, sig, seal, block) or None (UNDECODABLE): the strict
    reference of SPEC.md §9's decoder grammar with the observer's rules of §11c row 1 (oracle/wire_strict.py)"""
    return WS.observe_parse(bytes(fr))


def parse_loose(fr: bytes):
    """the same by msgpack.unpackb, which checks fewer types than the grammar: kept to cross-check `parse` on
    well-formed frames"""
    try:
        env = R._envelope(fr, R.P2P_CONSENSUS)
        if env is None:
            return None
        g = msgpack.unpackb(env[0])
        if not isinstance(g, list) or not 3 <= len(g) <= 5:
            return None
        cv, ctime, msg, sig, seal = list(g) + [None] * (5 - len(g))
        if not isinstance(cv, list) or len(cv) != 2 or cv[1] != [] or _uint(cv[0]) > 3:
            return None
        code = cv[0] + 1
        _uint(ctime)
        if sig is None:
            return None
        sig = R._bytes(sig, 65)
        seal = R._bytes(seal, 65) if seal is not None else None
        if (seal is not None) != (code == 3):
            return None
        m = msgpack.unpackb(bytes(msg))
        (rnd, height), body = m
        _uint(rnd), _uint(height)
        if code == 1:
            blk = R.block_from_obj(body)
            pm = msgpack.packb([[rnd, height], R.block_obj(blk)])
            sp = msgpack.packb([[0, []], ctime, list(pm), None, None])
            digest = O.keccak256(msgpack.packb(R.header_obj(dict(blk, votes=None))))
            return dict(code=code, round=rnd, height=height, digest=digest, sign_payload=sp, sig=sig, seal=None, block=blk)
        digest = R._bytes(body, 32)
        sp = R.gossip(code, ctime, R.subject(rnd, height, digest), None, seal)
        return dict(code=code, round=rnd, height=height, digest=digest, sign_payload=sp, sig=sig, seal=seal, block=None)
    except Exception:
        return None


def seed(h: bytes, n: int, le: bool) -> int:
    """randon_seed (validator.rs:39-48) under either reading of the 16-byte buffer"""
    return int.from_bytes(h[:8], "little") % n if le else (int.from_bytes(h[:8], "big") << 64) % n


def _recover(digests, sigs):
    if not digests:
        return []
    pubs, ok = O.secp_recover_batch(np.frombuffer(b"".join(digests), np.uint8).reshape(-1, 32),
                                    np.frombuffer(b"".join(sigs), np.uint8).reshape(-1, 65), threads=8)
    return [O.keccak256(pubs[i].tobytes())[12:] if ok[i] else None for i in range(len(digests))]


def observe(stream: bytes, frame_off, inst_frame0, addresses, seed_le: bool, max_heights: int, key_cap: int = 0) -> dict:
    """-> the arrays of bftsim.trace.Audit and `report`"""
    stream = bytes(stream)
    off = [int(x) for x in frame_off]
    f0 = [int(x) for x in inst_frame0]
    F, n_inst, H, n = len(off) - 1, len(f0) - 1, max_heights, len(addresses)
    index = {bytes(a): v for v, a in enumerate(addresses)}
    quorum = (2 * n) // 3
    cap = key_cap or 4 * H + 64
    ps = [parse(stream[off[k]:off[k + 1]]) for k in range(F)]
    good = [k for k in range(F) if ps[k] is not None]
    who = dict(zip(good, _recover([O.keccak256(ps[k]["sign_payload"]) for k in good], [ps[k]["sig"] for k in good])))
    cm = [k for k in good if ps[k]["code"] == 3]
    sealer = dict(zip(cm, _recover([O.keccak256(b"\x03" + ps[k]["digest"]) for k in cm], [ps[k]["seal"] for k in cm])))
    status, signer = np.zeros(F, np.uint8), np.full(F, -1, np.int32)
    rep = dict(frames=F, ok=0, undecodable=0, unrecoverable=0, not_validator=0, seal_bad=0, seal_foreign=0,
               by_code=[0, 0, 0, 0], out_of_range=0, certified=0, conflicts=0, key_overflows=0,
               recoveries=F + len(cm))      # the library recovers every frame's record, a zeroed one included
    names = ["ok", "undecodable", "unrecoverable", "not_validator", "seal_bad", "seal_foreign"]
    for k in range(F):
        if ps[k] is None:
            st = ST_UNDECODABLE
        elif who[k] is None:
            st = ST_UNRECOVERABLE
        elif who[k] not in index:
            st = ST_NOT_VALIDATOR
        else:
            signer[k] = index[who[k]]
            st = ST_OK
            if ps[k]["code"] == 3:
                st = ST_SEAL_BAD if sealer[k] is None else ST_SEAL_FOREIGN if sealer[k] != who[k] else ST_OK
        status[k] = st
        rep[names[st]] += 1
        if st in (ST_OK, ST_SEAL_FOREIGN):
            rep["by_code"][ps[k]["code"] - 1] += 1
    out = dict(frame_status=status, frame_signer=signer, inst_flags=np.zeros(n_inst, np.uint32),
               cert_round=np.full((n_inst, H), CERT_NONE, np.uint16), cert_digest=np.zeros((n_inst, H, 32), np.uint8),
               cert_voters=np.zeros((n_inst, H, 4), np.uint64), cert_frame=np.zeros((n_inst, H), np.uint32),
               cert_flags=np.zeros((n_inst, H), np.uint8), report=rep)
    for i in range(n_inst):
        keys, cert, flags = {}, {}, 0
        for k in range(f0[i], f0[i + 1]):
            p = ps[k]
            if status[k] not in (ST_OK, ST_SEAL_FOREIGN) or p["code"] not in (1, 3):
                continue
            h = p["height"]
            if not 1 <= h <= H:
                rep["out_of_range"] += 1
                continue
            key = (h, p["round"], p["digest"])
            if p["code"] == 3 and cert.get(h) == p["digest"]:
                continue
            if key not in keys:
                if len(keys) == cap:
                    flags |= KEY_OVERFLOW
                    continue
                keys[key] = dict(voters=set(), proposed=False, rightful=False)
            e = keys[key]
            s = int(signer[k])
            if p["code"] == 1:
                b = p["block"]
                want = (seed(b["prev_hash"], n, seed_le) + p["round"] % n) % n
                e["proposed"] = True
                e["rightful"] = e["rightful"] or (s == want and b["proposer"] == bytes(addresses[s]))
                continue
            if s in e["voters"]:
                continue
            e["voters"].add(s)
            if len(e["voters"]) != quorum + 1:
                continue
            if h in cert:
                flags |= CONFLICT
                rep["conflicts"] += 1
                continue
            cert[h] = p["digest"]
            rep["certified"] += 1
            out["cert_round"][i, h - 1] = min(p["round"], ROUND_MAX)
            out["cert_digest"][i, h - 1] = np.frombuffer(p["digest"], np.uint8)
            for v in e["voters"]:
                out["cert_voters"][i, h - 1, v >> 6] |= np.uint64(1 << (v & 63))
            out["cert_frame"][i, h - 1] = k - f0[i]
            out["cert_flags"][i, h - 1] = (1 if e["proposed"] else 0) | (2 if e["rightful"] else 0)
        out["inst_flags"][i] = flags
        rep["key_overflows"] += 1 if flags & KEY_OVERFLOW else 0
    return out


# ---- tampering (the tests' hostile inputs), by re-encoding a decoded frame with the msgpack oracle
def reframe(fr: bytes, **changes) -> bytes:
    """a Subject frame with fields replaced (signature=, commit_seal=, digest=, ...)"""
    d = R.decode(fr)
    d.update(changes)
    return R.encode(d)[0]


def splice(stream: bytes, frame_off, k: int, new: bytes):
    """the stream with frame k replaced -> (stream, frame_off)"""
    off = [int(x) for x in frame_off]
    s = stream[:off[k]] + new + stream[off[k + 1]:]
    d = len(new) - (off[k + 1] - off[k])
    return s, np.array(off[:k + 1] + [o + d for o in off[k + 1:]], np.uint64)


ARRAYS = ("frame_status", "frame_signer", "inst_flags", "cert_round", "cert_digest", "cert_voters", "cert_frame",
          "cert_flags")


def assert_same(got, want):
    """every output array and the report of an observer run (a dict, or a bftsim.trace.Audit) equal the reference's"""
    for k in ARRAYS:
        g = got[k] if isinstance(got, dict) else getattr(got, k)
        assert np.array_equal(np.asarray(g).reshape(want[k].shape), want[k]), k
    rep = got["report"] if isinstance(got, dict) else got.report
    assert {k: (list(v) if isinstance(v, (list, tuple)) else int(v)) for k, v in rep.items()} == want["report"]



# ---- the hostile variants of a trace_ref.reference() that the CPU and the GPU tests share
def commit_frames(secrets, height: int, digest: bytes, voters, round_: int = 0) -> list:
    """Commit frames for (height, round, digest) signed here with the validators' keys (Python secp256k1 oracle)"""
    import secp256k1_ref as S
    out = []
    for v in voters:
        d = dict(code=3, create_time=0, round=round_, height=height, digest=digest)
        d["commit_seal"] = S.sign(secrets[v], O.keccak256(b"\x03" + digest))
        d["signature"] = S.sign(secrets[v], O.keccak256(R.encode(d)[2]))
        out.append(R.encode(d)[0])
    return out


def appended(stream: bytes, frame_off, frames, new_instance: bool = False):
    """the one-instance stream with `frames` appended (to it, or as a second instance) -> (stream, frame_off, inst_frame0)"""
    offs, n0 = [int(x) for x in frame_off], len(frame_off) - 1
    for f in frames:
        stream += f
        offs.append(len(stream))
    f0 = [0, n0, len(offs) - 1] if new_instance else [0, len(offs) - 1]
    return stream, np.array(offs, np.uint64), np.array(f0, np.uint64)


def truncations(stream: bytes, frame_off, ks) -> list:
    """frames ks cut at every length below their own"""
    out = []
    for k in ks:
        fr = stream[int(frame_off[k]):int(frame_off[k + 1])]
        out += [fr[:cut] for cut in range(len(fr))]
    return out
