"""CPU reference of the accuser (SPEC.md §11g), test infrastructure only: frame bytes -> the evidence records of every
validator that signed two digests for one (code, height, round). Statuses and signers are audit_ref.observe's, the
fields audit_ref.parse's; the rule itself is a dictionary per group. Independent of the code under test."""
from __future__ import annotations

import numpy as np

import audit_ref as AR

NONE = 0xffffffff
VIEW_OVERFLOW = 1
RECORD = np.dtype([("round", "<u8"), ("inst", "<u4"), ("height", "<u4"), ("signer", "<u4"), ("code", "<u4"),
                   ("frame_a", "<u4"), ("frame_b", "<u4")])
ARRAYS = ("frame_pair", "inst_accused", "inst_flags", "records")


def accuse(stream, frame_off, inst_frame0, addresses, seed_le: bool, max_heights: int, view_cap: int = 0,
           rec_cap=None, audit=None) -> dict:
    """-> frame_pair [F] u32, inst_accused [n, 4] u64, inst_flags [n] u32, records (RECORD, the first rec_cap of them),
    report, audit (audit_ref.observe's, or the one passed in)"""
    stream = bytes(stream)
    off = [int(x) for x in frame_off]
    f0 = [int(x) for x in inst_frame0]
    F, n_inst, H = len(off) - 1, len(f0) - 1, max_heights
    a = audit or AR.observe(stream, off, f0, addresses, seed_le, H)
    cap = view_cap or 2 * H + 64
    pair = np.full(F, NONE, np.uint32)
    accused, flags = np.zeros((n_inst, 4), np.uint64), np.zeros(n_inst, np.uint32)
    recs = []
    for i in range(n_inst):
        views, first, done = [], {}, set()
        for k in range(f0[i], f0[i + 1]):
            if a["frame_status"][k] not in (AR.ST_OK, AR.ST_SEAL_FOREIGN):
                continue
            p = AR.parse(stream[off[k]:off[k + 1]])
            if p["code"] not in (1, 2, 3) or not 1 <= p["height"] <= H:
                continue
            view = (p["height"], p["round"])
            if view not in views:
                if len(views) == cap:
                    flags[i] |= VIEW_OVERFLOW
                    continue
                views.append(view)
            s = int(a["frame_signer"][k])
            g = (s, p["code"]) + view
            if g not in first:
                first[g] = (k, p["digest"])
            elif g not in done and first[g][1] != p["digest"]:
                done.add(g)
                pair[k] = first[g][0]
                accused[i, s >> 6] |= np.uint64(1 << (s & 63))
                recs.append((p["round"], i, p["height"], s, p["code"], first[g][0], k))
    report = dict(records=len(recs), by_code=[sum(r[4] == c for r in recs) for c in (1, 2, 3)],
                  accused=sum(bin(int(w)).count("1") for w in accused.ravel()),
                  accused_instances=int(accused.any(axis=1).sum()) if n_inst else 0,
                  view_overflows=int((flags & VIEW_OVERFLOW != 0).sum()))
    keep = recs if rec_cap is None else recs[:rec_cap]
    return dict(frame_pair=pair, inst_accused=accused, inst_flags=flags, records=np.array(keep, RECORD).reshape(-1),
                report=report, audit=a)


def accused(ref, i) -> list:
    return [v for v in range(256) if (int(ref["inst_accused"][i, v >> 6]) >> (v & 63)) & 1]


def assert_same(got, want):
    """every output array and the report of an accuser run (a dict, or a bftsim.trace.Accusation) equal the reference's"""
    for k in ARRAYS:
        g = np.asarray(got[k] if isinstance(got, dict) else getattr(got, k))
        if k == "records":
            assert g.dtype == RECORD and g.tolist() == want[k].tolist(), k
        else:
            assert np.array_equal(g.reshape(want[k].shape), want[k]), k
    rep = got["report"] if isinstance(got, dict) else got.report
    assert {k: (list(v) if isinstance(v, (list, tuple)) else int(v)) for k, v in rep.items()} == want["report"]


# ---- hand-made streams, signed here (Python secp256k1 oracle), that the CPU and the GPU tests share
def vote_frame(secret, code: int, height: int, round_: int, digest: bytes, seal_secret=None) -> bytes:
    """a Prepare / Commit / RoundChange frame for (height, round, digest) signed with `secret`; a Commit's seal with
    seal_secret (another key: SEAL_FOREIGN)"""
    import oracle_lib as O
    import secp256k1_ref as S
    import wire_ref as R
    d = dict(code=code, create_time=0, round=round_, height=height, digest=digest)
    if code == 3:
        d["commit_seal"] = S.sign(seal_secret or secret, O.keccak256(b"\x03" + digest))
    d["signature"] = S.sign(secret, O.keccak256(R.encode(d)[2]))
    return R.encode(d)[0]


def stream_of(instances):
    """[[frame, ...], ...] -> (stream, frame_off, inst_frame0)"""
    frames = [f for inst in instances for f in inst]
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    f0 = np.zeros(len(instances) + 1, np.uint64)
    f0[1:] = np.cumsum([len(inst) for inst in instances])
    return b"".join(frames), off, f0
