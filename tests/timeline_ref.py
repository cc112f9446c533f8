"""CPU reference of the chronicler (SPEC.md §11h), test infrastructure only: frame bytes -> per height the first prepare
certificate, the round-change quorums and the three verdicts that join them to the observer's commit certificate.
Statuses, signers and certificates are audit_ref.observe's, the fields audit_ref.parse's; the rule itself is a dictionary
per key, written from the SPEC text. Independent of the code under test."""
from __future__ import annotations

import numpy as np

import audit_ref as AR

NONE16, ROUND_MAX = 0xffff, 0xfffe
KEY_OVERFLOW = 1
PREPARED_FIRST, CERT_UNPREPARED, LOCKED_OPEN = 1, 2, 4
ROWS = ("prep_round", "prep_digest", "prep_voters", "prep_frame", "prep_quorums", "rc_quorums", "rc_max_round",
        "rc_max_frame", "rc_top_round", "rc_frames", "flags")
ARRAYS = ROWS + ("inst_flags", "open_height")
REPORT = ("prepare_frames", "rc_frames", "out_of_range", "prepared", "rc_quorums", "rc_heights", "prepared_first",
          "cert_unprepared", "locked_open", "key_overflows")


def _clip(r: int) -> int:
    return min(r, ROUND_MAX)


def timeline(stream, frame_off, inst_frame0, addresses, seed_le: bool, max_heights: int, tl_cap: int = 0, audit=None) -> dict:
    """-> the arrays of bftsim.trace.Timeline ([n, H, ...]), report, audit (audit_ref.observe's, or the one passed in:
    frame_status, frame_signer, cert_round, cert_digest, cert_frame)"""
    stream = bytes(stream)
    off = [int(x) for x in frame_off]
    f0 = [int(x) for x in inst_frame0]
    n_inst, H, n = len(f0) - 1, max_heights, len(addresses)
    a = audit or AR.observe(stream, off, f0, addresses, seed_le, H)
    quorum = (2 * n) // 3
    cap = tl_cap or 4 * H + 64
    cert_round = np.asarray(a["cert_round"]).reshape(n_inst, H)
    cert_digest = np.asarray(a["cert_digest"]).reshape(n_inst, H, 32)
    cert_frame = np.asarray(a["cert_frame"]).reshape(n_inst, H)
    out = dict(prep_round=np.full((n_inst, H), NONE16, np.uint16), prep_digest=np.zeros((n_inst, H, 32), np.uint8),
               prep_voters=np.zeros((n_inst, H, 4), np.uint64), prep_frame=np.zeros((n_inst, H), np.uint32),
               prep_quorums=np.zeros((n_inst, H), np.uint16), rc_quorums=np.zeros((n_inst, H), np.uint16),
               rc_max_round=np.full((n_inst, H), NONE16, np.uint16), rc_max_frame=np.zeros((n_inst, H), np.uint32),
               rc_top_round=np.full((n_inst, H), NONE16, np.uint16), rc_frames=np.zeros((n_inst, H), np.uint32),
               flags=np.zeros((n_inst, H), np.uint8), inst_flags=np.zeros(n_inst, np.uint32),
               open_height=np.full(n_inst, H + 1, np.uint32))
    rep = dict.fromkeys(REPORT, 0)
    for i in range(n_inst):
        keys = {}                                   # key -> dict(voters, done: the completing frame or None); ordered
        pq, rq = {}, {}                             # height -> [(round, digest, frame)] / [(round, frame)] in quorum order
        top, rcf = {}, {}
        for k in range(f0[i], f0[i + 1]):
            if a["frame_status"][k] not in (AR.ST_OK, AR.ST_SEAL_FOREIGN):
                continue
            p = AR.parse(stream[off[k]:off[k + 1]])
            if p["code"] not in (2, 4):
                continue
            h = p["height"]
            if not 1 <= h <= H:
                rep["out_of_range"] += 1
                continue
            rep["prepare_frames" if p["code"] == 2 else "rc_frames"] += 1
            key = (2, h, p["round"], p["digest"]) if p["code"] == 2 else (4, h, p["round"])
            if key not in keys:
                if len(keys) == cap:
                    out["inst_flags"][i] |= KEY_OVERFLOW
                    continue
                keys[key] = dict(voters=set(), done=None)
            if p["code"] == 4:
                rcf[h] = rcf.get(h, 0) + 1
                top[h] = max(top.get(h, 0), p["round"])
            e = keys[key]
            if e["done"] is not None:               # frozen at the completing frame
                continue
            e["voters"].add(int(a["frame_signer"][k]))
            if len(e["voters"]) <= quorum:
                continue
            e["done"] = k - f0[i]
            if p["code"] == 2:
                pq.setdefault(h, []).append((p["round"], p["digest"], k - f0[i], sorted(e["voters"])))
            else:
                rq.setdefault(h, []).append((p["round"], k - f0[i]))
        rep["key_overflows"] += int(out["inst_flags"][i] & KEY_OVERFLOW)
        for x in range(1, H + 1):
            r = x - 1
            if x in pq:
                rnd, dig, fr, voters = pq[x][0]
                out["prep_round"][i, r], out["prep_frame"][i, r] = _clip(rnd), fr
                out["prep_digest"][i, r] = np.frombuffer(dig, np.uint8)
                for v in voters:
                    out["prep_voters"][i, r, v >> 6] |= np.uint64(1 << (v & 63))
                out["prep_quorums"][i, r] = min(len(pq[x]), 0xffff)
                rep["prepared"] += 1
            if x in rq:
                rnd, fr = max(rq[x])
                out["rc_quorums"][i, r] = min(len(rq[x]), 0xffff)
                out["rc_max_round"][i, r], out["rc_max_frame"][i, r] = _clip(rnd), fr
                rep["rc_quorums"] += len(rq[x])
                rep["rc_heights"] += 1
            if x in top:
                out["rc_top_round"][i, r], out["rc_frames"][i, r] = _clip(top[x]), rcf[x]
            fl = 0
            if int(cert_round[i, r]) != NONE16:
                cf = int(cert_frame[i, r])
                cd = bytes(cert_digest[i, r])
                full = AR.parse(stream[off[f0[i] + cf]:off[f0[i] + cf + 1]])["round"]
                same = [q for q in pq.get(x, []) if q[1] == cd]
                if any(q[0] == full and q[2] < cf for q in same):
                    fl |= PREPARED_FIRST
                if not same:
                    fl |= CERT_UNPREPARED
            else:
                out["open_height"][i] = min(int(out["open_height"][i]), x)
                if x in pq:
                    fl |= LOCKED_OPEN
            out["flags"][i, r] = fl
            rep["prepared_first"] += bool(fl & PREPARED_FIRST)
            rep["cert_unprepared"] += bool(fl & CERT_UNPREPARED)
            rep["locked_open"] += bool(fl & LOCKED_OPEN)
    return dict(out, report={k: int(v) for k, v in rep.items()}, audit=a)


def stalled(t, i: int) -> bool:
    x = int(t["open_height"][i])
    H = t["flags"].shape[1]
    return x <= H and bool(int(t["flags"][i, x - 1]) & LOCKED_OPEN or int(t["rc_quorums"][i, x - 1]) > 0)


def assert_same(got, want):
    """every output array and the report of a chronicler run (a dict, or a bftsim.trace.Timeline) equal the reference's"""
    for k in ARRAYS:
        if isinstance(got, dict):
            g = got[k]
        else:
            g = got.open_heights if k == "open_height" else getattr(got, k)
        g = np.asarray(g)
        assert g.dtype == want[k].dtype, (k, g.dtype)
        assert np.array_equal(g.reshape(want[k].shape), want[k]), (k, g.reshape(want[k].shape), want[k])
    rep = got["report"] if isinstance(got, dict) else got.report
    assert {k: int(v) for k, v in rep.items()} == want["report"], (rep, want["report"])
