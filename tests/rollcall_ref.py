"""CPU reference of the roll call (SPEC.md §11i), test infrastructure only: frame bytes -> per (instance, validator) what
it signed, and per due view its proposer and whether that proposer's PrePrepare is in the instance. Statuses, signers
and certificates are audit_ref.observe's, the fields audit_ref.parse's, the seed audit_ref.seed; the quorate
RoundChange keys are recomputed here by the chronicler's rule (SPEC.md §11h: one table of Prepare and RoundChange keys
per instance under tl_cap, a key frozen at its completing frame) and checked against timeline_ref.timeline's rows. The
rule itself is dictionaries, written from the SPEC text. Independent of the code under test."""
from __future__ import annotations

import numpy as np

import audit_ref as AR
import timeline_ref as TL

NONE = 0xffffffff
PROPOSED, MISSED, UNATTRIBUTED, WON = 1, 2, 3, 0x100
PARTIAL = 1
ROWS = ("frames", "last_height", "last_frame", "due", "proposed", "missed", "won")
ARRAYS = ROWS + ("inst_views", "inst_silent", "inst_flags")
REPORT = ("frames", "out_of_range", "views", "by_outcome", "won", "silent", "silent_instances", "partial_instances")
RECORD = np.dtype([("round", "<u8"), ("inst", "<u4"), ("height", "<u4"), ("proposer", "<u4"), ("outcome", "<u4"),
                   ("start_frame", "<u4"), ("pp_frame", "<u4")])


def rc_quorums(stream, off, f0, audit, n: int, H: int, cap: int, i: int):
    """the chronicler's walk of instance i -> ({(height, round): completing frame} of the quorate RoundChange keys,
    the table overflowed)"""
    quorum = (2 * n) // 3
    keys, done, over = {}, {}, False
    for k in range(f0[i], f0[i + 1]):
        if audit["frame_status"][k] not in (AR.ST_OK, AR.ST_SEAL_FOREIGN):
            continue
        p = AR.parse(stream[off[k]:off[k + 1]])
        if p["code"] not in (2, 4) or not 1 <= p["height"] <= H:
            continue
        key = (2, p["height"], p["round"], p["digest"]) if p["code"] == 2 else (4, p["height"], p["round"])
        if key not in keys:
            if len(keys) == cap:
                over = True
                continue
            keys[key] = set()
        if key in done:
            continue
        keys[key].add(int(audit["frame_signer"][k]))
        if len(keys[key]) > quorum:
            done[key] = k - f0[i]
    return {(key[1], key[2]): fr for key, fr in done.items() if key[0] == 4}, over


def rollcall(stream, frame_off, inst_frame0, addresses, seed_le: bool, genesis: bytes, max_heights: int, tl_cap: int = 0,
             audit=None) -> dict:
    """-> the arrays of bftsim.trace.RollCall ([n, N, ...]), records (all of them), report, audit (audit_ref.observe's,
    or the one passed in)"""
    stream = bytes(stream)
    off = [int(x) for x in frame_off]
    f0 = [int(x) for x in inst_frame0]
    n_inst, H, n = len(f0) - 1, max_heights, len(addresses)
    a = audit or AR.observe(stream, off, f0, addresses, seed_le, H)
    cap = tl_cap or 4 * H + 64
    tl = TL.timeline(stream, off, f0, addresses, seed_le, H, tl_cap=tl_cap, audit=a)
    cert_round = np.asarray(a["cert_round"]).reshape(n_inst, H)
    cert_digest = np.asarray(a["cert_digest"]).reshape(n_inst, H, 32)
    cert_frame = np.asarray(a["cert_frame"]).reshape(n_inst, H)
    out = dict(frames=np.zeros((n_inst, n, 4), np.uint32), last_height=np.zeros((n_inst, n), np.uint32),
               last_frame=np.full((n_inst, n), NONE, np.uint32), due=np.zeros((n_inst, n), np.uint32),
               proposed=np.zeros((n_inst, n), np.uint32), missed=np.zeros((n_inst, n), np.uint32),
               won=np.zeros((n_inst, n), np.uint32), inst_views=np.zeros(n_inst, np.uint32),
               inst_silent=np.zeros((n_inst, 4), np.uint64), inst_flags=np.zeros(n_inst, np.uint32))
    rep = dict(frames=0, out_of_range=0, views=0, by_outcome=[0, 0, 0], won=0, silent=0, silent_instances=0,
               partial_instances=0)
    records = []
    for i in range(n_inst):
        pps = {}                                    # (height, round, signer) -> [(frame, digest)] in frame order
        spoke = set()
        for k in range(f0[i], f0[i + 1]):
            if a["frame_status"][k] not in (AR.ST_OK, AR.ST_SEAL_FOREIGN):
                continue
            p = AR.parse(stream[off[k]:off[k + 1]])
            if not 1 <= p["code"] <= 4:
                continue
            if not 1 <= p["height"] <= H:
                rep["out_of_range"] += 1
                continue
            v, rel = int(a["frame_signer"][k]), k - f0[i]
            rep["frames"] += 1
            spoke.add(v)
            out["frames"][i, v, p["code"] - 1] += 1
            out["last_height"][i, v] = max(int(out["last_height"][i, v]), p["height"])
            out["last_frame"][i, v] = rel
            if p["code"] == 1:
                pps.setdefault((p["height"], p["round"], v), []).append((rel, p["digest"]))
        certified = lambda x: 1 <= x <= H and int(cert_round[i, x - 1]) != 0xffff
        due = {(1, 0): NONE}                        # view -> start_frame
        for x in range(2, H + 1):
            if certified(x - 1):
                due[(x, 0)] = int(cert_frame[i, x - 2])
        rcq, over = rc_quorums(stream, off, f0, a, n, H, cap, i)
        assert over == bool(tl["inst_flags"][i] & TL.KEY_OVERFLOW)
        for x in range(1, H + 1):                   # the keys recomputed here against the chronicler's reference's rows
            mine = [r for (h, r) in rcq if h == x]
            assert int(tl["rc_quorums"][i, x - 1]) == min(len(mine), 0xffff)
            if mine:
                assert int(tl["rc_max_round"][i, x - 1]) == min(max(mine), 0xfffe)
                assert int(tl["rc_max_frame"][i, x - 1]) == rcq[(x, max(mine))]
        for (x, r), fr in rcq.items():
            if r > 0:
                due[(x, r)] = fr
        out["inst_views"][i] = len(due)
        out["inst_flags"][i] = PARTIAL if over else 0
        rep["partial_instances"] += int(over)
        for (x, r) in sorted(due):
            if x == 1:
                parent = genesis
            elif certified(x - 1):
                parent = bytes(cert_digest[i, x - 2])
            else:
                parent = None
            if parent is None:
                prop, oc, ppf = NONE, UNATTRIBUTED, NONE
            else:
                prop = (AR.seed(parent, n, seed_le) + r % n) % n
                mine = pps.get((x, r, prop), [])
                out["due"][i, prop] += 1
                if not mine:
                    oc, ppf = MISSED, NONE
                    out["missed"][i, prop] += 1
                else:
                    oc, ppf = PROPOSED, mine[0][0]
                    out["proposed"][i, prop] += 1
                    if certified(x):
                        cf = int(cert_frame[i, x - 1])
                        full = AR.parse(stream[off[f0[i] + cf]:off[f0[i] + cf + 1]])["round"]
                        if full == r and any(d == bytes(cert_digest[i, x - 1]) for _, d in mine):
                            oc |= WON
                            out["won"][i, prop] += 1
                            rep["won"] += 1
            rep["by_outcome"][(oc & 0xff) - 1] += 1
            records.append((r, i, x, prop, oc, due[(x, r)], ppf))
        rep["views"] += len(due)
        silent = [v for v in range(n) if v not in spoke]
        for v in silent:
            out["inst_silent"][i, v >> 6] |= np.uint64(1 << (v & 63))
        rep["silent"] += len(silent)
        rep["silent_instances"] += bool(silent)
    return dict(out, records=np.array(records, RECORD), report=rep, audit=a, timeline=tl)


def views_of(w, i: int) -> list:
    """[(height, round, proposer, outcome, start_frame, pp_frame)] of instance i"""
    rec = w["records"] if isinstance(w, dict) else w.records
    return [tuple(int(r[k]) for k in ("height", "round", "proposer", "outcome", "start_frame", "pp_frame"))
            for r in rec[rec["inst"] == i]]


def missed_of(w, i: int) -> list:
    return [(x, r, p) for x, r, p, oc, _, _ in views_of(w, i) if oc == MISSED]


def silent_of(w, i: int) -> list:
    m = w["inst_silent"] if isinstance(w, dict) else w.inst_silent
    return [v for v in range(256) if (int(m[i, v >> 6]) >> (v & 63)) & 1]


def assert_same(got, want, rec_cap: int = None):
    """every output array, the records and the report of a roll call (a dict, or a bftsim.trace.RollCall) equal the
    reference's; rec_cap: the call kept that many records at most"""
    for k in ARRAYS:
        g = np.asarray(got[k] if isinstance(got, dict) else got.arrays[k])
        assert g.dtype == want[k].dtype, (k, g.dtype)
        assert np.array_equal(g.reshape(want[k].shape), want[k]), (k, g.reshape(want[k].shape), want[k])
    rec = got["records"] if isinstance(got, dict) else got.records
    keep = len(want["records"]) if rec_cap is None else min(rec_cap, len(want["records"]))
    assert rec.dtype == RECORD and len(rec) == keep, (rec.dtype, len(rec), keep)
    assert np.array_equal(rec, want["records"][:keep]), (rec, want["records"][:keep])
    rep = got["report"] if isinstance(got, dict) else got.report
    rep = {k: ([int(x) for x in v] if k == "by_outcome" else int(v)) for k, v in rep.items()}
    assert rep == want["report"], (rep, want["report"])
