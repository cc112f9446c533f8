"""The trace of a run (SPEC.md §11b): every consensus broadcast of the last launch as the signed wire frame a
reference node would have read from its socket (include/bftsim.h bftsim_export_trace), and the receiver's side
of it, composed from libbftwire and libbftsig."""
from __future__ import annotations

import numpy as np

MT_PREPREPARE, MT_PREPARE, MT_COMMIT, MT_ROUND_CHANGE = 1, 2, 3, 4
FLAG_FORGED, FLAG_WILD, FLAG_EQUIV, FLAG_OLD = 1, 2, 4, 8
FLAG_TWIN = 1 << 16       # the frame is a twin (Simulator.set_trace_twins, SPEC.md §11f): not a log entry's own frame


class Trace:
    """Frames of instances [begin, begin + count) of a launch, in broadcast-log order.
    stream [bytes] u8; frame_off [frames + 1] u64; meta [frames, 4] u32 (log word 0, log word 1, flags, instance
    relative to begin); inst_frame0 [count + 1] u64."""

    def __init__(self, stream, frame_off, meta, inst_frame0, begin=0):
        self.stream, self.frame_off, self.meta, self.inst_frame0, self.begin = stream, frame_off, meta, inst_frame0, begin

    def __len__(self):
        return len(self.frame_off) - 1

    tick = property(lambda self: self.meta[:, 0])
    phase = property(lambda self: self.meta[:, 1] & 0xff)
    code = property(lambda self: (self.meta[:, 1] >> 8) & 0xff)
    sender = property(lambda self: self.meta[:, 1] >> 16)
    flags = property(lambda self: self.meta[:, 2])
    instance = property(lambda self: self.meta[:, 3])
    twin = property(lambda self: (self.meta[:, 2] & FLAG_TWIN) != 0)

    def frame(self, k: int) -> bytes:
        return bytes(self.stream[int(self.frame_off[k]):int(self.frame_off[k + 1])])

    def frames(self, i: int) -> list:
        """the frames of instance begin + i"""
        return [self.frame(k) for k in range(int(self.inst_frame0[i]), int(self.inst_frame0[i + 1]))]

    def instance_stream(self, i: int) -> np.ndarray:
        """the bytes instance begin + i put on the wire (what bftwire_split_frames takes)"""
        a, b = int(self.inst_frame0[i]), int(self.inst_frame0[i + 1])
        return self.stream[int(self.frame_off[a]):int(self.frame_off[b])]


def _gather(trace: Trace, idx: np.ndarray):
    """the frames `idx` as a contiguous stream of their own -> (bytes, offsets)"""
    off = trace.frame_off.astype(np.int64)
    lens = off[idx + 1] - off[idx]
    new = np.zeros(len(idx) + 1, np.int64)
    np.cumsum(lens, out=new[1:])
    src = np.repeat(off[idx] - new[:-1], lens) + np.arange(int(new[-1]), dtype=np.int64)
    return trace.stream[src], new


def audit(trace: Trace, addresses, codec, signer, decoded: dict = None) -> np.ndarray:
    """What a receiver does with each frame (handle_message, core.rs:314-322): decode it, rebuild the sign payload
    from the decoded fields (signature None), recover the signer and look it up in the validator set.
    -> [frames] int32: the recovered validator's index in `addresses`, or -1 (not decodable, not recoverable, or
    not a validator). codec / signer: bftsim.wire.Codec / bftsim.sig.Signer of the same device. `decoded` (a dict)
    receives what the frames carried: signature [frames, 65], commit_seal [frames, 65], has_seal [frames]."""
    t = codec.torch
    out = np.full(len(trace), -1, np.int32)
    addr = np.frombuffer(b"".join(bytes(a) for a in addresses), np.uint8).reshape(-1, 20)
    rec = np.zeros((len(trace), 20), np.uint8)
    good = np.zeros(len(trace), bool)
    sig, seal, has_seal = np.zeros((len(trace), 65), np.uint8), np.zeros((len(trace), 65), np.uint8), np.zeros(len(trace), bool)
    code = trace.code
    # Subject frames: the Commits carry a seal, the others none (GossipMessage::commit_seal)
    for sel, sealed in ((code == MT_COMMIT, True), ((code == MT_PREPARE) | (code == MT_ROUND_CHANGE), False)):
        idx = np.nonzero(sel)[0]
        if len(idx) == 0:
            continue
        sb, offs = _gather(trace, idx)
        dec, ok = codec.decode(sb, offs)
        rx = {k: dec[k] for k in ("code", "round", "height", "digest", "create_time")}
        if sealed:
            rx["commit_seal"] = dec["commit_seal"]
        _, _, sd, _, ok2 = codec.encode(rx)
        _, a, ok3 = signer.recover(sd, dec["signature"], want_pub=False)
        want_seal = 1 if sealed else 0
        fine = (ok == 1) & (ok2 == 1) & (ok3 == 1) & (dec["has_sig"] == 1) & (dec["has_seal"] == want_seal)
        t.cuda.synchronize(codec.device)
        rec[idx], good[idx] = a.cpu().numpy(), fine.cpu().numpy()
        sig[idx], has_seal[idx] = dec["signature"].cpu().numpy(), dec["has_seal"].cpu().numpy() == 1
        if sealed:
            seal[idx] = dec["commit_seal"].cpu().numpy()
    idx = np.nonzero(code == MT_PREPREPARE)[0]
    if len(idx):
        from . import wire
        sb, offs = _gather(trace, idx)
        arr, ok = codec.decode_preprepare(sb, offs)
        ms = wire.array_to_preprepares(arr)
        sigs = np.stack([np.frombuffer(m["signature"] or bytes(65), np.uint8) for m in ms])
        _, _, sd, _, ok2 = codec.encode_preprepare(ms)
        _, a, ok3 = signer.recover(sd, sigs, want_pub=False)
        t.cuda.synchronize(codec.device)
        has = np.array([m["signature"] is not None for m in ms])
        rec[idx], sig[idx] = a.cpu().numpy(), sigs
        good[idx] = (ok == 1) & (ok2.cpu().numpy() == 1) & (ok3.cpu().numpy() == 1) & has
    if decoded is not None:
        decoded.update(signature=sig, commit_seal=seal, has_seal=has_seal)
    for v in range(len(addr)):
        out[good & (rec == addr[v]).all(axis=1)] = v
    return out


# ---- the observer (SPEC.md §11c): bftsim_audit_trace / bftsim_audit_last_trace
ST_OK, ST_UNDECODABLE, ST_UNRECOVERABLE, ST_NOT_VALIDATOR, ST_SEAL_BAD, ST_SEAL_FOREIGN = range(6)
AUDIT_KEY_OVERFLOW, AUDIT_CONFLICT = 1, 2
CERT_NONE = 0xffff


class Audit:
    """What the observer made of a frame stream: frame_status [frames] u8, frame_signer [frames] i32, inst_flags
    [n] u32, and per (instance, height) the commit certificate: cert_round [n, H] u16 (CERT_NONE: none), cert_digest
    [n, H, 32] u8, cert_voters [n, H, 4] u64, cert_frame [n, H] u32, cert_flags [n, H] u8 (1 proposed before
    completion, 2 rightful proposer); report: bftsim_audit_report as a dict."""

    def __init__(self, arrs: dict, rep, n: int, heights: int):
        self.n, self.heights = n, heights
        self.frame_status, self.frame_signer, self.inst_flags = arrs["frame_status"], arrs["frame_signer"], arrs["inst_flags"]
        self.cert_round = arrs["cert_round"].reshape(n, heights)
        self.cert_digest = arrs["cert_digest"].reshape(n, heights, 32)
        self.cert_voters = arrs["cert_voters"].reshape(n, heights, 4)
        self.cert_frame = arrs["cert_frame"].reshape(n, heights)
        self.cert_flags = arrs["cert_flags"].reshape(n, heights)
        self.report = {k: (list(getattr(rep, k)) if k == "by_code" else int(getattr(rep, k))) for k, _ in rep._fields_}

    def voters(self, i: int, x: int) -> list:
        """validator indices of the certificate of height x (1-based) of instance i"""
        w = self.cert_voters[i, x - 1]
        return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]

    def certificates(self, i: int) -> list:
        """[(height, round, digest, voters, proposed, rightful)] of instance i, ascending height"""
        out = []
        for x in range(1, self.heights + 1):
            r = int(self.cert_round[i, x - 1])
            if r != CERT_NONE:
                f = int(self.cert_flags[i, x - 1])
                out.append((x, r, self.cert_digest[i, x - 1].tobytes(), self.voters(i, x), bool(f & 1), bool(f & 2)))
        return out


ACCUSE_NONE = 0xffffffff
ACCUSE_VIEW_OVERFLOW = 1


class Accusation:
    """What the accuser made of a frame stream (SPEC.md §11g): records, a structured array (round, inst, height,
    signer, code, frame_a, frame_b; one per (signer, code, height, round) that carries two digests, ascending frame_b,
    the frame indices among the call's frames); frame_pair [frames] u32 (frame_a of the record a frame closes, else
    ACCUSE_NONE); inst_accused [n, 4] u64; inst_flags [n] u32; report: bftsim_accuse_report as a dict (records: all
    that were found, also when rec_cap kept fewer); audit: the observer's outputs of the same call."""

    def __init__(self, arrs: dict, rep, n: int, audit: Audit = None):
        self.n, self.audit = n, audit
        self.frame_pair, self.inst_flags = arrs["frame_pair"], arrs["inst_flags"]
        self.inst_accused = arrs["inst_accused"].reshape(n, 4)
        self.report = {k: (list(getattr(rep, k)) if k == "by_code" else int(getattr(rep, k))) for k, _ in rep._fields_}
        self.records = arrs["records"][:min(self.report["records"], len(arrs["records"]))]

    def accused(self, i: int) -> list:
        """validator indices accused in instance i, ascending"""
        w = self.inst_accused[i]
        return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]

    def proof(self, trace, k: int) -> tuple:
        """the two frames' bytes of record k, out of the trace the call ran over: (frame_a, frame_b)"""
        r = self.records[k]
        return trace.frame(int(r["frame_a"])), trace.frame(int(r["frame_b"]))


TIMELINE_KEY_OVERFLOW = 1
TIMELINE_PREPARED_FIRST, TIMELINE_CERT_UNPREPARED, TIMELINE_LOCKED_OPEN = 1, 2, 4
ROUND_NONE = 0xffff


class Timeline:
    """What the chronicler made of a frame stream (SPEC.md §11h), per (instance, height): prep_round, prep_frame,
    prep_quorums, rc_quorums, rc_max_round, rc_max_frame, rc_top_round, rc_frames, flags [n, H]; prep_digest [n, H, 32];
    prep_voters [n, H, 4]; per instance inst_flags and open_heights [n]; report: bftsim_timeline_report as a dict; audit:
    the observer's outputs of the same call. Rounds are clipped at 0xfffe, ROUND_NONE means none; frame indices are
    within the instance."""

    def __init__(self, arrs: dict, rep, n: int, heights: int, audit: Audit = None):
        self.n, self.heights, self.audit = n, heights, audit
        for k in ("prep_round", "prep_frame", "prep_quorums", "rc_quorums", "rc_max_round", "rc_max_frame", "rc_top_round",
                  "rc_frames", "flags"):
            setattr(self, k, arrs[k].reshape(n, heights))
        self.prep_digest = arrs["prep_digest"].reshape(n, heights, 32)
        self.prep_voters = arrs["prep_voters"].reshape(n, heights, 4)
        self.inst_flags, self.open_heights = arrs["inst_flags"], arrs["open_height"]
        self.report = {k: int(getattr(rep, k)) for k, _ in rep._fields_}

    def row(self, i: int, x: int) -> dict:
        """height x (from 1) of instance i: every row field, the digest as bytes, the voters as ascending indices, the
        flags by name too"""
        w = self.prep_voters[i, x - 1]
        fl = int(self.flags[i, x - 1])
        out = {k: int(getattr(self, k)[i, x - 1]) for k in ("prep_round", "prep_frame", "prep_quorums", "rc_quorums",
                                                           "rc_max_round", "rc_max_frame", "rc_top_round", "rc_frames")}
        out.update(prep_digest=self.prep_digest[i, x - 1].tobytes(), flags=fl,
                   prep_voters=[v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1],
                   prepared_first=bool(fl & TIMELINE_PREPARED_FIRST), cert_unprepared=bool(fl & TIMELINE_CERT_UNPREPARED),
                   locked_open=bool(fl & TIMELINE_LOCKED_OPEN))
        return out

    def open_height(self, i: int) -> int:
        """the smallest height of instance i without a commit certificate, heights + 1 if there is none"""
        return int(self.open_heights[i])

    def rounds_walked(self, i: int, x: int) -> int:
        """how far round changes carried height x: the greatest round with a round-change quorum (clipped), 0 without"""
        r = int(self.rc_max_round[i, x - 1])
        return 0 if r == ROUND_NONE else r

    def stalled(self, i: int) -> bool:
        """the instance stopped at its open height with a lock standing or after a round-change quorum there"""
        x = self.open_height(i)
        if x > self.heights:
            return False
        return bool(int(self.flags[i, x - 1]) & TIMELINE_LOCKED_OPEN) or int(self.rc_quorums[i, x - 1]) > 0


ROLLCALL_PROPOSED, ROLLCALL_MISSED, ROLLCALL_UNATTRIBUTED, ROLLCALL_WON = 1, 2, 3, 0x100
ROLLCALL_PARTIAL = 1
ROLLCALL_NONE = 0xffffffff


class RollCall:
    """What the roll call made of a frame stream (SPEC.md §11i). Per (instance, validator): frames [n, N, 4] (the counting
    frames it signed, by code 1..4), last_height, last_frame, due, proposed, won [n, N] (these, and the missed counts
    beside the method missed(i), also in the dict `arrays`); per instance inst_views,
    inst_flags [n] and inst_silent [n, 4]; records, a structured array (round, inst, height, proposer, outcome,
    start_frame, pp_frame), one per due view, instance-major and by (height, round) within an instance; report:
    bftsim_rollcall_report as a dict (views: all that were found, also when rec_cap kept fewer); audit and timeline: the
    observer's and the chronicler's outputs of the same call. Frame indices are within the instance."""

    def __init__(self, arrs: dict, rep, n: int, validators: int, audit: Audit = None, timeline: Timeline = None):
        self.n, self.validators, self.audit, self.timeline = n, validators, audit, timeline
        self.arrays = {k: arrs[k].reshape(n, validators) for k in ("last_height", "last_frame", "due", "proposed", "missed", "won")}
        self.arrays.update(frames=arrs["frames"].reshape(n, validators, 4), inst_views=arrs["inst_views"],
                           inst_silent=arrs["inst_silent"].reshape(n, 4), inst_flags=arrs["inst_flags"])
        for k, a in self.arrays.items():
            if k != "missed":                      # missed(i) is the method; the counts are arrays["missed"]
                setattr(self, k, a)
        self.report = {k: (list(getattr(rep, k)) if k == "by_outcome" else int(getattr(rep, k))) for k, _ in rep._fields_}
        self.records = arrs["records"][:min(self.report["views"], len(arrs["records"]))]

    def row(self, i: int, v: int) -> dict:
        """validator v of instance i: every row field, frames as the list by code"""
        out = {k: int(self.arrays[k][i, v]) for k in ("last_height", "last_frame", "due", "proposed", "missed", "won")}
        out["frames"] = [int(x) for x in self.frames[i, v]]
        return out

    def views(self, i: int):
        """the records of instance i among those the call returned, by (height, round) ascending"""
        return self.records[self.records["inst"] == i]

    def missed(self, i: int) -> list:
        """[(height, round, proposer)] of the views of instance i whose proposer sent no PrePrepare"""
        return [(int(r["height"]), int(r["round"]), int(r["proposer"])) for r in self.views(i)
                if int(r["outcome"]) == ROLLCALL_MISSED]

    def silent(self, i: int) -> list:
        """validator indices without a counting frame in instance i, ascending"""
        w = self.inst_silent[i]
        return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]


def compare(audit: Audit, result: dict, begin: int = 0) -> dict:
    """The certificates against a run's result (Simulator.run / fetch; audit instance i = result instance begin + i).
    Per instance, over the committed heights: `certified` with a certificate for the committed hash, `missing`
    without one, `different` with one for another hash; `same_round` of the certified ones at the run's own round."""
    n = audit.n
    out = {k: np.zeros(n, np.uint32) for k in ("certified", "missing", "different", "same_round")}
    for i in range(n):
        ch = min(int(result["committed_height"][begin + i]), audit.heights)
        for x in range(ch):
            r = int(audit.cert_round[i, x])
            if r == CERT_NONE:
                out["missing"][i] += 1
            elif np.array_equal(audit.cert_digest[i, x], result["block_hash"][begin + i, x]):
                out["certified"][i] += 1
                out["same_round"][i] += r == int(result["round"][begin + i, x])
            else:
                out["different"][i] += 1
    return out
