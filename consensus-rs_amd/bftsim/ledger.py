"""The importer's verdict on a ledger (include/bftsim.h bftsim_verify_ledger, SPEC.md §11d): every Header of every
instance verified from its bytes on the device, as a syncing node's verify_header + verify_seal would
(src/consensus/backend.rs:319-367)."""
from __future__ import annotations

import numpy as np

(ST_OK, ST_ABSENT, ST_UNDECODABLE, ST_BAD_HEIGHT, ST_NO_PARENT, ST_BAD_PARENT, ST_BAD_TIME, ST_LACK_VOTES, ST_BAD_VOTE,
 ST_BAD_PROPOSER) = range(10)
STATUS_NAMES = ("OK", "ABSENT", "UNDECODABLE", "BAD_HEIGHT", "NO_PARENT", "BAD_PARENT", "BAD_TIME", "LACK_VOTES", "BAD_VOTE",
                "BAD_PROPOSER")
VOTES_SIGNATURES, VOTES_SEALS = 0, 1
VOTE_KINDS = {"signatures": VOTES_SIGNATURES, "seals": VOTES_SEALS}


def pack(ledger, slot_bytes: int = None, heights: int = None):
    """per instance a list of header byte strings (what Simulator.export_ledger returns) -> (hdr [n * H * slot] u8,
    hdr_len [n * H] u32, slot_bytes, H) in bftsim_export_ledger's layout; an empty string is an absent height"""
    n = len(ledger)
    H = max([len(row) for row in ledger] + [1]) if heights is None else heights
    longest = max([len(h) for row in ledger for h in row] + [8])
    slot = (longest + 7) & ~7 if slot_bytes is None else slot_bytes
    hdr = np.zeros(n * H * slot, np.uint8)
    lens = np.zeros(n * H, np.uint32)
    for i, row in enumerate(ledger):
        for x, h in enumerate(row[:H]):
            o = (i * H + x) * slot
            hdr[o:o + min(len(h), slot)] = np.frombuffer(bytes(h[:slot]), np.uint8)
            lens[i * H + x] = len(h)
    return hdr, lens, slot, H


class Verdict:
    """status [n, H] u8 (ST_*), block_hash [n, H, 32] u8 (zeros where absent or undecodable), voters [n, H, 4] u64
    (validators whose seal recovered), n_votes [n, H] u16, verified_height [n] u64 (the largest x with slots 1..x all
    OK); report: bftsim_ledger_report as a dict."""

    def __init__(self, arrs: dict, rep, n: int, heights: int):
        self.n, self.heights = n, heights
        self.status = arrs["status"].reshape(n, heights)
        self.block_hash = arrs["block_hash"].reshape(n, heights, 32)
        self.voters = arrs["voters"].reshape(n, heights, 4)
        self.n_votes = arrs["n_votes"].reshape(n, heights)
        self.verified_height = arrs["verified_height"]
        self.report = rep if isinstance(rep, dict) else {
            k: (list(getattr(rep, k)) if k == "by_status" else int(getattr(rep, k))) for k, _ in rep._fields_}

    def voter_list(self, i: int, x: int) -> list:
        """validator indices whose seal recovered in the header of height x (1-based) of instance i"""
        w = self.voters[i, x - 1]
        return [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]

    def names(self, i: int) -> list:
        return [STATUS_NAMES[int(s)] for s in self.status[i]]


AR_OK, AR_NONE, AR_NO_PROPOSAL = range(3)
ARCHIVE_NAMES = ("OK", "NONE", "NO_PROPOSAL")


class Archive:
    """What the archiver says of the ledger it wrote (bftsim_archive_trace, SPEC.md §11e): status [n, H] u8 (AR_*),
    pp_frame [n, H] u32 (the PrePrepare frame a header was taken from, index within its instance; 0xffffffff if none),
    n_votes [n, H] u16 (seals in the slot), archived_height [n] u64 (the largest x with slots 1..x all OK); report:
    bftsim_archive_report as a dict; audit: the observer's bftsim.trace.Audit of the same call."""

    def __init__(self, arrs: dict, rep, n: int, heights: int, audit=None):
        self.n, self.heights, self.audit = n, heights, audit
        self.status = arrs["status"].reshape(n, heights)
        self.pp_frame = arrs["pp_frame"].reshape(n, heights)
        self.n_votes = arrs["n_votes"].reshape(n, heights)
        self.archived_height = arrs["archived_height"]
        self.report = rep if isinstance(rep, dict) else {
            k: (list(getattr(rep, k)) if k == "by_status" else int(getattr(rep, k))) for k, _ in rep._fields_}

    def names(self, i: int) -> list:
        return [ARCHIVE_NAMES[int(s)] for s in self.status[i]]


def unpack(ledger):
    """(hdr, hdr_len, slot_bytes, heights) -> per instance the list of header byte strings, b"" for an absent height"""
    hdr, lens, slot, H = ledger
    hdr, lens = np.asarray(hdr, np.uint8).reshape(-1, slot), np.asarray(lens, np.uint32).reshape(-1, H)
    return [[bytes(hdr[i * H + x, :int(lens[i, x])]) for x in range(H)] for i in range(lens.shape[0])]


def compare(verdict: Verdict, result: dict, begin: int = 0) -> dict:
    """The verdict against a run's result (Simulator.run / fetch; verdict instance i = result instance begin + i). Per
    instance, over the committed heights: `ok` headers that verify, `same_hash` whose block hash is the run's;
    `verified_as_run`: verified_height equals committed_height."""
    n = verdict.n
    out = dict(ok=np.zeros(n, np.uint32), same_hash=np.zeros(n, np.uint32), verified_as_run=np.zeros(n, bool))
    for i in range(n):
        ch = min(int(result["committed_height"][begin + i]), verdict.heights)
        out["ok"][i] = int((verdict.status[i, :ch] == ST_OK).sum())
        out["same_hash"][i] = sum(np.array_equal(verdict.block_hash[i, x], result["block_hash"][begin + i, x]) for x in range(ch))
        out["verified_as_run"][i] = int(verdict.verified_height[i]) == ch
    return out
