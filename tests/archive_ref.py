"""CPU reference of the archiver (SPEC.md §11e), test infrastructure only and independent of the code under test: the
Python observer (tests/audit_ref.py) over the frames, then per certified height the header re-encoded with msgpack from
the parsed PrePrepare's block (oracle/wire_ref.py header_obj) and the seals of the Commit frames that set the
certificate's voter bits (ledger_ref.with_votes). No byte of it comes from csrc/."""
from __future__ import annotations

import msgpack
import numpy as np

import audit_ref as AR          # first: it puts oracle/ on the path
import ledger_ref as LR
import wire_ref as R

OK, NONE, NO_PROPOSAL = range(3)
NO_FRAME = 0xffffffff
ARRAYS = ("status", "pp_frame", "n_votes", "archived_height")


def slot_bytes(n: int) -> int:
    """bftsim_ledger_slot_bytes (include/bftsim.h)"""
    return (288 + 3 + n * 133 + 7) & ~7


def archive(stream: bytes, frame_off, inst_frame0, addresses, seed_le: bool, max_heights: int, key_cap: int = 0) -> dict:
    """-> dict(headers [n_inst][H] of bytes (b"" where none), the arrays of bftsim.ledger.Archive, report, audit: the
    observer's dict)"""
    stream = bytes(stream)
    off = [int(x) for x in frame_off]
    f0 = [int(x) for x in inst_frame0]
    n_inst, H = len(f0) - 1, max_heights
    obs = AR.observe(stream, off, f0, addresses, seed_le, H, key_cap)
    st, signer = obs["frame_status"], obs["frame_signer"]
    ps = {}

    def parsed(k):
        if k not in ps:
            ps[k] = AR.parse(stream[off[k]:off[k + 1]])
        return ps[k]

    status = np.full((n_inst, H), NONE, np.uint8)
    pp_frame = np.full((n_inst, H), NO_FRAME, np.uint32)
    n_votes = np.zeros((n_inst, H), np.uint16)
    height = np.zeros(n_inst, np.uint64)
    headers, votes, foreign, whole = [], 0, 0, 0
    for i in range(n_inst):
        row = [b""] * H
        accepted = [k for k in range(f0[i], f0[i + 1]) if st[k] in (AR.ST_OK, AR.ST_SEAL_FOREIGN)]
        for x in range(1, H + 1):
            if obs["cert_round"][i, x - 1] == AR.CERT_NONE:
                continue
            digest = obs["cert_digest"][i, x - 1].tobytes()
            rnd = parsed(f0[i] + int(obs["cert_frame"][i, x - 1]))["round"]        # the key's round, all 64 bits
            w = obs["cert_voters"][i, x - 1]
            voters = [v for v in range(256) if (int(w[v >> 6]) >> (v & 63)) & 1]
            pps = [k for k in accepted if st[k] == AR.ST_OK and parsed(k)["code"] == 1 and parsed(k)["height"] == x
                   and parsed(k)["digest"] == digest]
            if not pps:
                status[i, x - 1] = NO_PROPOSAL
                continue
            seals = []
            for v in voters:
                k = [k for k in accepted if signer[k] == v and parsed(k)["code"] == 3 and parsed(k)["height"] == x
                     and parsed(k)["digest"] == digest and parsed(k)["round"] == rnd][0]
                seals.append(parsed(k)["seal"])
                foreign += int(st[k] == AR.ST_SEAL_FOREIGN)
            blk = parsed(pps[0])["block"]
            row[x - 1] = LR.with_votes(msgpack.packb(R.header_obj(dict(blk, votes=None))), seals)
            status[i, x - 1], pp_frame[i, x - 1], n_votes[i, x - 1] = OK, pps[0] - f0[i], len(seals)
            votes += len(seals)
        headers.append(row)
        x = 0
        while x < H and status[i, x] == OK:
            x += 1
        height[i] = x
        whole += bool((status[i, x:] == NONE).all())
    report = dict(headers=int((status == OK).sum()), by_status=[int((status == s).sum()) for s in range(3)], votes=votes,
                  foreign_seals=foreign, archived_instances=whole)
    return dict(headers=headers, status=status, pp_frame=pp_frame, n_votes=n_votes, archived_height=height, report=report,
                audit=obs)


def assert_same(got, want):
    """got: a (ledger, bftsim.ledger.Archive) pair or the dict of tests/archive_lib.archive; want: archive()'s dict.
    Array for array, slot for slot (the bytes behind a header in its slot are zero)"""
    if isinstance(got, tuple):
        (hdr, lens, slot, H), a = got
        g = dict({k: getattr(a, k) for k in ARRAYS}, report=a.report)
    else:
        hdr, lens, slot, H, g = got["hdr"], got["hdr_len"], got["slot_bytes"], got["heights"], got
    for k in ARRAYS:
        assert np.array_equal(np.asarray(g[k]), want[k]), (k, np.asarray(g[k]).tolist(), want[k].tolist())
    assert g["report"] == want["report"], (g["report"], want["report"])
    hdr, lens = np.asarray(hdr, np.uint8).reshape(-1, slot), np.asarray(lens, np.uint32).reshape(-1)
    flat = [h for row in want["headers"] for h in row]
    assert len(flat) == len(lens) and H == want["status"].shape[1]
    for i, h in enumerate(flat):
        assert int(lens[i]) == len(h), (i, int(lens[i]), len(h))
        assert hdr[i, :len(h)].tobytes() == h, i
        assert not hdr[i, len(h):].any(), i
