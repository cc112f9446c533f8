"""The frame streams the CPU and the GPU tests of the archiver (SPEC.md §11e) share, each built once per session: the
reference traces of tests/trace_ref.py, hostile variants of them (audit_ref.splice / reframe / appended /
commit_frames), and one-height streams with 67 of 100 and 171 of 256 voters signed here with ledger_ref's cached keys.
Each case comes with the Python archiver's verdict on it (tests/archive_ref.py)."""
from __future__ import annotations

import functools

import numpy as np

import trace_ref as TR          # first: it puts oracle/ on the path
import archive_ref as ARC
import audit_ref as AR
import ledger_ref as LR
import oracle_lib as O
import secp256k1_ref as S
import sig_lib
import wire_ref as R

NAMES = ("cfg1", "n4", "no proposal", "late proposal", "conflict", "foreign seal", "key_cap 4", "truncated instance",
         "n100_67", "n256_171")


def _frames(stream, off):
    off = [int(x) for x in off]
    return [stream[off[k]:off[k + 1]] for k in range(len(off) - 1)]


def _joined(frames):
    return AR.appended(b"", np.zeros(1, np.uint64), frames)


def _wide(case: str):
    """one instance, height 1: a PrePrepare of the reference ledger's block by validator 0 and a Commit of each of its
    voters; every frame signed with the host build of the library's signer, as ledger_ref seals its headers"""
    ref = LR.reference(case)
    cfg, sec = ref["cfg"], ref["secrets"]
    blk = dict(LR.decode(ref["nil"][0][0]), txs=[])
    bh = bytes(ref["res"]["block_hash"][0, 0])
    m = dict(round=0, height=1, create_time=0, block=blk)
    m["signature"] = sig_lib.sign(sec[0], O.keccak256(R.preprepare_frame(m)[1]))
    frames = [R.preprepare_frame(m)[0]]
    for v in ref["voters"]:
        d = dict(code=3, create_time=0, round=0, height=1, digest=bh, commit_seal=LR.seal(sec[v], bh))
        d["signature"] = sig_lib.sign(sec[v], O.keccak256(R.encode(d)[2]))
        frames.append(R.encode(d)[0])
    return ref, frames


@functools.lru_cache(maxsize=None)
def case(name: str) -> dict:
    """-> dict(cfg, stream, off, f0, heights, key_cap, want: archive_ref.archive's dict, plus what the case knows)"""
    key_cap, extra = 0, {}
    if name in ("n100_67", "n256_171"):
        ref, frames = _wide(name)
        cfg, heights = ref["cfg"], 1
        stream, off, f0 = _joined(frames)
        extra = dict(header=ref["ledger"][0][0], voters=ref["voters"])
    elif name in ("n4", "key_cap 4"):
        ref = TR.reference("n4")
        cfg, heights = ref["cfg"], ref["cfg"].heights
        stream, off, _, f0 = TR.joined(ref)
        key_cap = 4 if name == "key_cap 4" else 0
        extra = dict(ref=ref)
    else:
        ref = TR.reference("cfg1")
        cfg, heights = ref["cfg"], ref["cfg"].heights
        stream, off, _, f0 = TR.joined(ref)
        ms = ref["inst"][0][3]
        frames = _frames(stream, off)
        extra = dict(ref=ref)
        pp3 = [k for k, m in enumerate(ms) if m["code"] == 1 and m["height"] == 3 and
               m["digest"] == bytes(ref["res"]["block_hash"][0, 2])]
        if name == "no proposal":                      # every PrePrepare of height 3's committed block, emptied
            for k in pp3:
                frames[k] = b""
            stream, off, f0 = _joined(frames)
            extra["removed"] = pp3
        elif name == "late proposal":                  # ... moved behind the last frame: after the completing Commit
            moved = [frames[k] for k in pp3]
            frames = [f for k, f in enumerate(frames) if k not in pp3] + moved
            stream, off, f0 = _joined(frames)
            extra["pp_frame"] = len(frames) - len(moved)
        elif name == "conflict":                       # a second quorum at height 2, for another digest
            other = AR.commit_frames(ref["secrets"], 2, O.keccak256(b"another block at height 2"), range(4))
            stream, off, f0 = AR.appended(stream, off, other)
        elif name == "foreign seal":                   # validator 1's Commit of height 2 carrying validator 0's seal
            cm = [k for k, m in enumerate(ms) if m["code"] == 3 and m["height"] == 2]
            k1 = [k for k in cm if (ms[k]["meta"][1] >> 16) == 1][0]
            k0 = [k for k in cm if (ms[k]["meta"][1] >> 16) == 0 and ms[k]["digest"] == ms[k1]["digest"]][0]
            d = R.decode(frames[k1])
            d["commit_seal"] = ms[k0]["seal"]
            d["signature"] = S.sign(ms[k1]["key"], O.keccak256(R.encode(d)[2]))
            stream, off = AR.splice(stream, off, k1, R.encode(d)[0])
            extra.update(frame=k1, seal=ms[k0]["seal"])
        elif name == "truncated instance":             # a second instance: one frame of each kind cut at every length
            ks = [[j for j, m in enumerate(ms) if m["code"] == code][0] for code in (1, 2, 3, 4)]
            stream, off, f0 = AR.appended(stream, off, AR.truncations(stream, off, ks), new_instance=True)
        elif name != "cfg1":
            raise KeyError(name)
    want = ARC.archive(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, heights, key_cap)
    return dict(extra, name=name, cfg=cfg, stream=stream, off=np.asarray(off, np.uint64), f0=np.asarray(f0, np.uint64),
                heights=heights, key_cap=key_cap, want=want)


def ledger_of(want: dict, n: int):
    """the reference's headers packed in bftsim_export_ledger's layout -> (hdr, hdr_len, slot_bytes, heights)"""
    from bftsim.ledger import pack
    return pack(want["headers"], slot_bytes=ARC.slot_bytes(n), heights=want["status"].shape[1])


def check_expectations(c: dict, got_status, verdict):
    """what each case must show, on the archiver's statuses (got_status: [n, H]) and the importer's verdict on its
    ledger (verdict: ledger_ref.verify's dict, or a bftsim.ledger.Verdict); shared by the CPU and the GPU tests"""
    name, want = c["name"], c["want"]
    vs = verdict["status"] if isinstance(verdict, dict) else verdict.status
    vh = verdict["verified_height"] if isinstance(verdict, dict) else verdict.verified_height
    bh = verdict["block_hash"] if isinstance(verdict, dict) else verdict.block_hash
    if name == "cfg1":
        assert (got_status == ARC.OK).all() and (want["n_votes"] == 4).all() and want["report"]["headers"] == 6
        assert (vs == LR.OK).all() and int(vh[0]) == 6 and np.array_equal(bh[0], c["ref"]["res"]["block_hash"][0])
    elif name == "n4":
        res = c["ref"]["res"]
        assert want["report"]["headers"] == int(res["committed_height"].sum()) == 15
        assert (vs[got_status == ARC.OK] == LR.OK).all() and np.array_equal(vh, res["committed_height"].astype(np.uint64))
        obs = want["audit"]
        forged = obs["frame_status"] == AR.ST_NOT_VALIDATOR
        f0 = [int(x) for x in c["f0"]]
        for i in range(3):
            for x in range(6):
                if got_status[i, x] == ARC.OK:
                    assert not forged[f0[i] + int(want["pp_frame"][i, x])]
        assert forged.any() and not (want["audit"]["cert_voters"][:, :, 0] & np.uint64(4)).any()     # validator 2 never votes
    elif name == "no proposal":
        assert got_status[0].tolist() == [ARC.OK, ARC.OK, ARC.NO_PROPOSAL, ARC.OK, ARC.OK, ARC.OK]
        assert int(want["archived_height"][0]) == 2 and want["report"]["archived_instances"] == 0
        assert vs[0].tolist() == [LR.OK, LR.OK, LR.ABSENT, LR.NO_PARENT, LR.OK, LR.OK]
    elif name == "late proposal":
        assert (got_status == ARC.OK).all() and int(want["pp_frame"][0, 2]) == c["pp_frame"]
        assert int(want["pp_frame"][0, 2]) > int(want["audit"]["cert_frame"][0, 2]) and want["audit"]["cert_flags"][0, 2] == 0
        assert (vs == LR.OK).all()
    elif name == "conflict":
        assert want["audit"]["inst_flags"][0] == AR.CONFLICT and (got_status == ARC.OK).all()
        assert (vs == LR.OK).all() and np.array_equal(bh[0], c["ref"]["res"]["block_hash"][0])
    elif name == "foreign seal":
        assert want["audit"]["frame_status"][c["frame"]] == AR.ST_SEAL_FOREIGN and want["report"]["foreign_seals"] == 1
        assert (got_status == ARC.OK).all()
        votes = LR.decode(want["headers"][0][1])["votes"]
        assert votes[0] == votes[1] == c["seal"]                                  # written as received
        assert vs[0, 1] == LR.LACK_VOTES and int(vh[0]) == 1                      # 3 distinct voters of 5: Q = 3
    elif name == "key_cap 4":
        assert (want["audit"]["inst_flags"] & 1).all() and 0 < want["report"]["headers"] < 15
    elif name == "truncated instance":
        assert (got_status[0] == ARC.OK).all() and (got_status[1] == ARC.NONE).all()
        assert want["report"]["archived_instances"] == 2 and want["archived_height"].tolist() == [6, 0]
    else:
        nv = len(c["voters"])
        assert want["headers"][0][0] == c["header"] and int(want["n_votes"][0, 0]) == nv and nv in (67, 171)
        assert vs[0, 0] == LR.OK
