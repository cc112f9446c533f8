"""The chronicler's cases that the CPU and the GPU tests share (SPEC.md §11h), each computed once per session: the
simulated traces of tests/twins_ref.py with the Python chronicler's verdict, and a hand-made stream, signed here with the
Python secp256k1 oracle, with one instance per rule of the semantics.

The simulated cases (all built on the CPU through twins_ref.reference):
    "n4"        N = 4, byz_count 1, seed 21, 6 heights, drop_ppm 100,000, instances 3..5, validator 2 forged: the lossy one
    "n4 plain"  the same without the twins
    "n7"        N = 7, byz_count 2, seed 5, 6 heights, lossless, instances 2..4, twinned
    "n7 plain"  the same without the twins"""
from __future__ import annotations

import functools

import numpy as np

import twins_ref as TW          # first: it puts oracle/ on the path
import accuse_ref as XR
import audit_ref as AR
import timeline_ref as TL
import oracle_lib as O

H = 6                           # max_heights of the hand-made stream
N, Q = 7, 4                     # its validators, and two_thirds_majority(7): a quorum is 5 distinct voters
BIG = (1 << 32) + 5
SIMULATED = (("n4", False), ("n4", True), ("n7", False), ("n7", True))
NAMES = ("four prepares", "fifth prepare", "sixth and seventh", "repeated signer", "two digests", "two rounds",
         "round change digests", "round change rounds", "round above 2^32", "heights out of range",
         "not validator, unrecoverable", "commits and preprepares", "prepared first", "prepared late", "cert unprepared",
         "prepared at another round", "locked open", "two blocks apart", "seventy keys", "empty")


def _want(cfg, stream, off, f0, heights, **kw):
    return TL.timeline(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, heights, **kw)


@functools.lru_cache(maxsize=None)
def twins(case: str, plain: bool = False):
    """twins_ref.reference(case) joined (twinned or plain) with the Python chronicler's verdict
    -> dict(ref, cfg, stream, off, meta, f0, heights, want)"""
    ref = TW.reference(case)
    stream, off, meta, f0 = TW.joined(ref, plain=plain)
    cfg = ref["cfg"]
    return dict(ref=ref, cfg=cfg, stream=stream, off=off, meta=meta, f0=f0, heights=cfg.heights,
                want=_want(cfg, stream, off, f0, cfg.heights))


@functools.lru_cache(maxsize=None)
def handmade():
    """N = 7 (the validators of twins_ref.reference("n7")), max_heights 6, one instance per name in NAMES
    -> dict(cfg, secrets, stream, off, f0, heights, index, want, want_cap2 (tl_cap 2))"""
    from bftsim.configs import BftConfig
    import trace_ref as TRC
    import wire_ref as R
    cfg, sec = TW._keyed(BftConfig(n=N, heights=H, seed=5), 7)
    dA, dB = (O.keccak256(b"timeline " + x) for x in (b"A", b"B"))
    E = bytes(32)                                                     # EMPTY_HASH, what a RoundChange carries
    # a Prepare or RoundChange is the tuple (validator, code, height, round, digest) until all are signed at once below
    P = lambda vs, h, r, d: [(v, 2, h, r, d) for v in vs]
    RC = lambda vs, h, r, d=E: [(v, 4, h, r, d) for v in vs]
    commits = lambda h, d, r=0: AR.commit_frames(sec, h, d, range(Q + 1), r)
    stranger = XR.vote_frame(O.keccak256(b"timeline stranger"), 2, 1, 0, dA)
    bad = XR.vote_frame(sec[4], 2, 1, 0, dA)
    bad = AR.reframe(bad, signature=bytes(32) + R.decode(bad)["signature"][32:])       # r = 0: never recovers
    vote = lambda v, code, h, r, d: (v, code, h, r, d)
    pps = [TRC.frame_of(m) for m in TW.reference("n7")["plain"][0][3] if m["code"] == 1][:2]
    assert len(pps) == 2
    keys70 = [(2 if k % 2 == 0 else 4, 1 + k % H, k // H) for k in range(70)]   # slots 64..69 are a lane's second
    k70 = lambda k, vs: [vote(v, keys70[k][0], keys70[k][1], keys70[k][2], dA if keys70[k][0] == 2 else E) for v in vs]
    inst = {
        "four prepares": P(range(4), 1, 0, dA),
        "fifth prepare": P(range(5), 1, 0, dA),
        "sixth and seventh": P(range(7), 1, 0, dA),
        "repeated signer": P([0, 0, 1, 2, 3, 0, 4], 1, 0, dA),
        "two digests": P(range(5), 2, 0, dA) + P(range(2, 7), 2, 0, dB),
        "two rounds": P(range(5), 1, 0, dA) + P(range(5), 1, 1, dA),
        "round change digests": RC([0], 1, 1) + RC([1], 1, 1, dA) + RC([2], 1, 1) + RC([3], 1, 1, dB) + RC([4], 1, 1),
        "round change rounds": RC(range(5), 2, 3) + RC(range(5), 2, 1) + RC([5], 2, 9) + RC(range(5), 3, 1) + RC(range(5), 3, 3),
        "round above 2^32": P([0, 1, 2], 2, BIG, dA) + P([5, 6], 2, 5, dA) + P([3, 4], 2, BIG, dA) + P([3, 4], 2, 5, dA) +
                            RC(range(5), 2, BIG) + RC(range(5), 2, BIG + 1),
        "heights out of range": P([0], 0, 0, dA) + P([1], H + 1, 0, dA) + RC([2], 0, 1) + RC([3], H + 1, 1),
        "not validator, unrecoverable": P(range(4), 1, 0, dA) + [stranger, bad],
        "commits and preprepares": pps + AR.commit_frames(sec, 1, dA, range(Q)),
        "prepared first": P(range(5), 1, 0, dA) + commits(1, dA),
        "prepared late": commits(1, dA) + P(range(5), 1, 0, dA),
        "cert unprepared": commits(1, dA) + P(range(4), 1, 0, dA) + P(range(5), 1, 0, dB) + commits(2, dB),
        "prepared at another round": P(range(5), 1, 1, dA) + commits(1, dA),
        "locked open": P(range(5), 1, 0, dA),
        "two blocks apart": P(range(4), 3, 0, dA) + P([0], 3, 0, dA) * 70 + P([4], 3, 0, dA),
        "seventy keys": [fr for k in range(70) for fr in k70(k, [3])] + k70(66, [0, 1, 2, 4]) + k70(1, [0, 1, 2, 4]) +
                        k70(69, [0, 1, 2]),
        "empty": [],
    }
    assert tuple(inst) == NAMES
    todo = sorted({fr for frames in inst.values() for fr in frames if isinstance(fr, tuple)})
    body = [dict(code=code, create_time=0, round=r, height=h, digest=d) for _, code, h, r, d in todo]
    sigs = TRC.sign_many([(sec[t[0]], O.keccak256(R.encode(b)[2])) for t, b in zip(todo, body)])
    signed = {t: R.encode(dict(b, signature=s))[0] for t, b, s in zip(todo, body, sigs)}
    inst = {name: [signed[fr] if isinstance(fr, tuple) else fr for fr in frames] for name, frames in inst.items()}
    stream, off, f0 = XR.stream_of(list(inst.values()))
    return dict(cfg=cfg, secrets=sec, stream=stream, off=off, f0=f0, heights=H, index={k: i for i, k in enumerate(NAMES)},
                want=_want(cfg, stream, off, f0, H), want_cap2=_want(cfg, stream, off, f0, H, tl_cap=2))


def rows_of(w, i) -> dict:
    """the non-empty rows of instance i as {height: (prep_round, prep_frame, prep_quorums, rc_quorums, rc_max_round,
    rc_max_frame, rc_top_round, rc_frames, flags)}"""
    out = {}
    for x in range(1, w["flags"].shape[1] + 1):
        t = tuple(int(w[k][i, x - 1]) for k in ("prep_round", "prep_frame", "prep_quorums", "rc_quorums", "rc_max_round",
                                                "rc_max_frame", "rc_top_round", "rc_frames", "flags"))
        if t != (0xffff, 0, 0, 0, 0xffff, 0, 0xffff, 0, 0):
            out[x] = t
    return out


def voters_of(w, i, x) -> list:
    return [v for v in range(256) if (int(w["prep_voters"][i, x - 1, v >> 6]) >> (v & 63)) & 1]


def check_handmade(c):
    """what each instance was built to show, on the reference's verdict"""
    w, ix = c["want"], c["index"]
    no, FIRST, UNPREP, OPEN = 0xffff, TL.PREPARED_FIRST, TL.CERT_UNPREPARED, TL.LOCKED_OPEN
    prep = lambda rnd, frame, quorums=1, flags=OPEN: (rnd, frame, quorums, 0, no, 0, no, 0, flags)
    rows = {name: rows_of(w, i) for name, i in ix.items()}
    assert rows == {
        "four prepares": {},
        "fifth prepare": {1: prep(0, 4)},
        "sixth and seventh": {1: prep(0, 4)},
        "repeated signer": {1: prep(0, 6)},
        "two digests": {2: prep(0, 4, 2)},
        "two rounds": {1: prep(0, 4, 2)},
        "round change digests": {1: (no, 0, 0, 1, 1, 4, 1, 5, 0)},
        "round change rounds": {2: (no, 0, 0, 2, 3, 4, 9, 11, 0), 3: (no, 0, 0, 2, 3, 20, 3, 10, 0)},
        "round above 2^32": {2: (0xfffe, 6, 1, 2, 0xfffe, 18, 0xfffe, 10, OPEN)},
        "heights out of range": {},
        "not validator, unrecoverable": {},
        "commits and preprepares": {},
        "prepared first": {1: prep(0, 4, flags=FIRST)},
        "prepared late": {1: prep(0, 9, flags=0)},
        "cert unprepared": {1: prep(0, 13, flags=UNPREP), 2: (no, 0, 0, 0, no, 0, no, 0, UNPREP)},
        "prepared at another round": {1: prep(1, 4, flags=0)},
        "locked open": {1: prep(0, 4)},
        "two blocks apart": {3: prep(0, 74)},
        "seventy keys": {1: (11, 73, 1, 0, no, 0, no, 0, OPEN), 2: (no, 0, 0, 1, 0, 77, 11, 16, 0),
                         4: (no, 0, 0, 0, no, 0, 11, 15, 0), 6: (no, 0, 0, 0, no, 0, 10, 11, 0)},
        "empty": {},
    }, rows
    assert voters_of(w, ix["sixth and seventh"], 1) == [0, 1, 2, 3, 4]            # frozen at the completing frame
    assert voters_of(w, ix["two digests"], 2) == [0, 1, 2, 3, 4]
    assert bytes(w["prep_digest"][ix["two digests"], 1]) == O.keccak256(b"timeline A")
    assert voters_of(w, ix["seventy keys"], 1) == [0, 1, 2, 3, 4]
    st = w["audit"]["frame_status"]
    f0 = [int(x) for x in c["f0"]]
    k = f0[ix["not validator, unrecoverable"]]
    assert st[k + 4] == AR.ST_NOT_VALIDATOR and st[k + 5] == AR.ST_UNRECOVERABLE
    assert (np.delete(st, [k + 4, k + 5]) == AR.ST_OK).all()
    k = f0[ix["commits and preprepares"]]
    assert [AR.parse(c["stream"][int(c["off"][j]):int(c["off"][j + 1])])["code"] for j in range(k, k + 6)] == [1, 1, 3, 3, 3, 3]
    cert = w["audit"]["cert_round"] != 0xffff
    assert {name: [x + 1 for x in np.nonzero(cert[i])[0]] for name, i in ix.items() if cert[i].any()} == {
        "prepared first": [1], "prepared late": [1], "cert unprepared": [1, 2], "prepared at another round": [1]}
    assert w["open_height"].tolist() == [3 if name == "cert unprepared" else 2 if cert[i].any() else 1 for name, i in ix.items()]
    assert {name for name, i in ix.items() if TL.stalled(w, i)} == {
        "fifth prepare", "sixth and seventh", "repeated signer", "two rounds", "round change digests", "locked open",
        "seventy keys"}                         # a lock or a round-change quorum at the open height, not above it
    assert not w["inst_flags"].any()
    assert w["report"] == dict(prepare_frames=199, rc_frames=78, out_of_range=4, prepared=13, rc_quorums=8, rc_heights=5,
                               prepared_first=1, cert_unprepared=2, locked_open=9, key_overflows=0), w["report"]
    # tl_cap 2: the instances with a third key overflow; what their first two keys hold stands
    c2 = c["want_cap2"]
    over = {name for name, i in ix.items() if c2["inst_flags"][i] & TL.KEY_OVERFLOW}
    assert over == {"round change rounds", "round above 2^32", "seventy keys"} and c2["report"]["key_overflows"] == 3
    for name in set(NAMES) - over:
        assert rows_of(c2, ix[name]) == rows[name], name
    assert rows_of(c2, ix["round change rounds"]) == {2: (no, 0, 0, 2, 3, 4, 3, 10, 0)}
    assert rows_of(c2, ix["round above 2^32"]) == {2: (0xfffe, 6, 1, 0, no, 0, no, 0, OPEN)}
    assert rows_of(c2, ix["seventy keys"]) == {2: (no, 0, 0, 1, 0, 77, 0, 5, 0)}
    assert c2["report"]["prepare_frames"] == 199 and c2["report"]["rc_frames"] == 78      # counted before the table
