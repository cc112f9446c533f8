"""The roll call's cases that the CPU and the GPU tests share (SPEC.md §11i), each computed once per session: the
simulated traces of tests/twins_ref.py and tests/trace_ref.py with the Python roll call's verdict, a proposer-crash run
built on the CPU, and two hand-made streams, signed here with the Python secp256k1 oracle, with one instance per rule.

The simulated cases:
    ("n4", plain) / ("n7", plain)   twins_ref.reference, twinned or plain
    "cfg1"                          trace_ref.reference("cfg1"): N = 5, c5 (validator 4) silent
    "crash"                         N = 7, 6 heights, seed CRASH_SEED, proposer_crash_ppm 300,000, lossless, byz_count 0,
                                    instances 0..3"""
from __future__ import annotations

import ctypes
import functools

import msgpack
import numpy as np

import twins_ref as TW          # first: it puts oracle/ on the path
import accuse_ref as XR
import audit_ref as AR
import rollcall_ref as RR
import trace_ref as TRC
import oracle_lib as O
import wire_ref as R

H = 6                           # max_heights of the hand-made streams
N, Q = 7, 4                     # the first one's validators, and two_thirds_majority(7): a quorum is 5 distinct voters
BIG = (1 << 32) + 5
CRASH_SEED = 9                  # the first seed from 9 upward whose run meets the premises (test_rollcall_cpu.py)
CRASH_PPM = 300_000
SIMULATED = (("n4", False), ("n4", True), ("n7", False), ("n7", True))
NAMES = ("genesis proposed", "genesis missed", "wrong signer", "round 0 after certificate", "round 2 not round 1",
         "four round changes", "round change of round 0", "round above 2^32", "unattributed", "certificate at another round",
         "certificate for another digest", "twin preprepares", "preprepare before start", "not validator, unrecoverable",
         "heights out of range", "seventy views", "empty")


def _want(cfg, stream, off, f0, heights, **kw):
    return RR.rollcall(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, TRC.genesis_hash(cfg), heights, **kw)


def _case(cfg, stream, off, f0, heights, **extra):
    return dict(cfg=cfg, stream=stream, off=off, f0=f0, heights=heights, genesis=TRC.genesis_hash(cfg),
                want=_want(cfg, stream, off, f0, heights), **extra)


@functools.lru_cache(maxsize=None)
def twins(case: str, plain: bool = False):
    ref = TW.reference(case)
    stream, off, _, f0 = TW.joined(ref, plain=plain)
    return _case(ref["cfg"], stream, off, f0, ref["cfg"].heights, ref=ref)


@functools.lru_cache(maxsize=None)
def cfg1():
    ref = TRC.reference("cfg1")
    stream, off, _, f0 = TRC.joined(ref)
    return _case(ref["cfg"], stream, off, f0, ref["cfg"].heights, ref=ref)


def crash_config(n: int = 7, heights: int = 6, seed: int = CRASH_SEED):
    from bftsim.configs import BftConfig
    return BftConfig(n=n, heights=heights, seed=seed, proposer_crash_ppm=CRASH_PPM)


@functools.lru_cache(maxsize=None)
def crash(seed: int = CRASH_SEED):
    cfg, secrets = TW._keyed(crash_config(seed=seed), 7)
    first, n = 0, 4
    res = O.run_crypto(cfg, first, n)
    ref = dict(cfg=cfg, secrets=secrets, first=first, n=n, forged=(), res=res,
               inst=[TRC.instance_trace(cfg, first, res, i, secrets, (), rel=i) for i in range(n)])
    stream, off, _, f0 = TRC.joined(ref)
    return _case(cfg, stream, off, f0, cfg.heights, ref=ref)


def crashed(cfg, inst: int, height: int, round_: int) -> bool:
    """SPEC.md §5, domain CRASH: the proposer of view (height, round) of the instance does not send its PrePrepare"""
    ctr = (ctypes.c_uint32 * 4)(inst, height, round_ & 0xffffffff, 3)
    key = (ctypes.c_uint32 * 2)(cfg.seed & 0xffffffff, cfg.seed >> 32)
    out = (ctypes.c_uint32 * 4)()
    O.lib().orc_philox4x32_10(ctr, key, out)
    return out[0] < (cfg.proposer_crash_ppm << 32) // 1_000_000


def check_against_run(got, cfg, res, first: int):
    """the closure against the run (lossless, byz_count 0): the MISSED views are exactly the started views whose
    CRASH draw fell (or whose proposer is silent), and every committed height has one WON view, the run's"""
    n_inst = len(res["committed_height"])
    for i in range(n_inst):
        views = RR.views_of(got, i)
        for x, r, p, oc, _, _ in views:
            assert oc != RR.UNATTRIBUTED, (i, x, r)
            down = crashed(cfg, first + i, x, r) or p in cfg.silent
            assert (oc == RR.MISSED) == down, (i, x, r, p, oc, down)
        for x in range(1, int(res["committed_height"][i]) + 1):
            won = [(r, p) for y, r, p, oc, _, _ in views if y == x and oc & RR.WON]
            assert won == [(int(res["round"][i, x - 1]), int(res["proposer"][i, x - 1]))], (i, x, won)


def _pp_digest(blk) -> bytes:
    return O.keccak256(msgpack.packb(R.header_obj(dict(blk, votes=None))))


def _sign_all(inst, sec, block):
    """the instances' frames: tuples (validator, code 2 | 4, height, round, digest) and ("pp", key, height, round, tag)
    are signed here at once (key: a validator index or a secret), bytes pass through"""
    blk_of = lambda h, tag: dict(block, height=h, tx_hash=O.keccak256(b"rollcall " + tag))
    todo = sorted({fr for frames in inst.values() for fr in frames if isinstance(fr, tuple)}, key=repr)
    body, keys = [], []
    for t in todo:
        if t[0] == "pp":
            m = dict(round=t[3], height=t[2], block=blk_of(t[2], t[4]), create_time=0)
            body.append(m)
            keys.append((sec[t[1]] if isinstance(t[1], int) else t[1], O.keccak256(R.preprepare_frame(m)[1])))
        else:
            b = dict(code=t[1], create_time=0, round=t[3], height=t[2], digest=t[4])
            body.append(b)
            keys.append((sec[t[0]], O.keccak256(R.encode(b)[2])))
    sigs = TRC.sign_many(keys)
    signed = {t: (R.preprepare_frame(dict(b, signature=s))[0] if t[0] == "pp" else R.encode(dict(b, signature=s))[0])
              for t, b, s in zip(todo, body, sigs)}
    return {name: [signed[fr] if isinstance(fr, tuple) else fr for fr in frames] for name, frames in inst.items()}


def _block():
    pp = [TRC.frame_of(m) for m in TW.reference("n7")["plain"][0][3] if m["code"] == 1][0]
    return AR.parse(pp)["block"]


@functools.lru_cache(maxsize=None)
def handmade():
    """N = 7 (the validators of twins_ref.reference("n7")), max_heights 6, one instance per name in NAMES
    -> dict(cfg, stream, off, f0, heights, genesis, index, prop, want, want_cap2 (tl_cap 2))"""
    from bftsim.configs import BftConfig
    cfg, sec = TW._keyed(BftConfig(n=N, heights=H, seed=5), 7)
    genesis, le = TRC.genesis_hash(cfg), cfg.seed_byte_order == 1
    block = _block()
    dig = lambda h, tag: _pp_digest(dict(block, height=h, tx_hash=O.keccak256(b"rollcall " + tag)))
    dA, dB = dig(1, b"A"), dig(1, b"B")
    g = lambda r: (AR.seed(genesis, N, le) + r % N) % N              # the proposer of (1, r)
    p2 = (AR.seed(dA, N, le)) % N                                    # of (2, 0) above a certificate for dA
    E = bytes(32)
    P = lambda vs, h, r, d: [(v, 2, h, r, d) for v in vs]
    RC = lambda vs, h, r: [(v, 4, h, r, E) for v in vs]
    PP = lambda v, h, r, tag: [("pp", v, h, r, tag)]
    commits = lambda h, d, r=0: AR.commit_frames(sec, h, d, range(Q + 1), r)
    bad = R.preprepare_frame(dict(round=0, height=1, block=dict(block, height=1, tx_hash=O.keccak256(b"rollcall A")),
                                  create_time=0, signature=bytes(32) + bytes([1] * 32) + b"\x00"))[0]      # r = 0: never recovers
    inst = {
        "genesis proposed": PP(g(0), 1, 0, b"A"),
        "genesis missed": P([0], 1, 0, dA),
        "wrong signer": PP((g(0) + 1) % N, 1, 0, b"A"),
        "round 0 after certificate": PP(g(0), 1, 0, b"A") + commits(1, dA),
        "round 2 not round 1": RC(range(5), 1, 2) + RC(range(4), 1, 1),
        "four round changes": RC(range(4), 1, 1),
        "round change of round 0": RC(range(5), 1, 0),
        "round above 2^32": RC(range(5), 1, BIG) + PP(g(BIG), 1, BIG, b"A"),
        "unattributed": RC(range(5), 3, 1),
        "certificate at another round": PP(g(0), 1, 0, b"A") + commits(1, dA, 1),
        "certificate for another digest": PP(g(0), 1, 0, b"A") + commits(1, dB),
        "twin preprepares": PP(g(0), 1, 0, b"B") + PP(g(0), 1, 0, b"A") + commits(1, dA),
        "preprepare before start": PP(p2, 2, 0, b"C") + PP(g(0), 1, 0, b"A") + commits(1, dA),
        "not validator, unrecoverable": PP(O.keccak256(b"rollcall stranger"), 1, 0, b"A") + [bad],
        "heights out of range": P([0], 0, 0, dA) + P([1], H + 1, 0, dA) + PP(g(0), H + 1, 0, b"A"),
        "seventy views": [fr for r in range(1, 70) for fr in RC(range(5), 1, r)] + PP(g(66), 1, 66, b"A"),
        "empty": [],
    }
    assert tuple(inst) == NAMES
    stream, off, f0 = XR.stream_of(list(_sign_all(inst, sec, block).values()))
    return dict(_case(cfg, stream, off, f0, H), index={k: i for i, k in enumerate(NAMES)}, prop=dict(g=g, p2=p2),
                want_cap2=_want(cfg, stream, off, f0, H, tl_cap=2))


@functools.lru_cache(maxsize=None)
def hundred():
    """N = 100, one instance: a RoundChange quorum (67 voters) at the round whose proposer is validator 80, who never
    speaks; the validators 67..99 but 70 and 80 send one Prepare each, so 70 and 80 are silent: bitmap word 1, and the
    rows past lane 63"""
    from bftsim.configs import BftConfig
    n = 100
    cfg, sec = TW._keyed(BftConfig(n=n, heights=2, seed=5), 7)
    genesis, le = TRC.genesis_hash(cfg), cfg.seed_byte_order == 1
    r = (80 - AR.seed(genesis, n, le)) % n or n                      # above 0, its proposer 80
    frames = [(v, 4, 1, r, bytes(32)) for v in range(67)] + \
        [(v, 2, 1, 0, O.keccak256(b"rollcall hundred")) for v in range(67, n) if v not in (70, 80)]
    stream, off, f0 = XR.stream_of(list(_sign_all({"hundred": frames}, sec, None).values()))
    return dict(_case(cfg, stream, off, f0, 2), round=r)


def stream_cases():
    """every stream case by name -> the case dict (all computed on first use, shared by the session)"""
    out = {f"{c}{' plain' if p else ''}": (lambda c=c, p=p: twins(c, p)) for c, p in SIMULATED}
    out.update(cfg1=cfg1, crash=crash, handmade=handmade, hundred=hundred)
    return out


def check_handmade(c):
    """what each instance was built to show, on the reference's verdict"""
    w, ix, no = c["want"], c["index"], RR.NONE
    g, p2 = c["prop"]["g"], c["prop"]["p2"]
    PR, MI, UN, WON = RR.PROPOSED, RR.MISSED, RR.UNATTRIBUTED, RR.WON
    views = {name: RR.views_of(w, i) for name, i in ix.items()}      # (height, round, proposer, outcome, start, pp)
    assert views == {
        "genesis proposed": [(1, 0, g(0), PR, no, 0)],
        "genesis missed": [(1, 0, g(0), MI, no, no)],
        "wrong signer": [(1, 0, g(0), MI, no, no)],
        "round 0 after certificate": [(1, 0, g(0), PR | WON, no, 0), (2, 0, p2, MI, 5, no)],
        "round 2 not round 1": [(1, 0, g(0), MI, no, no), (1, 2, g(2), MI, 4, no)],
        "four round changes": [(1, 0, g(0), MI, no, no)],
        "round change of round 0": [(1, 0, g(0), MI, no, no)],
        "round above 2^32": [(1, 0, g(0), MI, no, no), (1, BIG, g(BIG), PR, 4, 5)],
        "unattributed": [(1, 0, g(0), MI, no, no), (3, 1, no, UN, 4, no)],
        "certificate at another round": [(1, 0, g(0), PR, no, 0), (2, 0, p2, MI, 5, no)],
        "certificate for another digest": [(1, 0, g(0), PR, no, 0), (2, 0, AR.seed(_dB(c), N, c["cfg"].seed_byte_order == 1) % N, MI, 5, no)],
        "twin preprepares": [(1, 0, g(0), PR | WON, no, 0), (2, 0, p2, MI, 6, no)],
        "preprepare before start": [(1, 0, g(0), PR | WON, no, 1), (2, 0, p2, PR, 6, 0)],
        "not validator, unrecoverable": [(1, 0, g(0), MI, no, no)],
        "heights out of range": [(1, 0, g(0), MI, no, no)],
        "seventy views": [(1, 0, g(0), MI, no, no)] + [(1, r, g(r), PR if r == 66 else MI, 5 * r - 1, 345 if r == 66 else no)
                                                        for r in range(1, 70)],
        "empty": [(1, 0, g(0), MI, no, no)],
    }, views
    st = w["audit"]["frame_status"]
    k = int(c["f0"][ix["not validator, unrecoverable"]])
    assert st[k] == AR.ST_NOT_VALIDATOR and st[k + 1] == AR.ST_UNRECOVERABLE
    assert (np.delete(st, [k, k + 1]) == AR.ST_OK).all()
    # rows: the proposer of "genesis proposed" signed one PrePrepare at frame 0; the others are silent
    i = ix["genesis proposed"]
    assert w["frames"][i, g(0)].tolist() == [1, 0, 0, 0] and int(w["last_height"][i, g(0)]) == 1
    assert int(w["last_frame"][i, g(0)]) == 0 and int(w["due"][i, g(0)]) == 1 and int(w["proposed"][i, g(0)]) == 1
    assert RR.silent_of(w, i) == [v for v in range(N) if v != g(0)]
    i = ix["round 0 after certificate"]
    assert int(w["won"][i, g(0)]) == 1 and int(w["missed"][i, p2]) == 1
    assert w["frames"][i].sum(axis=0).tolist() == [1, 0, 5, 0] and RR.silent_of(w, i) == [v for v in (5, 6) if v != g(0)]
    i = ix["heights out of range"]
    assert RR.silent_of(w, i) == list(range(N)) and not w["frames"][i].any()
    assert RR.silent_of(w, ix["empty"]) == list(range(N)) and (w["last_frame"][ix["empty"]] == no).all()
    i = ix["seventy views"]
    assert int(w["inst_views"][i]) == 70 and int(w["due"][i].sum()) == 70 and int(w["last_frame"][i, 4]) == (345 if g(66) == 4 else 344)
    assert not w["inst_flags"].any()
    rep = w["report"]
    assert rep["out_of_range"] == 3 and rep["views"] == int(w["inst_views"].sum()) == len(w["records"]) == 94
    assert rep["by_outcome"] == [9, 84, 1] and rep["won"] == 3 and rep["partial_instances"] == 0
    assert rep["silent_instances"] == len(NAMES)
    # tl_cap 2: only the seventy views overflow; what the first two keys hold stands
    c2 = c["want_cap2"]
    assert [name for name, i in ix.items() if c2["inst_flags"][i] & RR.PARTIAL] == ["seventy views"]
    assert RR.views_of(c2, ix["seventy views"]) == views["seventy views"][:3]
    for name in set(NAMES) - {"seventy views"}:
        assert RR.views_of(c2, ix[name]) == views[name], name
    assert c2["report"]["partial_instances"] == 1 and c2["report"]["frames"] == rep["frames"]


def _dB(c) -> bytes:
    """the digest of the hand-made block B"""
    return _pp_digest(dict(_block(), height=1, tx_hash=O.keccak256(b"rollcall B")))
