"""The accuser's cases that the CPU and the GPU tests share (SPEC.md §11g), each computed once per session: the pinned
twins references with the Python accuser's verdict, and a hand-made stream, signed here with the Python secp256k1
oracle, with one instance per rule of the semantics."""
from __future__ import annotations

import ctypes
import functools

import numpy as np

import twins_ref as TW          # first: it puts oracle/ on the path
import accuse_ref as XR
import oracle_lib as O

H = 6                           # max_heights of the hand-made stream
NAMES = ("three digests", "duplicate", "first frame unrecoverable", "other round, other code", "round above 2^32",
         "heights out of range", "round changes", "foreign seal", "two chunks apart", "empty", "seventy views")


def seeded_byz(cfg, inst) -> set:
    """the oracle's draw of an instance's Byzantine validators (SPEC.md §5)"""
    c, keep = O.to_orc(cfg)
    out = (ctypes.c_uint64 * 4)()
    O.lib().orc_byz_mask(ctypes.byref(c), ctypes.c_uint32(inst), out)
    del keep
    return {v for v in range(cfg.n) if (out[v >> 6] >> (v & 63)) & 1}


def _want(cfg, stream, off, f0, heights, **kw):
    return XR.accuse(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, heights, **kw)


@functools.lru_cache(maxsize=None)
def twins(case: str, plain: bool = False):
    """twins_ref.reference(case) joined (twinned or plain) with the Python accuser's verdict
    -> dict(ref, cfg, stream, off, meta, f0, heights, want)"""
    ref = TW.reference(case)
    stream, off, meta, f0 = TW.joined(ref, plain=plain)
    cfg = ref["cfg"]
    return dict(ref=ref, cfg=cfg, stream=stream, off=off, meta=meta, f0=f0, heights=cfg.heights,
                want=_want(cfg, stream, off, f0, cfg.heights))


@functools.lru_cache(maxsize=None)
def handmade():
    """N = 4, max_heights 6, one instance per name in NAMES -> dict(cfg, secrets, stream, off, f0, heights, index, want,
    want_cap2 (view_cap 2), want_rec1 (rec_cap 1))"""
    from bftsim.configs import BftConfig
    cfg, sec = TW._keyed(BftConfig(n=4, heights=H, seed=21), 7)
    dA, dB, dC = (O.keccak256(b"accuse " + x) for x in (b"A", b"B", b"C"))
    f = lambda v, code, h, r, d, **kw: XR.vote_frame(sec[v], code, h, r, d, **kw)
    import audit_ref as AR
    import wire_ref as R
    bad = f(0, 2, 1, 0, dA)
    bad = AR.reframe(bad, signature=bytes(32) + R.decode(bad)["signature"][32:])       # r = 0: never recovers
    big = (1 << 32) + 5
    filler = f(1, 2, 1, 0, dA)
    views = [(1 + k % H, k // H) for k in range(70)]              # 70 (height, round) pairs: slots 64..69 are a lane's second
    inst = {
        "three digests": [f(0, 2, 1, 0, dA), f(0, 2, 1, 0, dB), f(0, 2, 1, 0, dC), f(0, 2, 1, 0, dA)],
        "duplicate": [f(0, 2, 1, 0, dA)] * 2 + [f(1, 3, 1, 0, dA)] * 2,
        "first frame unrecoverable": [bad, f(0, 2, 1, 0, dB), f(0, 2, 1, 0, dC)],
        "other round, other code": [f(0, 2, 1, 0, dA), f(0, 2, 1, 1, dB), f(0, 3, 1, 0, dB), f(0, 2, 2, 0, dB), f(1, 2, 1, 0, dB)],
        "round above 2^32": [f(1, 2, 2, big, dA), f(1, 2, 2, 5, dB), f(1, 2, 2, big, dB)],
        "heights out of range": [f(0, 2, 0, 0, dA), f(0, 2, 0, 0, dB), f(0, 2, H + 1, 0, dA), f(0, 2, H + 1, 0, dB)],
        "round changes": [f(0, 4, 1, 1, dA), f(0, 4, 1, 1, dB)],
        "foreign seal": [f(0, 3, 1, 0, dA), f(0, 3, 1, 0, dB, seal_secret=sec[1])],
        "two chunks apart": [f(2, 2, 3, 0, dA)] + [filler] * 70 + [f(2, 2, 3, 0, dB)],
        "empty": [],
        "seventy views": [f(3, 2, h, r, dA) for h, r in views] + [f(3, 2, *views[66], dB), f(3, 2, *views[1], dB),
                                                                   f(3, 2, *views[69], dC)],
    }
    assert tuple(inst) == NAMES
    stream, off, f0 = XR.stream_of(list(inst.values()))
    return dict(cfg=cfg, secrets=sec, stream=stream, off=off, f0=f0, heights=H, index={k: i for i, k in enumerate(NAMES)},
                want=_want(cfg, stream, off, f0, H), want_cap2=_want(cfg, stream, off, f0, H, view_cap=2),
                want_rec1=_want(cfg, stream, off, f0, H, rec_cap=1))


def check_handmade(c):
    """what each instance was built to show, on the reference's verdict (relative frame pairs per instance)"""
    import audit_ref as AR
    w, f0 = c["want"], [int(x) for x in c["f0"]]
    pairs = {name: [(int(r["frame_a"]) - f0[i], int(r["frame_b"]) - f0[i], int(r["signer"]), int(r["code"]))
                    for r in w["records"] if r["inst"] == i] for name, i in c["index"].items()}
    assert pairs == {"three digests": [(0, 1, 0, 2)], "duplicate": [], "first frame unrecoverable": [(1, 2, 0, 2)],
                     "other round, other code": [], "round above 2^32": [(0, 2, 1, 2)], "heights out of range": [],
                     "round changes": [], "foreign seal": [(0, 1, 0, 3)], "two chunks apart": [(0, 71, 2, 2)], "empty": [],
                     "seventy views": [(66, 70, 3, 2), (1, 71, 3, 2), (69, 72, 3, 2)]}, pairs
    st = w["audit"]["frame_status"]
    assert st[f0[c["index"]["first frame unrecoverable"]]] == AR.ST_UNRECOVERABLE
    assert st[f0[c["index"]["foreign seal"]] + 1] == AR.ST_SEAL_FOREIGN
    assert (np.delete(st, [f0[2], f0[7] + 1]) == AR.ST_OK).all()
    big = [r for r in w["records"] if r["inst"] == c["index"]["round above 2^32"]]
    assert int(big[0]["round"]) == (1 << 32) + 5
    assert not w["inst_flags"].any() and w["report"]["view_overflows"] == 0
    assert w["report"] == dict(records=8, by_code=[0, 7, 1], accused=6, accused_instances=6, view_overflows=0)
    # view_cap 2: the instances with a third view overflow; what they found within their first two views stays
    c2 = c["want_cap2"]
    over = {name for name, i in c["index"].items() if c2["inst_flags"][i] & XR.VIEW_OVERFLOW}
    assert over == {"other round, other code", "seventy views"} and c2["report"]["view_overflows"] == 2
    assert [(int(r["frame_a"]) - f0[10], int(r["frame_b"]) - f0[10]) for r in c2["records"] if r["inst"] == 10] == [(1, 71)]
    assert c2["report"]["records"] == 6
    # rec_cap 1: the first record alone, the report and the other arrays whole
    c1 = c["want_rec1"]
    assert len(c1["records"]) == 1 and c1["records"].tolist() == w["records"][:1].tolist() and c1["report"] == w["report"]
    assert np.array_equal(c1["frame_pair"], w["frame_pair"])
