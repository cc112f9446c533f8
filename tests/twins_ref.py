"""CPU reference of trace twins (SPEC.md §11f), test infrastructure only: the reference trace of tests/trace_ref.py
with the second frame of every equivocating broadcast inserted behind its original. Built from the oracle's broadcast
log alone (oracle_lib.run_crypto), with the helpers of crypto_ref on the flipped block id, the msgpack oracle and the
Python secp256k1 oracle. Independent of the code under test."""
from __future__ import annotations

import functools

import msgpack
import numpy as np

import trace_ref as TR          # first: it puts oracle/ on the path
import crypto_ref as C
import oracle_lib as O
import wire_ref as R

FORGED, WILD, EQUIV, OLD = 1, 2, 4, 8
TWIN = 1 << 16                  # frame_meta word 2 of a twin
FLIP = 1 << 33                  # the variant bit of a block id


def log_of(res, i):
    return res["mlog"][i, : int(res["mlog_n"][i])]


def byzantine_senders(log) -> set:
    """the Byzantine validators of an instance as its log shows them: every sender of an equivocating PrePrepare or of
    a wildcard vote"""
    return {int(e[1]) >> 16 for e in log if int(e[6]) & (WILD | EQUIV)}


def needs_twin(e, byz) -> int:
    """0: none; 1: a PrePrepare's twin; 2: a vote's twin"""
    code, fl = (int(e[1]) >> 8) & 0xff, int(e[6])
    b = int(e[4]) | (int(e[5]) << 32)
    if code == 1:
        return 1 if fl & EQUIV else 0
    if code in (2, 3) and fl & WILD:
        u = C._unpack(b)
        if u["valid"] and u["h"] != 0 and u["prop"] in byz:
            return 2
    return 0


def messages(cfg, first, res, i, secrets, forged=()):
    """trace_ref.messages of instance i with the twins inserted: each dict carries twin (bool); a twin's meta has TWIN
    set in its flags. -> (messages, (PrePrepare twins, vote twins))"""
    ms = TR.messages(cfg, first, res, i, secrets, forged)
    log = log_of(res, i)
    byz = byzantine_senders(log)
    genesis = TR.genesis_hash(cfg)
    inst = first + i
    tw = []
    for k, (e, m) in enumerate(zip(log, ms)):
        kind = needs_twin(e, byz)
        if not kind:
            continue
        b = (int(e[4]) | (int(e[5]) << 32)) ^ FLIP
        d = C._digest(cfg, res, i, inst, b, genesis)
        hdr = None
        if m["code"] == 1:
            u = C._unpack(b)
            hdr = C._header(cfg, inst, u["h"], u["prop"], u["var"], u["T"], C._parent(cfg, res, i, u["h"], genesis))
            msg = b"\x92" + msgpack.packb([m["round"], m["height"]]) + b"\x92" + hdr + b"\x90"
        else:
            msg = R.subject(m["round"], m["height"], d)
        tick, w1, fl = m["meta"]
        tw.append((k, dict(code=m["code"], ctime=m["ctime"], round=m["round"], height=m["height"], digest=d, header=hdr,
                           sig=None, seal=None, msg=msg, key=m["key"], meta=(tick, w1, fl | TWIN), twin=True, kind=kind)))
    cm = [t for _, t in tw if t["code"] == 3]
    for t, seal in zip(cm, TR.sign_many([(t["key"], O.keccak256(bytes([3]) + t["digest"])) for t in cm])):
        t["seal"] = seal
    sigs = TR.sign_many([(t["key"], O.keccak256(R.gossip(t["code"], t["ctime"], t["msg"], None, t["seal"]))) for _, t in tw])
    for (_, t), sig in zip(tw, sigs):
        t["sig"] = sig
    after = dict(tw)
    out = []
    for k, m in enumerate(ms):
        out.append(dict(m, twin=False))
        if k in after:
            out.append(after[k])
    return out, (sum(t["kind"] == 1 for _, t in tw), sum(t["kind"] == 2 for _, t in tw))


def instance_trace(cfg, first, res, i, secrets, forged=(), rel=0):
    """trace_ref.instance_trace with twins -> (stream, frame_off, meta, messages, twin counts)"""
    ms, counts = messages(cfg, first, res, i, secrets, forged)
    frames = [TR.frame_of(m) for m in ms]
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    meta = np.array([list(m["meta"]) + [rel] for m in ms], np.uint32).reshape(-1, 4)
    return b"".join(frames), off, meta, ms, counts


def plain_of(inst):
    """the twins-off trace inside a twinned instance tuple: (stream, frame_off, meta, messages)"""
    ms = [m for m in inst[3] if not m["twin"]]
    frames = [TR.frame_of(m) for m in ms]
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    meta = np.array([list(m["meta"]) + [0] for m in ms], np.uint32).reshape(-1, 4)
    return b"".join(frames), off, meta, ms


# ---- the shapes the CPU and the GPU tests share, each computed once per session

def _keyed(cfg, seed):
    import secp256k1_ref as S
    from bftsim.crypto import synthetic_secrets, keyed_config
    sec = synthetic_secrets(cfg.n, seed)
    return keyed_config(cfg, sec, [S.address(S.pubkey(k), O.keccak256) for k in sec])


@functools.lru_cache(maxsize=None)
def reference(case: str):
    """'n7': N = 7, byz_count 2, seed 5, 6 heights, lossless, synthetic keys, instances 2..4 (the pinned case: instance
    2 commits variant 1 at heights 3 and 6, instance 4 at height 5, instance 3 never);
    'n4': N = 4, byz_count 1, seed 21, 6 heights, drop_ppm 100,000, instances 3..5, validator `forged` forged.
    -> dict(cfg, secrets, first, n, forged, res, inst=[twinned instance tuples], plain=[twins-off tuples])"""
    from bftsim.configs import BftConfig
    if case == "n7":
        cfg, secrets = _keyed(BftConfig(n=7, heights=6, seed=5, byz_count=2), 7)
        first, n, forged = 2, 3, ()
    elif case == "n4":
        cfg, secrets = _keyed(BftConfig(n=4, heights=6, seed=21, byz_count=1, drop_ppm=100_000), 7)
        first, n = 3, 3
        probe = O.run_crypto(cfg, first, n)
        byz = sorted(set().union(*[byzantine_senders(log_of(probe, i)) for i in range(n)]))
        forged = (byz[0],) if byz else (2,)     # a Byzantine validator of some instance of the range
    else:
        raise KeyError(case)
    res = O.run_crypto(cfg, first, n, forged=forged)
    inst = [instance_trace(cfg, first, res, i, secrets, forged, rel=i) for i in range(n)]
    return dict(cfg=cfg, secrets=secrets, first=first, n=n, forged=forged, res=res, inst=inst,
                plain=[plain_of(t) for t in inst], counts=tuple(sum(t[4][k] for t in inst) for k in (0, 1)))


def joined(ref, begin=0, count=None, plain=False):
    """trace_ref.joined over the twinned (or the plain) instances"""
    return TR.joined(dict(ref, inst=[t[:4] for t in (ref["plain"] if plain else ref["inst"])]), begin, count)


def verdicts(cfg, res, stream, off, f0):
    """the Python observer's, archiver's and importer's verdicts on a stream -> dict(archive, ledger, certified: [n, H]
    bool, the observer certified the run's own block hash)"""
    import archive_ref as ARC
    import ledger_ref as LR
    from bftsim.ledger import pack
    H = cfg.heights
    arc = ARC.archive(stream, off, f0, cfg.addresses, cfg.seed_byte_order == 1, H, 0)
    hdr, lens, slot, _ = pack(arc["headers"], slot_bytes=ARC.slot_bytes(cfg.n), heights=H)
    led = LR.verify(hdr, lens, slot, H, cfg, TR.genesis_hash(cfg))
    a = arc["audit"]
    n = len(f0) - 1
    cert = np.zeros((n, H), bool)
    for i in range(n):
        for x in range(int(res["committed_height"][i])):
            cert[i, x] = int(np.asarray(a["cert_round"]).reshape(n, H)[i, x]) != 0xffff and \
                bytes(np.asarray(a["cert_digest"]).reshape(n, H, 32)[i, x]) == bytes(res["block_hash"][i, x])
    return dict(archive=arc, ledger=led, certified=cert)
