"""CPU reference of the trace (SPEC.md §11b), test infrastructure only: from the oracle's broadcast log
(oracle_lib.run_crypto) the wire frame of every logged message, built with the msgpack oracle (oracle/wire_ref.py)
and the Python secp256k1 oracle, through the helpers of crypto_ref. Independent of the code under test."""
from __future__ import annotations

import ctypes
import functools
import json
import os

import msgpack
import numpy as np

import crypto_ref as C
import oracle_lib as O
import secp256k1_ref as S
import wire_ref as R


def genesis_hash(cfg) -> bytes:
    c, keep = O.to_orc(cfg)
    g = (ctypes.c_uint8 * 32)()
    O.lib().orc_genesis_hash(ctypes.byref(c), g)
    del keep
    return bytes(g)


_pool = None


def sign_many(jobs):
    """[S.sign(key, digest) for key, digest in jobs]; a long list (the Python oracle signs ~25 per second) over
    fresh worker processes that import the oracle alone (one pool per session, closed at exit)"""
    global _pool
    if len(jobs) < 64:
        return [S.sign(k, d) for k, d in jobs]
    if _pool is None:
        import atexit
        import multiprocessing as mp
        _pool = mp.get_context("spawn").Pool(min(16, os.cpu_count() or 1))
        atexit.register(_pool.terminate)
    return _pool.starmap(S.sign, jobs, chunksize=8)


def messages(cfg, first, res, i, secrets, forged=()):
    """the logged messages of instance i of a run_crypto result, as dicts with every value the frame carries:
    code, ctime, round, height, digest, header (Preprepare, else None), sig, seal (Commit, else None), meta"""
    genesis = genesis_hash(cfg)
    keys = list(secrets) + [O.keccak256(k) for k in secrets]
    fs = set(forged)
    inst = first + i
    out = []
    for e in res["mlog"][i, : int(res["mlog_n"][i])]:
        tick, w1, h, r = int(e[0]), int(e[1]), int(e[2]), int(e[3])
        code, sender = (w1 >> 8) & 0xff, w1 >> 16
        b = int(e[4]) | (int(e[5]) << 32)
        key = keys[sender + (cfg.n if sender in fs else 0)]
        assert bool(int(e[6]) & 1) == (sender in fs)
        ctime = 1000 * (cfg.genesis_time + cfg.block_period * tick) if code == 4 else 0
        d = bytes(32) if code == 4 else C._digest(cfg, res, i, inst, b, genesis)
        hdr = None
        if code == 1:
            u = C._unpack(b)
            hdr = C._header(cfg, inst, u["h"], u["prop"], u["var"], u["T"], C._parent(cfg, res, i, u["h"], genesis))
            msg = b"\x92" + msgpack.packb([r, h]) + b"\x92" + hdr + b"\x90"
        else:
            msg = R.subject(r, h, d)
        out.append(dict(code=code, ctime=ctime, round=r, height=h, digest=d, header=hdr, sig=None, seal=None, msg=msg,
                        key=key, meta=(tick, w1, int(e[6]))))
    # the Commits' seals first (they are part of the sign payload), then every message's signature
    cm = [m for m in out if m["code"] == 3]
    for m, seal in zip(cm, sign_many([(m["key"], O.keccak256(bytes([3]) + m["digest"])) for m in cm])):
        m["seal"] = seal
    sigs = sign_many([(m["key"], O.keccak256(R.gossip(m["code"], m["ctime"], m["msg"], None, m["seal"]))) for m in out])
    for m, sig in zip(out, sigs):
        m["sig"] = sig
    return out


def frame_of(m) -> bytes:
    return R.frame(R.gossip(m["code"], m["ctime"], m["msg"], m["sig"], m["seal"]))


def instance_trace(cfg, first, res, i, secrets, forged=(), rel=0):
    """-> (stream bytes, frame_off [k + 1] uint64, meta [k, 4] uint32, messages) of instance i; rel: the instance
    index the meta's last column carries"""
    ms = messages(cfg, first, res, i, secrets, forged)
    frames = [frame_of(m) for m in ms]
    off = np.zeros(len(frames) + 1, np.uint64)
    off[1:] = np.cumsum([len(f) for f in frames])
    meta = np.array([list(m["meta"]) + [rel] for m in ms], np.uint32).reshape(-1, 4)
    return b"".join(frames), off, meta, ms


# ---- the shapes the CPU and the GPU tests share, each computed once per session
def _reference_keys():
    gold = json.load(open(os.path.join(os.path.dirname(__file__), "golden", "sig_vectors.json")))
    return {bytes.fromhex(k["address"]): bytes.fromhex(k["secret"]) for k in gold["reference_keys"]}


@functools.lru_cache(maxsize=None)
def reference(case: str):
    """'cfg1': cfg1 (N=5, c1..c5 keys of examples/*.toml, c5 silent), 6 heights, instance 0;
    'n4': N=4, seed 21, 6 heights, drop_ppm 100,000, instances 3..5, validator 2 forged.
    -> dict(cfg, secrets, first, n, forged, res, inst=[(stream, frame_off, meta, messages) per instance])"""
    from bftsim.configs import BftConfig, cfg1
    from bftsim.crypto import synthetic_secrets, keyed_config
    if case == "cfg1":
        keys = _reference_keys()
        cfg = cfg1(True, heights=6)
        secrets, first, n, forged = [keys[a] for a in cfg.addresses], 0, 1, ()
    elif case == "n4":
        sec = synthetic_secrets(4, 7)
        cfg, secrets = keyed_config(BftConfig(n=4, heights=6, seed=21, drop_ppm=100_000), sec,
                                    [S.address(S.pubkey(k), O.keccak256) for k in sec])
        first, n, forged = 3, 3, (2,)
    else:
        raise KeyError(case)
    res = O.run_crypto(cfg, first, n, forged=forged)
    inst = [instance_trace(cfg, first, res, i, secrets, forged, rel=i) for i in range(n)]
    return dict(cfg=cfg, secrets=secrets, first=first, n=n, forged=forged, res=res, inst=inst)


def joined(ref, begin=0, count=None):
    """instances [begin, begin + count) of a reference() as one trace: (stream, frame_off, meta, inst_frame0)"""
    count = ref["n"] - begin if count is None else count
    stream, offs, metas, f0 = b"", [np.zeros(1, np.uint64)], [], [0]
    for rel in range(count):
        s, o, m, _ = ref["inst"][begin + rel]
        offs.append(o[1:] + np.uint64(len(stream)))
        stream += s
        m = m.copy()
        m[:, 3] = rel
        metas.append(m)
        f0.append(f0[-1] + len(m))
    return stream, np.concatenate(offs), np.concatenate(metas).reshape(-1, 4), np.array(f0, np.uint64)
