#!/usr/bin/env python3
"""Measures the trace export (bftsim_export_trace, SPEC.md §11b) on one GPU at the crypto line's
shape: cfg3, 1,024 instances x 10 heights, every broadcast signed. After one launch + bftsim_crypto_verify (keep on)
it exports the whole launch 1 + 5 times with the library's emitter (`coop`: a wave per 64 frames through an LDS
stage, 16-byte coalesced stores; the lane-per-frame emitter it was measured against is retired)
and records, from the library's HIP events, the emit kernel's frames/s and device-side GB/s, the device-to-host
copy time, the size pass, and the wall time of the verify pass in the same process.

    python scripts/trace_bench.py [--instances 1024] [--heights 10] [--repeats 5] [--twins] [--out FILE.json]

--twins (SPEC.md §11f): the verifies run with bftsim_set_trace_twins on, and the record gains the twin
counts, their share of the frames, and per verify the device times of the twin passes (mark + scan + merge, digests,
signing) next to the size pass and the emit kernel, which then run over the merged index.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--heights", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--twins", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07", "trace_export", "trace_bench.json"))
    args = ap.parse_args()
    from bftsim.configs import cfg3
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.runtime import Simulator, lib, _check, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(64, 3)
    cfg, secrets = keyed_config(cfg3(heights=args.heights), sec, [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), 24_576)
    sim.set_trace_keep(True)
    sim.set_trace_twins(args.twins)
    sim.prepare(args.instances)
    verify_s, twin_ms, size_each = [], [], []
    for _ in range(1 + args.repeats):                      # the first is the warm-up
        sim.launch(0)
        sim.sync()
        t0 = time.perf_counter()
        rep = sim.crypto_verify()
        verify_s.append(time.perf_counter() - t0)
        twin_ms.append(sim.trace_twins_ms())
        sim.trace_sizes()                                   # the size pass + scan of this verify's trace
        size_each.append(sim.trace_ms()[0])
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0, rep
    t0 = time.perf_counter()
    fr, by = sim.trace_sizes()
    sizes_wall = time.perf_counter() - t0
    size_ms = sim.trace_ms()[0]
    frames, nbytes = int(fr.sum()), int(by.sum())
    twins = sim.trace_twin_counts()
    stream, off = np.zeros(nbytes, np.uint8), np.zeros(frames + 1, np.uint64)
    rows = []
    for r in range(1 + args.repeats):
        t0 = time.perf_counter()
        rc = lib().bftsim_export_trace(sim.h, 0, args.instances, stream.ctypes.data, nbytes, off.ctypes.data, frames,
                                       None, None)
        wall = time.perf_counter() - t0
        _check(sim.h, rc, "bftsim_export_trace")
        _, emit_ms, copy_ms = sim.trace_ms()
        if r == 0:                                           # warm-up; the stream's digest identifies the bytes
            dig = ctypes.create_string_buffer(32)
            lib().bftsim_keccak256(ctypes.cast(stream.ctypes.data, ctypes.c_char_p), nbytes, dig)
            continue
        rows.append(dict(emit_ms=emit_ms, copy_ms=copy_ms, wall_ms=1000 * wall))
    sim.close()

    def summary(rows):
        e = sorted(x["emit_ms"] for x in rows)
        med = e[len(e) // 2]
        return dict(emit_ms=[round(x["emit_ms"], 4) for x in rows], emit_ms_median=med, emit_ms_min=e[0], emit_ms_max=e[-1],
                    frames_per_s=frames / (med * 1e-3), device_GB_per_s=nbytes / (med * 1e-3) / 1e9,
                    copy_ms=[round(x["copy_ms"], 3) for x in rows], wall_ms=[round(x["wall_ms"], 3) for x in rows])

    out = dict(shape=f"cfg3, {args.instances} instances x {args.heights} heights, one GPU; 1 warm-up + {args.repeats} repeats",
               frames=frames, stream_bytes=nbytes, mean_frame_bytes=nbytes / max(frames, 1),
               messages=rep["messages"], seals=rep["seals"],
               verify_wall_ms=[round(1000 * x, 2) for x in verify_s[1:]], size_pass_ms=size_ms, sizes_call_wall_ms=1000 * sizes_wall,
               coop=summary(rows), stream_keccak256=dig.raw.hex())
    out["size_pass_ms_each"] = [round(x, 4) for x in size_each[1:]]
    if args.twins:
        pp, votes = twins
        med = lambda xs: sorted(xs)[len(xs) // 2]
        t = dict(pp_twins=pp, vote_twins=votes, twin_share_of_frames=(pp + votes) / max(frames, 1),
                 index_ms=[round(x[0], 4) for x in twin_ms[1:]], digest_ms=[round(x[1], 4) for x in twin_ms[1:]],
                 sign_ms=[round(x[2], 4) for x in twin_ms[1:]])
        t["median_ms"] = dict(index=med(t["index_ms"]), digest=med(t["digest_ms"]), sign=med(t["sign_ms"]),
                              size=med(out["size_pass_ms_each"]), emit=out["coop"]["emit_ms_median"])
        t["twin_passes_over_verify_wall"] = (t["median_ms"]["index"] + t["median_ms"]["digest"] + t["median_ms"]["sign"]) * 1e-3 / \
            sorted(verify_s[1:])[len(verify_s[1:]) // 2]
        out["twins"] = t
    vmed = sorted(verify_s[1:])[len(verify_s[1:]) // 2]
    out["emit_over_verify"] = out["coop"]["emit_ms_median"] * 1e-3 / vmed
    out["export_wall_over_verify"] = sorted(out["coop"]["wall_ms"])[len(out["coop"]["wall_ms"]) // 2] * 1e-3 / vmed
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
