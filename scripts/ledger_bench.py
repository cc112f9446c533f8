#!/usr/bin/env python3
"""Measures the importer (bftsim_verify_ledger, SPEC.md §11d) on one GPU: cfg3's shape with
byz_count = 0 (N = 64), 1,024 instances x 10 heights, the ledger kept with commit seals. After one launch +
bftsim_crypto_verify + bftsim_export_ledger it verifies the exported ledger 1 + 5 times and records, from the library's
HIP events (bftsim_ledger_last_ms), decode (with the vote scan and scatter), the recoveries, tally + link and the copies;
votes and headers per second; the share of everything but the recoveries. Then the tally-mapping A/B: the same ledger,
and an N = 4 ledger of 3 votes a header (--small-instances), with the tally forced to a lane per header and to a wave
per header (BFTSIM_TESTING=1 + BFTSIM_LEDGER_TALLY, read by every call).

    python scripts/ledger_bench.py [--instances 1024] [--heights 10] [--repeats 5] [--small-instances 16384] [--out FILE.json]
"""
import argparse
import dataclasses
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def med(v):
    v = sorted(v)
    return v[len(v) // 2]


def sealed_ledger(cfg, seed, instances, log_cap):
    """a run of `cfg` with seals kept -> (sim, packed ledger arrays, result)"""
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.ledger import pack
    from bftsim.runtime import Simulator, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(cfg.n, seed)
    cfg, secrets = keyed_config(cfg, sec, [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), log_cap)
    sim.set_ledger_votes("seals")
    sim.prepare(instances)
    sim.launch(0)
    sim.sync()
    rep = sim.crypto_verify()
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0, rep
    res = sim.fetch()
    return sim, pack(sim.export_ledger(), heights=cfg.heights), res


def timed(sim, packed, repeats, mapping=None):
    """1 warm-up + `repeats` calls -> (verdict, rows); mapping: None (the library's choice), 1 lane, 2 wave per header"""
    before = {k: os.environ.get(k) for k in ("BFTSIM_TESTING", "BFTSIM_LEDGER_TALLY")}
    if mapping is None:
        os.environ.pop("BFTSIM_LEDGER_TALLY", None)
    else:
        os.environ["BFTSIM_TESTING"], os.environ["BFTSIM_LEDGER_TALLY"] = "1", str(mapping)
    rows, first = [], None
    for r in range(1 + repeats):
        t0 = time.perf_counter()
        v = sim.verify_ledger(packed)
        wall = time.perf_counter() - t0
        first = first or v
        assert v.report == first.report and (v.status == first.status).all()
        if r:
            d, rc, t, c = sim.ledger_ms()
            rows.append(dict(decode_ms=d, recover_ms=rc, tally_ms=t, copy_ms=c, wall_ms=1000 * wall))
    for k, val in before.items():                          # the switches hold for these calls alone
        if val is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = val
    return first, rows


def summary(v, rows):
    d, rc, t = (med([r[k] for r in rows]) for k in ("decode_ms", "recover_ms", "tally_ms"))
    span = lambda k: [round(min(r[k] for r in rows), 4), round(max(r[k] for r in rows), 4)]
    return dict(decode_ms_median=d, recover_ms_median=rc, tally_ms_median=t, copy_ms_median=med([r["copy_ms"] for r in rows]),
                wall_ms_median=med([r["wall_ms"] for r in rows]), decode_ms=span("decode_ms"), recover_ms=span("recover_ms"),
                tally_ms=span("tally_ms"), copy_ms=span("copy_ms"), wall_ms=span("wall_ms"),
                votes_per_s=v.report["votes"] / ((d + rc + t) * 1e-3), headers_per_s=v.report["headers"] / ((d + rc + t) * 1e-3),
                recoveries_per_s=v.report["recoveries"] / (rc * 1e-3) if rc else None, own_share=(d + t) / (d + rc + t))


def main():
    from bftsim.configs import BftConfig, cfg3
    from bftsim.ledger import compare
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--heights", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small-instances", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r10", "ledger_verify", "ledger_bench.json"))
    args = ap.parse_args()
    cfg = dataclasses.replace(cfg3(heights=args.heights), byz_count=0, name="cfg3-honest")
    sim, packed, res = sealed_ledger(cfg, 3, args.instances, 24_576)
    v, rows = timed(sim, packed, args.repeats)
    c = {k: int(x.sum()) for k, x in compare(v, res).items()}
    assert c["ok"] == c["same_hash"] == int(res["committed_height"].sum()) == v.report["by_status"][0], (c, v.report)
    out = dict(shape=f"cfg3 with byz_count = 0 (N = 64), {args.instances} instances x {args.heights} heights, one GPU; "
                     f"1 warm-up + {args.repeats} repeats", slot_bytes=int(packed[2]), report=v.report, compare=c,
               library=summary(v, rows), tally_ab={})
    ab = out["tally_ab"]["n64"] = {}
    for name, m in (("lane_per_header", 1), ("wave_per_header", 2)):
        v2, r2 = timed(sim, packed, args.repeats, m)
        assert v2.report == v.report and (v2.voters == v.voters).all()
        ab[name] = dict(tally_ms_median=med([r["tally_ms"] for r in r2]),
                        tally_ms=[round(min(r["tally_ms"] for r in r2), 4), round(max(r["tally_ms"] for r in r2), 4)])
    sim.close()
    if args.small_instances:
        small = BftConfig(n=4, heights=args.heights, seed=21)
        sim, packed, res = sealed_ledger(small, 7, args.small_instances, 0)
        ab = out["tally_ab"]["n4"] = dict(shape=f"N = 4, {args.small_instances} instances x {args.heights} heights, 3 votes a header")
        base = None
        for name, m in (("lane_per_header", 1), ("wave_per_header", 2)):
            v2, r2 = timed(sim, packed, args.repeats, m)
            base = base or v2
            assert v2.report == base.report and v2.report["by_status"][0] == int(res["committed_height"].sum())
            ab[name] = dict(tally_ms_median=med([r["tally_ms"] for r in r2]),
                            tally_ms=[round(min(r["tally_ms"] for r in r2), 4), round(max(r["tally_ms"] for r in r2), 4)])
        ab["headers"], ab["votes"] = base.report["headers"], base.report["votes"]
        sim.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
