#!/usr/bin/env python3
"""Measures the accuser (bftsim_accuse_last_trace, SPEC.md §11g) on one GPU: cfg3 (N = 64, 21 equivocating
validators), 1,024 instances x 10 heights, every broadcast signed, twins on. After one launch + bftsim_crypto_verify
(keep on) it accuses the whole kept trace 1 + 5 times and records, from the library's HIP events (bftsim_accuse_last_ms
and bftsim_audit_last_ms of the same call), the walk kernel and the compaction (mark + scan + gather) beside the
observer's decode, recoveries and classify + tally; the walk against classify + tally, the pass with the same
wave-per-instance walk over the same frames; and checks the records against the twins (every twin's sender accused,
the accused within the seeded Byzantine set). --parent-lib: bftsim_audit_last_trace alone, 1 + repeats times per
process, in child processes that alternate between the parent commit's libbftsim and this one, recorded side by side:
the observer's passes must stay inside the parent's own min-max.

    python scripts/accuse_bench.py [--instances 1024] [--heights 10] [--repeats 5] [--parent-lib LIB.so] [--rounds 3]
                                   [--out FILE.json]
"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def kept_trace(args):
    from bftsim.configs import cfg3
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.runtime import Simulator, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(64, 3)
    cfg, secrets = keyed_config(cfg3(heights=args.heights), sec, [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), 24_576)
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    sim.prepare(args.instances)
    sim.launch(0)
    sim.sync()
    rep = sim.crypto_verify()
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0 and rep["log_overflows"] == 0, rep
    return cfg, sim


def measure_audit(args):
    """the observer alone (what both libraries have): per-pass device ms of 1 + repeats bftsim_audit_last_trace"""
    cfg, sim = kept_trace(args)
    rows, first = [], None
    for r in range(1 + args.repeats):
        a = sim.audit_last_trace()
        first = first or a.report
        assert a.report == first
        if r:
            d, rc, t, cp = sim.audit_ms()
            rows.append(dict(decode_ms=d, recover_ms=rc, tally_ms=t, copy_ms=cp))
    sim.close()
    return dict(audit_report=first, rows=rows)


def byz_masks(cfg, n):
    """the seeded Byzantine set of instances 0..n - 1 (SPEC.md §5), from the test oracle if it is built"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import oracle_lib as O
    c, keep = O.to_orc(cfg)
    out = []
    for i in range(n):
        m = (ctypes.c_uint64 * 4)()
        O.lib().orc_byz_mask(ctypes.byref(c), ctypes.c_uint32(i), m)
        out.append([int(x) for x in m])
    del keep
    return out


def measure(args):
    import numpy as np
    cfg, sim = kept_trace(args)
    twins = sim.trace_twin_counts()
    rows, first = [], None
    for r in range(1 + args.repeats):                      # the first is the warm-up
        t0 = time.perf_counter()
        a = sim.accuse_last_trace()
        wall = time.perf_counter() - t0
        if first is None:
            first = a
        assert a.report == first.report and a.audit.report == first.audit.report
        if r:
            au, wk, cm, cp = sim.accuse_ms()
            d, rc, t, _ = sim.audit_ms()
            rows.append(dict(audit_ms=au, walk_ms=wk, compact_ms=cm, copy_ms=cp, decode_ms=d, recover_ms=rc, tally_ms=t,
                             wall_ms=1000 * wall))
    tr = sim.export_trace()
    sim.close()
    tw = tr.twin
    # every twin's sender is accused in its instance; the accused are within the seeded Byzantine set
    inst, sender = tr.instance[tw].astype(np.int64), tr.sender[tw].astype(np.int64)
    bit = (first.inst_accused[inst, sender >> 6] >> (sender & 63).astype(np.uint64)) & np.uint64(1)
    checks = dict(twins=int(tw.sum()), twin_senders_accused=bool(bit.all()),
                  frame_b_are_twins=bool(tw[first.records["frame_b"]].all()))
    try:
        byz = np.array(byz_masks(cfg, args.instances), np.uint64)
        checks["accused_within_seeded_byzantine"] = bool(((first.inst_accused & ~byz) == 0).all())
    except Exception as e:                                 # the oracle is test infrastructure: the timings stand without it
        checks["accused_within_seeded_byzantine"] = f"not checked: {e}"
    return dict(report=first.report, audit_report=first.audit.report, twin_counts=list(twins), frames=len(tr),
                checks=checks, rows=rows)


def summary(rows, keys):
    def med(k):
        v = sorted(r[k] for r in rows)
        return v[len(v) // 2]
    s = {k: [round(r[k], 4) for r in rows] for k in keys}
    s.update({k + "_median": med(k) for k in keys})
    s.update({k + "_minmax": [min(r[k] for r in rows), max(r[k] for r in rows)] for k in keys})
    return s


def child_audit(args, lib_path):
    env = dict(os.environ)
    if lib_path:
        env.update(BFTSIM_TESTING="1", BFTSIM_LIB=os.path.abspath(lib_path))
    cmd = [sys.executable, os.path.abspath(__file__), "--child-audit", "--instances", str(args.instances), "--heights",
           str(args.heights), "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child run failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--heights", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library under --parent-lib")
    ap.add_argument("--child-audit", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r13", "accuse", "accuse_bench.json"))
    args = ap.parse_args()
    if args.child_audit:
        print(json.dumps(measure_audit(args)))
        return
    m = measure(args)
    keys = ("audit_ms", "walk_ms", "compact_ms", "copy_ms", "decode_ms", "recover_ms", "tally_ms", "wall_ms")
    s = summary(m["rows"], keys)
    own = s["walk_ms_median"] + s["compact_ms_median"]
    s["walk_over_tally"] = s["walk_ms_median"] / s["tally_ms_median"]
    s["accuse_over_tally"] = own / s["tally_ms_median"]
    s["accuse_share_of_device"] = own / (s["audit_ms_median"] + own)
    out = dict(shape=f"cfg3 (21 Byzantine of 64), twins on, {args.instances} instances x {args.heights} heights, one GPU; "
                     f"1 warm-up + {args.repeats} repeats; tally_ms is the observer's classify + tally",
               frames=m["frames"], twin_counts=m["twin_counts"], report=m["report"], audit_report=m["audit_report"],
               checks=m["checks"], library=s)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def dump():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    dump()                                                 # the accuser's timings are kept whatever the A/B does
    if args.parent_lib:                                    # fresh processes: a binding loads one library
        akeys = ("decode_ms", "recover_ms", "tally_ms")
        sides = dict(parent=[], this=[])
        for _ in range(args.rounds):                       # interleaved: parent, this, parent, this, ...
            for side, path in (("parent", args.parent_lib), ("this", None)):
                c = child_audit(args, path)
                assert c["audit_report"] == m["audit_report"], f"{side}: the observer's report differs"
                sides[side] += c["rows"]
        ab = {side: summary(rows, akeys) for side, rows in sides.items()}
        ab["this_inside_parent_minmax"] = {k: bool(ab["parent"][k + "_minmax"][0] <= ab["this"][k + "_median"] <=
                                                   ab["parent"][k + "_minmax"][1]) for k in akeys}
        out["audit_last_trace_ab"] = ab
        dump()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
