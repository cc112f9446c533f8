#!/usr/bin/env python3
"""Measures the chronicler (bftsim_timeline_last_trace, SPEC.md §11h) on one GPU over two shapes: cfg3
(N = 64, 21 equivocating validators) with twins, 1,024 instances x 10 heights (Prepare keys with two digests, no round
changes), and the same shape with 5 % drops at 256 instances (the round-change path). After one launch +
bftsim_crypto_verify (keep on) it chronicles the whole kept trace 1 + 5 times and records, from the library's HIP events
(bftsim_timeline_last_ms and bftsim_audit_last_ms of the same call), the walk and the rows kernels beside the observer's
decode, recoveries and classify + tally; walk + rows against classify + tally, the pass with the same wave-per-instance
walk over the same frames. --parent-lib: bftsim_audit_last_trace alone, 1 + repeats times per process, in child processes
that alternate between the parent commit's libbftsim and this one, recorded side by side: the observer's passes must stay
inside the parent's own min-max. --bench-rounds N (with --parent-lib): bench.py --gpus 1 --steps 20 --warmup 5 as well,
N processes per library, interleaved, into profiles/r14/timeline/bench_ab.json.

    python scripts/timeline_bench.py [--repeats 5] [--parent-lib LIB.so] [--rounds 3] [--bench-rounds 0]
                                     [--out FILE.json] [--bench-out FILE.json]
"""
import argparse
import json
import os
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
SHAPES = dict(twins=dict(instances=1024, heights=10, drop_ppm=0, log_cap=24_576),
              lossy=dict(instances=256, heights=10, drop_ppm=50_000, log_cap=98_304))


def kept_trace(shape):
    import dataclasses
    from bftsim.configs import cfg3
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.runtime import Simulator, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(64, 3)
    base = dataclasses.replace(cfg3(heights=shape["heights"]), drop_ppm=shape["drop_ppm"])
    cfg, secrets = keyed_config(base, sec, [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), shape["log_cap"])
    sim.set_trace_keep(True)
    sim.set_trace_twins(True)
    sim.prepare(shape["instances"])
    sim.launch(0)
    sim.sync()
    rep = sim.crypto_verify()
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0, rep
    return cfg, sim, rep


def measure_audit(shape, repeats):
    """the observer alone (what both libraries have): per-pass device ms of 1 + repeats bftsim_audit_last_trace"""
    cfg, sim, _ = kept_trace(shape)
    rows, first = [], None
    for r in range(1 + repeats):
        a = sim.audit_last_trace()
        first = first or a.report
        assert a.report == first
        if r:
            d, rc, t, cp = sim.audit_ms()
            rows.append(dict(decode_ms=d, recover_ms=rc, tally_ms=t, copy_ms=cp))
    sim.close()
    return dict(audit_report=first, rows=rows)


def measure(shape, repeats):
    cfg, sim, rep = kept_trace(shape)
    rows, first = [], None
    for r in range(1 + repeats):                           # the first is the warm-up
        t0 = time.perf_counter()
        a = sim.timeline_last_trace()
        wall = time.perf_counter() - t0
        if first is None:
            first = a
        assert a.report == first.report and a.audit.report == first.audit.report
        if r:
            au, wk, rw, cp = sim.timeline_ms()
            d, rc, t, _ = sim.audit_ms()
            rows.append(dict(audit_ms=au, walk_ms=wk, rows_ms=rw, copy_ms=cp, decode_ms=d, recover_ms=rc, tally_ms=t,
                             wall_ms=1000 * wall))
    sim.close()
    stalled = sum(first.stalled(i) for i in range(first.n))
    return dict(report=first.report, audit_report=first.audit.report, log_overflows=int(rep["log_overflows"]),
                stalled_instances=int(stalled), rows=rows)


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
    cmd = [sys.executable, os.path.abspath(__file__), "--child-audit", "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child run failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def bench_ab(args):
    """bench.py --gpus 1 --steps 20 --warmup 5 on the parent's library and on this one, one process per run, interleaved
    (parent, this, parent, this, ...), --bench-rounds runs each -> --bench-out"""
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5"]
    sides = dict(parent=[], this=[])
    for _ in range(args.bench_rounds):
        for side in ("parent", "this"):
            print(f"bench.py: {side}", file=sys.stderr, flush=True)
            env = dict(os.environ)
            if side == "parent":
                env.update(BFTSIM_TESTING="1", BFTSIM_LIB=os.path.abspath(args.parent_lib))
            r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
            if r.returncode != 0:
                raise SystemExit(f"bench.py ({side}) failed ({r.returncode}): {r.stderr[-2000:]}")
            sides[side].append(json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])["value"])
    med = lambda v: sorted(v)[len(v) // 2]
    out = dict(command=f"bench.py --gpus 1 --steps 20 --warmup 5, the parent commit's libbftsim and this one, one process "
                       f"per run, interleaved, {args.bench_rounds} runs each (scripts/timeline_bench.py --bench-rounds)",
               unit="instance-rounds/s", parent=sides["parent"], this=sides["this"],
               parent_median=med(sides["parent"]), parent_minmax=[min(sides["parent"]), max(sides["parent"])],
               this_median=med(sides["this"]), this_minmax=[min(sides["this"]), max(sides["this"])])
    out["this_median_inside_parent_minmax"] = bool(out["parent_minmax"][0] <= out["this_median"] <= out["parent_minmax"][1])
    os.makedirs(os.path.dirname(os.path.abspath(args.bench_out)), exist_ok=True)
    with open(args.bench_out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--rounds", type=int, default=3, help="child processes per library under --parent-lib")
    ap.add_argument("--bench-rounds", type=int, default=0, help="bench.py runs per library under --parent-lib (0: none)")
    ap.add_argument("--bench-out", default=os.path.join(ROOT, "profiles", "r14", "timeline", "bench_ab.json"))
    ap.add_argument("--child-audit", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r14", "timeline", "timeline_bench.json"))
    args = ap.parse_args()
    if args.child_audit:
        print(json.dumps(measure_audit(SHAPES["twins"], args.repeats)))
        return
    keys = ("audit_ms", "walk_ms", "rows_ms", "copy_ms", "decode_ms", "recover_ms", "tally_ms", "wall_ms")
    out = dict(note=f"cfg3 (21 Byzantine of 64), twins on, one GPU; 1 warm-up + {args.repeats} repeats; tally_ms is the "
                    "observer's classify + tally", shapes={})
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def dump():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    for name, shape in SHAPES.items():
        m = measure(shape, args.repeats)
        s = summary(m["rows"], keys)
        own = s["walk_ms_median"] + s["rows_ms_median"]
        s["timeline_over_tally"] = own / s["tally_ms_median"]
        s["timeline_share_of_device"] = own / (s["audit_ms_median"] + own)
        out["shapes"][name] = dict(shape=shape, report=m["report"], audit_report=m["audit_report"],
                                   log_overflows=m["log_overflows"], stalled_instances=m["stalled_instances"], library=s)
        dump()                                             # the chronicler's timings are kept whatever comes after
    if args.parent_lib:                                    # fresh processes: a binding loads one library
        akeys = ("decode_ms", "recover_ms", "tally_ms")
        sides = dict(parent=[], this=[])
        for _ in range(args.rounds):                       # interleaved: parent, this, parent, this, ...
            for side, path in (("parent", args.parent_lib), ("this", None)):
                print(f"audit_last_trace: {side}", file=sys.stderr, flush=True)
                c = child_audit(args, path)
                assert c["audit_report"] == out["shapes"]["twins"]["audit_report"], f"{side}: the observer's report differs"
                sides[side] += c["rows"]
        ab = {side: summary(rows, akeys) for side, rows in sides.items()}
        ab["this_inside_parent_minmax"] = {k: bool(ab["parent"][k + "_minmax"][0] <= ab["this"][k + "_median"] <=
                                                   ab["parent"][k + "_minmax"][1]) for k in akeys}
        out["audit_last_trace_ab"] = ab
        dump()
        if args.bench_rounds:
            out["bench_ab"] = bench_ab(args)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
