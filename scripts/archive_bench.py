#!/usr/bin/env python3
"""Measures the archiver (bftsim_archive_last_trace, SPEC.md §11e) on one GPU: cfg3's shape with
byz_count = 0 (N = 64), 1,024 instances x 10 heights, every broadcast signed. After one launch + bftsim_crypto_verify
(keep on) it archives the whole kept trace 1 + 5 times and records, from the library's HIP events
(bftsim_archive_last_ms and bftsim_audit_last_ms of the same call), the observer's passes, the pick kernel, the
emit + heights kernels and the copies; pick + emit against the observer's classify + tally and against the whole
device time; and the importer's verdict on the archived ledger. --alt-lib: the same measurement in a child process on
another build of libbftsim (the scratch build with a lane-per-header serial emitter), recorded side by side as
`alt_lib`. --kernel-stats: one more child under `rocprofv3 --kernel-trace --stats`, its per-kernel totals recorded as
`kernel_stats`.

    python scripts/archive_bench.py [--instances 1024] [--heights 10] [--repeats 5] [--alt-lib LIB.so] [--kernel-stats]
                                    [--out FILE.json]
"""
import argparse
import csv
import dataclasses
import glob
import json
import os
import subprocess
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "consensus-rs_amd"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))


def measure(args):
    from bftsim.configs import cfg3
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.runtime import Simulator, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(64, 3)
    cfg, secrets = keyed_config(dataclasses.replace(cfg3(heights=args.heights), byz_count=0, name="cfg3-honest"), sec,
                                [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), 24_576)
    sim.set_trace_keep(True)
    sim.prepare(args.instances)
    sim.launch(0)
    sim.sync()
    rep = sim.crypto_verify()
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0, rep
    rows, first, ledger = [], None, None
    for r in range(1 + args.repeats):                      # the first is the warm-up
        t0 = time.perf_counter()
        ledger, a = sim.archive_last_trace()
        wall = time.perf_counter() - t0
        if first is None:
            first = a
        assert a.report == first.report and a.audit.report == first.audit.report
        if r:
            au, pk, em, cp = sim.archive_ms()
            d, rc, t, _ = sim.audit_ms()
            rows.append(dict(audit_ms=au, pick_ms=pk, emit_ms=em, copy_ms=cp, decode_ms=d, recover_ms=rc, tally_ms=t,
                             wall_ms=1000 * wall))
    res = sim.fetch()
    committed = int(res["committed_height"].sum())
    assert first.report["headers"] == first.audit.report["certified"] and first.report["by_status"][2] == 0
    verdict = sim.verify_ledger(ledger)
    out = dict(report=first.report, audit_report=first.audit.report, committed_heights=committed,
               archived_as_run=bool((first.archived_height == res["committed_height"]).all()),
               import_report=verdict.report, slot_bytes=int(ledger[2]), ledger_bytes=int(ledger[1].sum()), rows=rows)
    sim.close()
    return out


def summary(m):
    def med(k):
        v = sorted(r[k] for r in m["rows"])
        return v[len(v) // 2]
    keys = ("audit_ms", "pick_ms", "emit_ms", "copy_ms", "decode_ms", "recover_ms", "tally_ms", "wall_ms")
    s = {k: [round(r[k], 4) for r in m["rows"]] for k in keys}
    s.update({k + "_median": med(k) for k in keys})
    own = med("pick_ms") + med("emit_ms")
    s["pick_emit_ms"] = own
    s["pick_emit_over_tally"] = own / med("tally_ms")
    s["pick_emit_share_of_device"] = own / (med("audit_ms") + own)
    s["non_crypto_share_of_device"] = (med("decode_ms") + med("tally_ms") + own) / (med("audit_ms") + own)
    s["headers_per_s"] = m["report"]["headers"] / (own * 1e-3)
    return s


def child(args, extra_env=None, wrap=()):
    env = dict(os.environ, **(extra_env or {}))
    cmd = list(wrap) + [sys.executable, os.path.abspath(__file__), "--child", "--instances", str(args.instances), "--heights",
                        str(args.heights), "--repeats", str(args.repeats)]
    r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        raise SystemExit(f"child run failed ({r.returncode}): {r.stderr[-2000:]}")
    return json.loads([ln for ln in r.stdout.strip().splitlines() if ln.startswith("{")][-1])


def kernel_stats(args):
    """the per-kernel totals of one whole child run under the profiler (launch, crypto_verify and 1 + repeats archives)"""
    with tempfile.TemporaryDirectory() as d:
        child(args, wrap=("rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "run", "--"))
        files = glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True)
        if not files:
            raise SystemExit("rocprofv3 wrote no kernel_stats.csv")
        with open(files[0]) as f:
            rows = list(csv.DictReader(f))
    try:
        out = [dict(name=r["Name"].split("(")[0], calls=int(r["Calls"]), total_ms=int(r["TotalDurationNs"]) / 1e6,
                    avg_us=float(r["AverageNs"]) / 1e3, percent=float(r["Percentage"])) for r in rows]
    except (KeyError, ValueError):                         # another profiler version's columns: keep the rows as they are
        return rows[:24]
    return sorted(out, key=lambda r: -r["total_ms"])[:24]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--heights", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--kernel-stats", action="store_true")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r11", "archive", "archive_bench.json"))
    args = ap.parse_args()
    m = measure(args)
    if args.child:
        print(json.dumps(m))
        return
    out = dict(shape=f"cfg3 with byz_count = 0, {args.instances} instances x {args.heights} heights, one GPU; "
                     f"1 warm-up + {args.repeats} repeats",
               report=m["report"], audit_report=m["audit_report"], committed_heights=m["committed_heights"],
               archived_as_run=m["archived_as_run"], import_report=m["import_report"], slot_bytes=m["slot_bytes"],
               ledger_bytes=m["ledger_bytes"], library=summary(m))
    if args.alt_lib:                                       # a fresh process: the binding loads one library
        alt = child(args, dict(BFTSIM_TESTING="1", BFTSIM_LIB=os.path.abspath(args.alt_lib)))
        assert alt["report"] == m["report"] and alt["import_report"] == m["import_report"], "the two emitters disagree"
        out["alt_lib"] = summary(alt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)

    def dump():
        with open(args.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
    dump()                                                 # the timings are kept whatever the profiler pass does
    if args.kernel_stats:
        out["kernel_stats"] = kernel_stats(args)
        dump()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
