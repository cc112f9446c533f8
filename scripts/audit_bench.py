#!/usr/bin/env python3
"""Measures the observer (bftsim_audit_last_trace, SPEC.md §11c) on one GPU at the trace export's
shape: cfg3, 1,024 instances x 10 heights, every broadcast signed. After one launch + bftsim_crypto_verify (keep on)
it audits the whole kept trace 1 + 5 times and records, from the library's HIP events (bftsim_audit_last_ms), the
decode kernel, the recoveries, classification + tally and the copies; the frame rate; the share of
decode + classify + tally in the total; and the wall time of the Python receiver (bftsim.trace.audit) on a 1/64
sample of the same trace. --alt-lib: the same measurement in a child process on another build of libbftsim (the
scratch build whose decode kernel staged a wave's 64 frames in LDS), recorded side by side as `alt_lib`.

    python scripts/audit_bench.py [--instances 1024] [--heights 10] [--repeats 5] [--alt-lib LIB.so] [--out FILE.json]
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


def measure(args):
    from bftsim.configs import cfg3
    from bftsim.crypto import synthetic_secrets, keyed_config
    from bftsim.runtime import Simulator, keccak256
    import secp256k1_ref as S                              # the addresses on the CPU: libbftsim is all this needs
    sec = synthetic_secrets(64, 3)
    cfg, secrets = keyed_config(cfg3(heights=args.heights), sec, [S.address(S.pubkey(k), keccak256) for k in sec])
    sim = Simulator(cfg)
    sim.set_crypto(secrets, (), 24_576)
    sim.set_trace_keep(True)
    sim.prepare(args.instances)
    sim.launch(0)
    sim.sync()
    rep = sim.crypto_verify()
    assert rep["mismatches"] == 0 and rep["seal_errors"] == 0, rep
    rows, first = [], None
    for r in range(1 + args.repeats):                      # the first is the warm-up
        t0 = time.perf_counter()
        a = sim.audit_last_trace()
        wall = time.perf_counter() - t0
        if first is None:
            first = a
        assert a.report == first.report
        if r:
            d, rc, t, c = sim.audit_ms()
            rows.append(dict(decode_ms=d, recover_ms=rc, tally_ms=t, copy_ms=c, wall_ms=1000 * wall))
    assert first.report["ok"] == first.report["frames"] == rep["messages"] and first.report["conflicts"] == 0
    res = sim.fetch()
    from bftsim.trace import compare
    cmp_ = {k: int(v.sum()) for k, v in compare(first, res).items()}
    out = dict(report=first.report, compare=cmp_, committed_heights=int(res["committed_height"].sum()), rows=rows)
    if args.sample:                                        # the Python receiver on the first instances / 64
        from bftsim.sig import Signer
        from bftsim.trace import audit
        from bftsim.wire import Codec
        tr = sim.export_trace(0, max(1, args.instances // 64))
        cd, sg = Codec(), Signer()
        audit(tr, cfg.addresses, cd, sg)                   # warm-up
        t0 = time.perf_counter()
        who = audit(tr, cfg.addresses, cd, sg)
        out["python_audit"] = dict(frames=len(tr), wall_ms=1000 * (time.perf_counter() - t0), recovered=int((who >= 0).sum()))
        cd.close()
        sg.close()
    sim.close()
    return out


def summary(m):
    def med(k):
        v = sorted(r[k] for r in m["rows"])
        return v[len(v) // 2]
    frames = m["report"]["frames"]
    d, rc, t = med("decode_ms"), med("recover_ms"), med("tally_ms")
    s = dict(decode_ms=[round(r["decode_ms"], 4) for r in m["rows"]], recover_ms=[round(r["recover_ms"], 3) for r in m["rows"]],
             tally_ms=[round(r["tally_ms"], 4) for r in m["rows"]], copy_ms=[round(r["copy_ms"], 3) for r in m["rows"]],
             wall_ms=[round(r["wall_ms"], 2) for r in m["rows"]], decode_ms_median=d, recover_ms_median=rc, tally_ms_median=t,
             frames_per_s=frames / ((d + rc + t) * 1e-3), decode_frames_per_s=frames / (d * 1e-3),
             recoveries_per_s=m["report"]["recoveries"] / (rc * 1e-3), own_share=(d + t) / (d + rc + t))
    if "python_audit" in m:
        p = m["python_audit"]
        s["python_audit"] = dict(p, frames_per_s=p["frames"] / (p["wall_ms"] * 1e-3))
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--instances", type=int, default=1024)
    ap.add_argument("--heights", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--alt-lib", default=None)
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r08", "trace_audit", "audit_bench.json"))
    args = ap.parse_args()
    args.sample = not args.child
    m = measure(args)
    if args.child:
        print(json.dumps(m))
        return
    out = dict(shape=f"cfg3, {args.instances} instances x {args.heights} heights, one GPU; 1 warm-up + {args.repeats} repeats",
               report=m["report"], compare=m["compare"], committed_heights=m["committed_heights"], library=summary(m))
    if args.alt_lib:                                       # a fresh process: the binding loads one library
        env = dict(os.environ, BFTSIM_TESTING="1", BFTSIM_LIB=os.path.abspath(args.alt_lib))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--instances", str(args.instances),
                            "--heights", str(args.heights), "--repeats", str(args.repeats)], env=env, capture_output=True,
                           text=True, timeout=900)
        if r.returncode != 0:
            raise SystemExit(f"alt-lib run failed ({r.returncode}): {r.stderr[-2000:]}")
        alt = json.loads(r.stdout.strip().splitlines()[-1])
        assert alt["report"] == m["report"], "the two decode forms disagree"
        out["alt_lib"] = summary(alt)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
