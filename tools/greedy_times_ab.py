#!/usr/bin/env python3
"""Same-box measurement of the sequential greedy at per-pod times (greedy_times.hip).

  (a) equal times: crane_dyn_greedy_times with every pod at one `now` against the sequential
      kernel of crane_dyn_greedy ("greedy_form" 1) on configs 3 and 5 — the same placements, so
      the difference is what the per-pod head checks and event-group loads cost.
  (b) advancing times: config 3's own pod times (1 ms apart, 10 s span) and config-4-like times on
      one device (100k nodes x 100k pods, 100 s span): per-pod time, the events by class, the
      event-building kernels.

Per route: the engine's own kernel times (crane_dyn_set_profiling / crane_dyn_stage_times, the
dispatches' begin -> end) and the whole synchronous call on the host clock, median and minimum
over --reps after --warmup.  All routes run in this one process, alternating.

  python tools/greedy_times_ab.py --out profiles/ab/greedy_times.txt
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crane-scheduler_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

NS = 10**9


def event_counts(np, spec, c, now, chosen):
    """Events of a run by class: record (a node's expiries inside the batch), log (a log binding
    leaves a window), placements of the batch that left a window before the last pod."""
    period = dict(spec["syncPolicy"])
    row = {n: i for i, n in enumerate(c.metric_names)}
    never = np.iinfo(np.int64).min

    def expiry(name, sel):
        m = row[name]
        return np.where((c.ok[m] == 1) & ~(c.val[m] < 0.0) & sel(c.val[m]), c.ts[m] + period[name] + 300 * NS, never)

    e_fail = np.full(c.n_nodes, never, np.int64)
    for name, lim in spec["predicate"]:
        e_fail = np.maximum(e_fail, expiry(name, lambda v, lim=lim: v > lim))
    exp = [e_fail] + [expiry(name, lambda v: v == v) for name, _ in spec["priority"]]
    rec = sum(int(((now[0] < e) & ~(now[-1] < e)).sum()) for e in exp)
    unix = now // NS
    log = left = 0
    for tr, _ in spec["hotValue"]:
        t = int(tr / 1e9)
        log += int(((c.b_ts > unix[0] - t) & ~(c.b_ts > unix[-1] - t)).sum())
        if t > 0:
            left += int(((unix <= unix[-1] - t) & (chosen >= 0)).sum())
    return rec, log, left


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import crane_dyn as cd
    from crane_dyn import synth

    if not torch.cuda.is_available():
        sys.exit("greedy_times_ab: no GPU (nothing is measured without one)")
    spec = cd.default_policy_spec()
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# sequential greedy at per-pod times, {torch.cuda.get_device_name(0)}; median (min) of {args.reps} "
        f"after {args.warmup} warm-up calls; us/pod = the run kernel's time / pods")

    def engine(c):
        eng = cd.Engine(cd.Policy(spec), 0)
        val, ts, _ = c.rows(eng.metric_names)
        eng.upload_nodes(val, ts, c.hv, c.hv_ts)
        eng.upload_bindings(c.b_node, c.b_ts)
        eng.set_option("greedy_form", 1)
        eng.set_profiling(True)
        return eng

    def timed(eng, call, reps):
        """[(host ms, {kernel: ms})] per repetition, and the last result"""
        out, res = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = call()
            ms = (time.perf_counter() - t0) * 1e3
            k = {}
            for name, t in eng.stage_times():
                k[name] = k.get(name, 0.0) + t
            out.append((ms, k))
        return out, res

    def med(rows, key):
        xs = [k.get(key, 0.0) for _, k in rows] if key else [ms for ms, _ in rows]
        return statistics.median(xs), min(xs)

    def fmt(x):
        return f"{x[0]:.3f} ({x[1]:.3f})"

    def report(label, P, rows, run):
        r = med(rows, run)
        s = f"{label}: {run} {fmt(r)} ms = {r[0] * 1e3 / P:.3f} ({r[1] * 1e3 / P:.3f}) us/pod; call {fmt(med(rows, None))} ms"
        for k in ("greedy_ev_count", "greedy_ev_scan", "greedy_ev_fill"):
            if any(k in kk for _, kk in rows):
                s += f"; {k[7:]} {fmt(med(rows, k))}"
        say(s)
        return r

    shapes = {"config 3": (3, 20250215 + 3000), "config 5": (5, 20255215)}
    clusters = {}
    for label, (cfg, seed) in shapes.items():
        g = synth.CONFIGS[cfg]
        clusters[label] = synth.make_cluster(spec, g["nodes"], g["pods"], n_bindings=g["bindings"], seed=seed)

    # ---- (a) equal times against the sequential kernel of crane_dyn_greedy
    for label, c in clusters.items():
        P = len(c.now)
        now = int(synth.NOW0_NS)
        same = np.full(P, now, np.int64)
        eng = engine(c)
        seq = lambda: eng.greedy(P, now, c.ds)  # noqa: E731
        tim = lambda: eng.greedy_times(same, c.ds)  # noqa: E731
        _, a = timed(eng, seq, args.warmup)
        _, b = timed(eng, tim, args.warmup)
        if not np.array_equal(a, b):
            sys.exit(f"greedy_times_ab: {label}: equal times differ from crane_dyn_greedy")
        ra, rb = [], []
        for _ in range(3):  # the routes alternate: three rounds of reps / 3
            per = max(1, args.reps // 3)
            ra += timed(eng, seq, per)[0]
            rb += timed(eng, tim, per)[0]
        say(f"[a] {label}: {c.n_nodes} nodes x {P} pods, {len(c.b_node)} bindings, equal times; placements equal")
        x = report(f"[a] {label} greedy (greedy_form 1)", P, ra, "greedy_run")
        y = report(f"[a] {label} greedy_times          ", P, rb, "greedy_run_times")
        say(f"[a] {label} run kernel ratio greedy_times / greedy: median {y[0] / x[0]:.3f}, min {y[1] / x[1]:.3f}")
        eng.close()

    # ---- (b) advancing times
    g4 = dict(nodes=100_000, pods=100_000, bindings=1_000_000)
    clusters["config-4-like, one device"] = synth.make_cluster(spec, g4["nodes"], g4["pods"], n_bindings=g4["bindings"],
                                                               seed=20250215 + 4000)
    for label in ("config 3", "config-4-like, one device"):
        c = clusters[label]
        P = len(c.now)
        now = int(synth.NOW0_NS) + np.arange(P, dtype=np.int64) * 1_000_000
        eng = engine(c)
        tim = lambda: eng.greedy_times(now, c.ds)  # noqa: E731
        timed(eng, tim, args.warmup)
        rows, ch = timed(eng, tim, args.reps)
        rec, log, left = event_counts(np, spec, c, now, ch)
        say(f"[b] {label}: {c.n_nodes} nodes x {P} pods, {len(c.b_node)} bindings, 1 ms apart ({P / 1000:.0f} s span); "
            f"events: record {rec}, log {log}, own placements leaving {left}; placed {int((ch >= 0).sum())}, "
            f"distinct nodes {len(np.unique(ch))}")
        report(f"[b] {label} greedy_times", P, rows, "greedy_run_times")
        eng.close()

    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
