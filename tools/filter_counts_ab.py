#!/usr/bin/env python3
"""Same-box comparison of the two routes to the filter diagnosis of a pod batch:

  counts  crane_dyn_filter_counts_async (diagnose.hip), swept over the "diag_slices" option;
  matrix  crane_dyn_eval_matrix_async writing the P x N int8 first-fail matrix only, then a torch
          histogram of it (one compare + row sum per column) — the only route before that kernel.

Per route: the engine's own kernel times (crane_dyn_set_profiling / crane_dyn_stage_times, the
dispatch's begin -> end) and the whole call between two events on one stream (with the output's
zeroing, the histogram), median and minimum over --reps after --warmup.  Both routes run in this
one process, alternating, and their rows must be equal.  Default: config 3 (100k nodes x 10k pods,
the bench's seeded single-box cluster), pod times in queue order and shuffled.

  python tools/filter_counts_ab.py --out profiles/ab/filter_counts.txt
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "crane-scheduler_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nodes", type=int, default=100_000)
    ap.add_argument("--pods", type=int, default=10_000)
    ap.add_argument("--slices", type=int, nargs="*", default=[0, 1, 8, 32, 128])
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    args = ap.parse_args()

    import numpy as np
    import torch

    import crane_dyn as cd
    from crane_dyn import synth

    if not torch.cuda.is_available():
        sys.exit("filter_counts_ab: no GPU (nothing is measured without one)")
    dev = torch.device("cuda", 0)
    spec = cd.default_policy_spec()
    N, P = args.nodes, args.pods
    c = synth.make_cluster(spec, N, P, seed=20250215 + 3000)
    c.now, c.ds = synth.make_pods(P, seed=20250215 + 3)
    eng = cd.Engine(cd.Policy(spec), 0)
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts)
    n_pred = eng.n_pred
    st = torch.cuda.Stream(dev)
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    say(f"# filter diagnosis, {N} nodes x {P} pods, {n_pred} predicates, {torch.cuda.get_device_name(0)}; "
        f"ms, median (min) of {args.reps} after {args.warmup} warm-up calls")
    say(f"# output {P * (n_pred + 1) * 4 / 1e3:.0f} KB per batch; first-fail matrix {P * N / 1e6:.0f} MB")

    def timed(call, reps):
        """[(kernel ms by name, call ms)] per repetition: events on `st` around the call."""
        out = []
        for _ in range(reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            with torch.cuda.stream(st):
                a.record()
                call()
                b.record()
            b.synchronize()
            k = {}
            for name, ms in eng.stage_times():
                k[name] = k.get(name, 0.0) + ms
            out.append((k, a.elapsed_time(b)))
        return out

    def summary(rows, kernel):
        ks = [r[0].get(kernel, float("nan")) for r in rows]
        cs = [r[1] for r in rows]
        return (f"kernel {statistics.median(ks):.4f} ({min(ks):.4f})  call {statistics.median(cs):.4f} ({min(cs):.4f})")

    d_flags = torch.from_numpy(c.ds).to(dev)
    d_counts = torch.empty((P, n_pred + 1), dtype=torch.int32, device=dev)
    d_ff = torch.empty((P, N), dtype=torch.int8, device=dev)
    hist = torch.empty((P, n_pred + 1), dtype=torch.int32, device=dev)
    eng.set_profiling(True)

    def matrix_route(d_now):
        eng.eval_matrix_async(d_now, d_flags, d_ff, None, stream=st.cuda_stream)
        for j in range(n_pred):
            hist[:, j] = (d_ff == j).sum(dim=1, dtype=torch.int32)
        hist[:, n_pred] = (d_ff < 0).sum(dim=1, dtype=torch.int32)

    orders = {"queue order": c.now, "shuffled": c.now[np.random.default_rng(9).permutation(P)]}
    for label, now in orders.items():
        d_now = torch.from_numpy(np.ascontiguousarray(now)).to(dev)
        torch.cuda.synchronize()
        timed(lambda: matrix_route(d_now), args.warmup)
        ref = hist.clone()
        res = {}
        for s in args.slices:  # warm up every form, and check it
            eng.set_option("diag_slices", s)
            timed(lambda: eng.filter_counts_async(d_now, d_flags, d_counts, stream=st.cuda_stream), args.warmup)
            if not torch.equal(d_counts, ref):
                sys.exit(f"filter_counts_ab: diag_slices {s} differs from the matrix route ({label})")
            res[s] = []
        mat = []
        for _ in range(3):  # the routes alternate: three rounds of reps / 3
            for s in args.slices:
                eng.set_option("diag_slices", s)
                res[s] += timed(lambda: eng.filter_counts_async(d_now, d_flags, d_counts, stream=st.cuda_stream),
                                max(1, args.reps // 3))
            mat += timed(lambda: matrix_route(d_now), max(1, args.reps // 3))
        say(f"[{label}] rows equal on both routes for diag_slices {args.slices}")
        for s in args.slices:
            say(f"[{label}] counts diag_slices={s:<4d} {summary(res[s], 'k_filter_counts')}")
        say(f"[{label}] matrix first-fail + histogram  {summary(mat, 'k3m_matrix')}")
    eng.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
