"""Do the slots' one-launch steps queue for places to run?  (engine options step_defer 2 + trace)

    python tools/slot_spread.py [--slots 4] [--batches 48] [--reps 5] [--config 3]

K engines, each on its own dispatch queue, take the batches in turn as the group's slots do (two key
buffers per slot in alternation, batch times cycling as bench.py's), with the phase trace on.  After
the queues have run — without a flush, so the last launch of every slot that carried a K1 is a
steady-state one — each engine's trace holds that launch's K1 and K3s stamps.  Printed per slot,
as medians over the repetitions (us): the spread between the first and the last K1 workgroup's
start stamp (a launch resident at once starts all its workgroups within the dispatcher's time,
one that waits for places spreads them over the span of what it waits for), the same for K3s (of
the launch before: the trace keeps each body's last), and K1's span first start -> last end.
One slot alone (--slots 1) is the comparison.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "crane-scheduler_amd")]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import crane_dyn as cd  # noqa: E402
from crane_dyn import synth  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--config", type=int, default=3)
ap.add_argument("--slots", type=int, default=4)
ap.add_argument("--batches", type=int, default=48)
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--now-cycle", type=int, default=6)
args = ap.parse_args()
dev = torch.device("cuda", 0)
spec = cd.default_policy_spec()
cfg = synth.CONFIGS[args.config]
N, P, B = cfg["nodes"], cfg["pods"], cfg["bindings"]
c = synth.make_cluster(spec, N, P, n_bindings=B, seed=20250215 + args.config * 1000)
c.now, c.ds = synth.make_pods(P, seed=20250215 + args.config)
K = args.slots
engs, qs = [], []
for _ in range(K):
    e = cd.Engine(cd.Policy(spec), 0)
    e.set_option("step_defer", 2)
    val, ts, _ = c.rows(e.metric_names)
    e.upload_nodes(val, ts, c.hv, c.hv_ts)
    e.upload_bindings(c.b_node, c.b_ts)
    engs.append(e)
    qs.append(cd.Queue(0))
step = int(c.now[1] - c.now[0])
span = int(c.now[-1] - c.now[0]) + step
now0 = int(c.now[0])
nows = [now0 + j * span for j in range(args.now_cycle)]
d_now = [torch.from_numpy(c.now + j * span).to(dev) for j in range(args.now_cycle)]
d_flags = torch.from_numpy(c.ds).to(dev)
keys = [[torch.empty(P, dtype=torch.int64, device=dev) for _ in range(2)] for _ in range(K)]
torch.cuda.synchronize()
nk1 = -(-N // 256)


def run(nb):
    for i in range(nb):
        s, j = i % K, i % args.now_cycle
        engs[s].step_keys_queue(nows[j], nows[j], d_now[j], d_flags, keys[s][(i // K) % 2], qs[s])
    for q in qs:
        q.wait()


def drain():
    for e in engs:
        e.step_flush()
    for q in qs:
        q.wait()


run(args.batches)  # warm-up: allocations, the anchors
drain()
k1_spread, k1_span, k3_spread, packets = [[] for _ in range(K)], [[] for _ in range(K)], [[] for _ in range(K)], []
for _ in range(args.reps):
    for e in engs:
        e.set_option("trace", 1)  # (clears the stamps)
    before = [q.packets() for q in qs]
    run(args.batches)
    packets.append([q.packets() - b for q, b in zip(qs, before)])
    for s, e in enumerate(engs):
        t = e.debug_trace(1, nk1).astype(np.int64)
        t = t[t[:, 0] > 0]
        if len(t):
            k1_spread[s].append((t[:, 0].max() - t[:, 0].min()) / 100.0)
            k1_span[s].append((t[:, 4].max() - t[:, 0].min()) / 100.0)
        t = e.debug_trace(2, 4096).astype(np.int64)
        t = t[t[:, 0] > 0]
        if len(t):
            k3_spread[s].append((t[:, 0].max() - t[:, 0].min()) / 100.0)
    drain()
med = lambda xs: [round(float(np.median(x)), 2) if len(x) else None for x in xs]  # noqa: E731
print(json.dumps({"config": args.config, "slots": K, "batches": args.batches, "reps": args.reps, "unit": "us",
                  "k1_workgroups": nk1, "packets_per_rep": packets[-1],
                  "k1_start_spread": med(k1_spread), "k1_start_spread_all": [[round(v, 2) for v in x] for x in k1_spread],
                  "k1_span": med(k1_span), "k3s_start_spread": med(k3_spread)}))
for e in engs:
    e.close()
for q in qs:
    q.close()
