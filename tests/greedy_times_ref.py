"""Shared by test_greedy_times_model.py (CPU) and test_greedy_times_gpu.py: the reference of
crane_dyn_greedy_times composed from the committed oracle, the targeted cases, and a numpy model
of the kernels' event scheme.

The reference is the normative definition itself: pod p is the oracle's greedy loop of one pod at
now[p] over the uploaded log plus one binding {chosen[q], now[q] // 1e9} per earlier placement
(binding.go:81-97, node.go:113-121, plugins.go:91; time.Now() per pod).
"""
import functools

import numpy as np

import crane_dyn as cd
from crane_dyn import synth
from oracle import oracle as O

NS = 10**9
MIN = 60 * NS
T0 = int(synth.NOW0_NS) + 1234567


def ref(spec, c, now, ds):
    bn, bt = list(c.b_node), list(c.b_ts)
    ts = np.where(c.ok == 1, c.ts, 0)
    out = []
    for p in range(len(now)):
        ch = O.greedy(spec, c.metric_names, c.ok, c.val, ts, np.array(bn, np.int32), np.array(bt, np.int64),
                      int(now[p]), 1, ds[p:p + 1])[0]
        out.append(ch)
        if ch >= 0:
            bn.append(int(ch))
            bt.append(int(now[p]) // NS)
    return np.array(out, np.int64)


def frozen(spec, c, now, ds):
    """crane_dyn_greedy's answer: every pod at now[0]."""
    return O.greedy(spec, c.metric_names, c.ok, c.val, np.where(c.ok == 1, c.ts, 0), c.b_node, c.b_ts, int(now[0]),
                    len(now), ds)


def times(P, step_ns):
    return T0 + np.arange(P, dtype=np.int64) * int(step_ns)


# name -> (hotValue or None = the default, N, P, B, step ns, seed, ds_frac or None, fresh annotations)
CASES = {
    "expiries_only": ([], 1000, 256, 0, NS // 2, 31, 0.3, False),
    "expiries_feedback": (None, 300, 200, 0, NS // 4, 51, 0.1, False),
    "log_leaves": (None, 300, 160, 3000, NS // 4, 12, None, True),
    "placements_leave": (None, 40, 256, 0, NS // 2, 13, None, True),
    "everything": (None, 64, 200, 1000, 2 * NS, 14, None, False),
    "many_events_per_pod": (None, 64, 100, 20000, 4 * NS, 71, None, False),
    "three_levels": (None, 4097, 200, 50000, NS, 74, None, False),
    "global_leaves": (None, 200000, 48, 100000, NS, 76, None, False),
    "four_levels": (None, 262145, 48, 100000, NS, 77, None, False),
    "daemonset_mix": (None, 3000, 300, 30000, NS // 2, 75, 0.3, False),
    "odd_windows": ([(0, 1), (-60 * MIN, 2), (30 * MIN, -3)], 300, 200, 5000, 2 * NS, 72, None, False),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """(spec, cluster, now, ds, ref, frozen) of a targeted case; computed once per process."""
    hot, N, P, B, step, seed, ds_frac, fresh = CASES[name]
    spec = cd.default_policy_spec()
    if hot is not None:
        spec = dict(spec, hotValue=hot)
    kw = {} if ds_frac is None else {"ds_frac": ds_frac}
    if fresh:
        kw["invalid"] = False
    c = synth.make_cluster(spec, N, P, n_bindings=B, seed=seed, **kw)
    if fresh:
        c.ts[:] = synth.NOW0_NS  # nothing expires inside the batch
    now = times(P, step)
    want, froz = ref(spec, c, now, c.ds), frozen(spec, c, now, c.ds)
    for a in (now, want, froz):
        a.setflags(write=False)
    return spec, c, now, c.ds, want, froz


# ---------------------------------------------------------------------------------------------
# The event scheme of csrc/greedy_times.hip in numpy: node records, the state at pod 0, the events
# as a CSR by the first pod that sees them, per-window heads over chosen[], and the recompute of
# touched nodes only.  Every other node keeps the score computed at an earlier time.

def _go_int(x):
    if not (-9223372036854775808.0 <= x < 9223372036854775808.0):  # NaN too
        return -2**63
    return int(x)


def _trunc_div(c, k):
    q = abs(c) // abs(k)
    return q if (c >= 0) == (k > 0) else -q


def records(spec, c):
    """e_fail [N], e_prio [K][N], term [K][N], wsum (stats.go:42-48, 89, 94-150)."""
    period = dict(spec["syncPolicy"])
    row = {n: i for i, n in enumerate(c.metric_names)}
    N = c.n_nodes
    never = np.full(N, synth.TS_INVALID, np.int64)
    e_fail = never.copy()
    for name, lim in spec["predicate"]:
        if period.get(name, 0) <= 0 or name not in row or lim == 0:
            continue
        m = row[name]
        usable = (c.ok[m] == 1) & ~(c.val[m] < 0.0)
        over = usable & (c.val[m] > lim)
        e_fail = np.maximum(e_fail, np.where(over, c.ts[m] + period[name] + 5 * MIN, never))
    e_prio, term, wsum = [], [], 0.0
    for name, w in spec["priority"]:
        wsum += w
        if period.get(name, 0) <= 0 or name not in row:
            continue
        m = row[name]
        usable = (c.ok[m] == 1) & ~(c.val[m] < 0.0)
        e_prio.append(np.where(usable, c.ts[m] + period[name] + 5 * MIN, never))
        term.append(np.where(usable, ((1.0 - c.val[m]) * w) * 100.0, 0.0))
    return e_fail, e_prio, term, wsum


def model(spec, c, now, ds):
    N, P = c.n_nodes, len(now)
    e_fail, e_prio, term, wsum = records(spec, c)
    noprio = len(spec["priority"]) == 0
    hot = spec["hotValue"]
    trs = [int(tr / 1e9) for tr, _ in hot]  # int64(d.Seconds())
    unix = now // NS
    inc = [t > 0 for t in trs]  # a binding stamped unix_p is counted at pod p

    def base_at(n, t):
        if noprio:
            return 0
        s = 0.0
        for k in range(len(term)):
            if t < e_prio[k][n]:
                s += term[k][n]
        return _go_int(s / wsum)

    def pen(n):
        v = sum(_trunc_div(int(cnt[w][n]), hot[w][1]) for w in range(len(hot)))
        return 0 if v < 0 else _go_int(float(v) * 10.0)

    def score(n):
        return max(0, min(100, base[n] - pen(n)))

    # the state at pod 0
    live = (c.b_node >= 0) & (c.b_node < N)
    bn, bt = c.b_node[live].astype(np.int64), c.b_ts[live]
    cnt = [np.bincount(bn[bt > unix[0] - t], minlength=N).astype(np.int64) for t in trs]
    base = [base_at(n, now[0]) for n in range(N)]
    feas = ~(now[0] < e_fail)
    sc = np.array([score(n) for n in range(N)], np.int64)
    # the events, grouped by first pod: (node, window or -1)
    groups = [[] for _ in range(P)]
    for e in [e_fail] + e_prio:
        hit = np.flatnonzero((now[0] < e) & ~(now[P - 1] < e))
        for n, p in zip(hit, np.searchsorted(now, e[hit], side="left")):  # first p with !(now_p < e)
            groups[p].append((int(n), -1))
    for w, t in enumerate(trs):
        hit = np.flatnonzero((bt > unix[0] - t) & ~(bt > unix[P - 1] - t))
        for n, p in zip(bn[hit], np.searchsorted(unix, bt[hit] + t, side="left")):  # first p with ts <= unix_p - trs
            groups[p].append((int(n), w))
    head = [0] * len(hot)
    chosen = np.full(P, -1, np.int64)
    recomputed = 0
    for p in range(P):
        touched = set()
        for w, t in enumerate(trs):
            while inc[w] and head[w] < p and unix[head[w]] <= unix[p] - t:
                if chosen[head[w]] >= 0:
                    cnt[w][chosen[head[w]]] -= 1
                    touched.add(int(chosen[head[w]]))
                head[w] += 1
        for n, w in groups[p][::-1]:  # (any order)
            if w >= 0:
                cnt[w][n] -= 1
            touched.add(n)
        for n in touched:
            base[n] = base_at(n, now[p])
            feas[n] = not (now[p] < e_fail[n])
            sc[n] = score(n)
        recomputed += len(touched)
        cand = sc if ds[p] else np.where(feas, sc, -1)
        best = int(np.argmax(cand))  # the first maximum: lowest index on ties
        if cand[best] < 0:
            continue
        chosen[p] = best
        for w in range(len(hot)):
            cnt[w][best] += 1 if inc[w] else 0
        sc[best] = score(best)
    assert min(int(x.min()) for x in cnt) >= 0 if cnt else True
    return chosen, recomputed, sum(len(g) for g in groups)
