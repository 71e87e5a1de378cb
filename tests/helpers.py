"""Shared test helpers: run the HIP engine and the CPU oracle on the same inputs."""
import numpy as np

import crane_dyn as cd
from crane_dyn import synth
from oracle import oracle as O

SH = 8 * 3600


def engine_for(spec, cluster=None, device=0, opts=None):
    eng = cd.Engine(cd.Policy(spec), device)
    for k, v in (opts or {}).items():
        eng.set_option(k, v)
    if cluster is not None:
        val, ts, _ = cluster.rows(eng.metric_names)
        eng.upload_nodes(val, ts, cluster.hv, cluster.hv_ts)
    return eng


def oracle_soa(spec, c, now=None, ds=None, want_matrix=True, threads=8, hv_override=None):
    hv_ok = (c.hv_ts != synth.TS_INVALID).astype(np.uint8)
    hv, hv_ts = c.hv, c.hv_ts
    if hv_override is not None:
        hv, hv_ts = hv_override
        hv_ok = np.ones(len(hv), np.uint8)
    return O.eval_soa(spec, c.metric_names, c.ok, c.val, np.where(c.ok == 1, c.ts, 0), hv_ok, hv, hv_ts,
                      c.now if now is None else now, c.ds if ds is None else ds, threads=threads,
                      want_matrix=want_matrix)


# ---------------------------------------------------------------------------------------------
# Value-domain edges (tests/test_value_edges.py, tests/test_value_edges_gpu.py)
#
# synth.make_cluster writes usages in about [-1.2, 1.2] with five decimals and whole hot values
# 0..12.  The scheduler takes whatever strconv.ParseFloat accepts and the C ABI any double, so
# edge_cluster overwrites a seeded share of cells with the values below.  The reference's results
# on them (stats.go:51-76, 114-138, plugins.go:73-98): a NaN usage passes validation and the
# Filter and makes int(score / weight) INT64_MIN; +Inf and huge usages fail the Filter and
# overflow the same conversion; the int64 subtraction of int(hotValue * 10) wraps; NormalizeScore
# clamps what is left.
T0 = int(synth.NOW0_NS)
NS = 10**9
EDGE_SPAN = 60 * NS  # the pods' spread
INF, NAN = float("inf"), float("nan")


def edge_policy(kind):
    """default: the weights sum to 2.0 (the quotient is a multiply by 0.5); wsum21: they sum to
    2.1 (a true division); negw: one negative weight, sum 2.0 (a huge usage on it gives q >> 0)."""
    s = cd.default_policy_spec()
    if kind == "wsum21":
        s["priority"] = [(n, 0.6 if n == "mem_usage_max_avg_1d" else w) for n, w in s["priority"]]
    elif kind == "negw":  # (1.5 on the last metric keeps ordinary nodes' scores below 100)
        s["priority"] = [(n, {"cpu_usage_max_avg_1d": -0.5, "mem_usage_max_avg_1d": 1.5}.get(n, w)) for n, w in s["priority"]]
    else:
        assert kind == "default", kind
    return s


def _q_metric(spec):
    """The priority whose term reaches |q| = 2^31 at the smallest usage: a negative weight first
    (q > 0, the side where a penalty can bring the score back inside the clamp), then the largest."""
    k = min(range(len(spec["priority"])), key=lambda i: (spec["priority"][i][1] >= 0, -abs(spec["priority"][i][1]), -i))
    return spec["priority"][k]


def _q_usage(spec, d):
    """The usage of _q_metric at which its term alone gives |q| = 2^31 + d."""
    wsum = 0.0
    for _, w in spec["priority"]:
        wsum += w
    return 1.0 + (2.0**31 + d) * abs(wsum) / (100.0 * abs(_q_metric(spec)[1]))


def _limit_of(spec, metric):
    for n, lim in spec["predicate"]:
        if n == metric and lim != 0:
            return lim
    return None


# (class, value or function of (spec, metric), where): where = "any" metric, a "pred"icate's
# metric, or "q": _q_metric with every other metric of the node at 1.0 (terms exactly 0), so the
# quotient is that one term's.
USAGE_CLASSES = [
    ("NaN", NAN, "any"), ("+Inf", INF, "any"), ("1e300", 1e300, "any"), ("1e17", 1e17, "any"),
    ("2^31/50-", float(np.nextafter(2.0**31 / 50, 0)), "any"), ("2^31/50", 2.0**31 / 50, "any"),
    ("2^31/50+", float(np.nextafter(2.0**31 / 50, INF)), "any"),
    ("4.3e7", 4.3e7, "any"), ("4.4e7", 4.4e7, "any"),
    ("q=2^31-60", lambda s, m: _q_usage(s, -60), "q"), ("q=2^31", lambda s, m: _q_usage(s, 0), "q"),
    ("q=2^31+60", lambda s, m: _q_usage(s, 60), "q"),
    ("-0.0", -0.0, "any"), ("5e-324", 5e-324, "any"), ("1.0", 1.0, "any"),
    ("1.0+", float(np.nextafter(1.0, 2)), "any"),
    ("limit", lambda s, m: _limit_of(s, m), "pred"),
    ("limit+", lambda s, m: float(np.nextafter(_limit_of(s, m), INF)), "pred"),
    ("100.0", 100.0, "any"), ("-Inf", -INF, "any"), ("-1e300", -1e300, "any"),
    ("0x1p-2", 0.25, "any"), ("1_0.5", 10.5, "any"),
]
# (class, value, the value the liveness check replaces it by).  That is 0, except where the class
# itself scores as 0 (int(h * 10) = 0, or h < 0: rejected): no result can differ from 0's there,
# so those are replaced by 1 (a penalty of 10) — the node's hot value is then shown to matter.
HOT_CLASSES = [
    ("NaN", NAN, 0.0), ("+Inf", INF, 0.0), ("-Inf", -INF, 1.0), ("1e300", 1e300, 0.0), ("9.3e17", 9.3e17, 0.0),
    ("9.2e17", 9.2e17, 0.0), ("2^31/10-", float(np.nextafter(2.0**31 / 10, 0)), 0.0), ("2^31/10", 2.0**31 / 10, 0.0),
    ("2^31/10+", float(np.nextafter(2.0**31 / 10, INF)), 0.0), ("0.05", 0.05, 1.0), ("0.15", 0.15, 0.0),
    ("0.7", 0.7, 0.0), ("1.26", 1.26, 0.0), ("-0.0", -0.0, 1.0), ("-1.0", -1.0, 1.0), ("1e9", 1e9, 0.0),
]
# usage x hot-value classes that every cluster with hot values carries on one node each: a wrapped
# or huge base beside a wrapped, huge or small penalty, and base ~ penalty ~ 2^31
EDGE_COMBOS = [("NaN", "NaN"), ("NaN", "9.3e17"), ("NaN", "1.26"), ("1e17", "NaN"), ("1e17", "9.3e17"),
               ("1e17", "9.2e17"), ("1e17", "1.26"), ("1e300", "0.7"), ("+Inf", "+Inf"), ("q=2^31+60", "2^31/10"),
               ("q=2^31+60", "2^31/10-"), ("q=2^31", "2^31/10+"), ("q=2^31-60", "2^31/10")]


def edge_cluster(spec, n_nodes, n_pods, seed, share=0.35, hot=True, expire=0.5, n_bindings=0, bind_half=False,
                 ds_frac=0.1, span_ns=EDGE_SPAN, on_expiries=False):
    """synth.make_cluster(spec, n_nodes, n_pods, seed=seed) with a seeded `share` of its nodes
    turned into edge nodes: one usage cell, the hot-value annotation (hot=True), or both, take a
    value of USAGE_CLASSES / HOT_CLASSES in rotation (usages alternately on a predicate's metric
    and on a priority-only one), after one node per EDGE_COMBOS pair.  Half of the edge nodes get
    their other cells lightly loaded and fresh, so that they compete.  Stamps stay in synth's
    range.  expire: the share of edge cells whose expiry (stamp + period + 5 min; the hot value's
    stamp + 5 min) is placed inside the pods' range (tmin, tmax], to the ns — the usage cells of
    the lowest-indexed edge nodes, in index order (see below), hot values at random; a quarter of
    those nodes also wait behind an overloaded predicate that expires before.  bind_half: a few
    bindings of the last minutes on every other edge node.  on_expiries: the pods' times are
    those in-range expiries, 1 ns either side, and both ends of the range.
    Returns (cluster, labels): labels[n] is None or a dict u / metric / h (class names or None)
    and u_exp / h_exp (the in-range expiry or None)."""
    step = span_ns // (n_pods - 1) if n_pods > 1 else 0
    c = synth.make_cluster(spec, n_nodes, n_pods, n_bindings=n_bindings, seed=seed, ds_frac=ds_frac, pod_step_ns=step)
    rng = np.random.default_rng(seed + 77)
    names = c.metric_names
    dur = {n: p + 300 * NS for n, p in spec["syncPolicy"]}
    pred = [n for n, lim in spec["predicate"] if lim != 0]
    prio_only = [n for n, _ in spec["priority"] if n not in pred] or [n for n, _ in spec["priority"]]
    tmin, tmax = T0, T0 + step * (n_pods - 1)
    ucls = {k: (v, w) for k, v, w in USAGE_CLASSES}
    hcls = {k: v for k, v, _ in HOT_CLASSES}
    edge = rng.permutation(n_nodes)[:max(1, int(share * n_nodes))]
    labels = [None] * n_nodes
    plan = [(u, h) for u, h in EDGE_COMBOS] if hot else []
    iu = ih = 0
    while len(plan) < len(edge):
        mode = len(plan) % 3 if hot else 0
        u = h = None
        if mode != 1:
            u, iu = USAGE_CLASSES[iu % len(USAGE_CLASSES)][0], iu + 1
        if mode != 0:
            h, ih = HOT_CLASSES[ih % len(HOT_CLASSES)][0], ih + 1
        plan.append((u, h))

    def fresh():
        return (synth.NOW0 - int(rng.integers(1, 100))) * NS

    def in_range():
        return tmin + 1 + int(rng.integers(0, max(1, tmax - tmin))) if tmax > tmin and rng.random() < expire else None

    # The usage cells that expire in range do so in the order of their nodes' indices, within the
    # first 85 % of the range, and those that stay fresh sit on the highest indices: ties go to the
    # lowest index, so the nodes that score 100 hand the maximum on one after the other instead of
    # the first one keeping it for the whole batch.
    stepping = sorted(n for n, (u, _) in zip(edge.tolist(), plan) if u is not None)
    stepping = stepping[:int(expire * len(stepping))] if tmax > tmin else []
    at = np.sort(tmin + 1 + rng.integers(0, max(1, (tmax - tmin) * 85 // 100), len(stepping)))
    u_exp = dict(zip(stepping, at.tolist()))

    for i, (n, (u, h)) in enumerate(zip(edge.tolist(), plan)):
        lab = dict(u=u, metric=None, h=h, u_exp=None, h_exp=None)
        if u is not None:
            v, where = ucls[u]
            metric = _q_metric(spec)[0] if where == "q" else (pred if where == "pred" or i % 2 == 0 else prio_only)[
                (i // 2) % len(pred if where == "pred" or i % 2 == 0 else prio_only)]
            if where == "q":  # the other terms exactly 0
                c.val[:, n], c.ok[:, n], c.malformed[:, n] = 1.0, 1, False
                c.ts[:, n] = [fresh() for _ in names]
            elif i % 4 < 2:  # lightly loaded: competes for the maximum
                c.val[:, n], c.ok[:, n], c.malformed[:, n] = np.round(0.05 + 0.4 * rng.random(len(names)), 5), 1, False
                c.ts[:, n] = [fresh() for _ in names]
            m = names.index(metric)
            c.val[m, n] = v(spec, metric) if callable(v) else v
            c.ok[m, n], c.malformed[m, n] = 1, False
            e = u_exp.get(n)
            c.ts[m, n] = fresh() if e is None else e - dur[metric]
            lab.update(metric=metric, u_exp=e)
            if e is not None and where == "any" and i % 4 == 0:
                # behind another predicate that expires earlier: infeasible for non-DaemonSet pods until then
                gate = [p for p in pred if p != metric][i // 4 % max(1, len(pred) - 1)]
                g = names.index(gate)
                c.val[g, n], c.ts[g, n] = 0.9, tmin + 1 + int(rng.integers(0, e - tmin)) - dur[gate]
        if h is not None:
            c.hv[n] = hcls[h]
            e = in_range()
            c.hv_ts[n] = fresh() if e is None else e - 300 * NS
            lab.update(h_exp=e)
        labels[n] = lab
    c._raw_ts_s = np.where(c.ok == 1, c.ts // NS, c._raw_ts_s)
    if bind_half:
        bn, bt = [c.b_node], [c.b_ts]
        for n in edge.tolist()[::2]:
            k = int(rng.integers(2, 15))
            bn.append(np.full(k, n, np.int32))
            bt.append(synth.NOW0 - rng.integers(1, 280, k).astype(np.int64))
        bn, bt = np.concatenate(bn), np.concatenate(bt)
        o = np.argsort(bt, kind="stable")  # a time-ordered log, as the ring keeps it
        c.b_node, c.b_ts = bn[o].astype(np.int32), bt[o].astype(np.int64)
    if on_expiries:
        exp = np.array(sorted({e for lab in labels if lab for e in (lab["u_exp"], lab["h_exp"]) if e is not None}), np.int64)
        k = (n_pods - 2) // 3
        pick = rng.choice(exp, k, replace=len(exp) < k)
        rest = rng.integers(tmin, tmax + 1, n_pods - 2 - 3 * k).astype(np.int64)
        now = np.concatenate([pick, pick - 1, pick + 1, rest, [tmin, tmax]]).astype(np.int64)
        rng.shuffle(now)
        c.now = now
    return c, labels


def go_float(v):
    """A double as an annotation would spell it, in the forms strconv.ParseFloat accepts."""
    v = float(v)
    if v != v:
        return "NaN"
    if v in (INF, -INF):
        return "+Inf" if v > 0 else "-Inf"
    return {1e300: "1e300", 0.25: "0x1p-2", 10.5: "1_0.5"}.get(v, repr(v))


def go_stamp(ts_ns, tz_offset_s=SH):
    s, f = divmod(int(ts_ns), NS)
    out = synth._fmt(s, tz_offset_s)
    return out if f == 0 else out[:-1] + ".%09dZ" % f


def edge_annotations(c, tz_offset_s=SH):
    """The cluster as node annotation dicts with every value written by go_float and every stamp
    to the ns (Cluster.annotations rounds to five decimals and whole seconds)."""
    out = []
    for n in range(c.n_nodes):
        a = {}
        for m, name in enumerate(c.metric_names):
            if c.malformed[m, n]:
                stamp = synth._fmt(c.ts_seconds(m, n), tz_offset_s)
                a[name] = go_float(c.val[m, n]) if n % 2 else f"n/a,{stamp}"
            elif c.ok[m, n]:
                a[name] = f"{go_float(c.val[m, n])},{go_stamp(c.ts[m, n], tz_offset_s)}"
        if c.hv_ts[n] != synth.TS_INVALID:
            a["node_hot_value"] = f"{go_float(c.hv[n])},{go_stamp(c.hv_ts[n], tz_offset_s)}"
        out.append(a)
    return out


# ---- the worlds the value-edge tests share: the CPU file asserts from the oracle alone that each
# is live (edge nodes win pods, every class changes some result, edge nodes step inside the
# batch), the GPU file runs the engine on them.
EDGE_TIMES = [T0 + k * 9 * NS for k in range(4)]  # batch times of the step worlds (hot values move)
EDGE_WORLDS = {
    # matrices, top-k, diagnosis, selection: a partial second node block, a partial second sub-chunk
    "mat-default": dict(policy="default", n=257, p=65, seed=8105, share=0.5, on_expiries=True),
    "mat-wsum21": dict(policy="wsum21", n=257, p=65, seed=8103, share=0.5, on_expiries=True),
    "mat-negw": dict(policy="negw", n=257, p=65, seed=8116, share=0.5, on_expiries=True),
    # keys with annotation hot values: two full node blocks and a partial one, two pod tiles
    "keys-default": dict(policy="default", n=600, p=1025, seed=8115),
    "keys-wsum21": dict(policy="wsum21", n=600, p=1025, seed=8116),
    "keys-negw": dict(policy="negw", n=600, p=1025, seed=8119),
    # the step path: hot values from a binding log with bindings on every other edge node
    "step-default": dict(policy="default", n=600, p=1025, seed=8119, hot=False, n_bindings=4000, bind_half=True),
    "step-wsum21": dict(policy="wsum21", n=600, p=1025, seed=8116, hot=False, n_bindings=4000, bind_half=True),
    "step-negw": dict(policy="negw", n=600, p=1025, seed=8117, hot=False, n_bindings=4000, bind_half=True),
}


class EdgeWorld:
    """An edge cluster and the oracle's answers on it, each computed once.  A step world has one
    answer per batch time (hot values from the binding log at that time, stamped with it:
    binding.go:81-97, node.go:113-121), any other world one (the annotations' hot values)."""

    def __init__(self, name):
        kw = dict(EDGE_WORLDS[name])
        self.name = name
        self.spec = edge_policy(kw.pop("policy"))
        self.step = bool(kw.get("bind_half"))
        self.hot = kw.get("hot", True)
        self.c, self.labels = edge_cluster(self.spec, kw.pop("n"), kw.pop("p"), kw.pop("seed"), **kw)
        self.edge = np.array([lab is not None for lab in self.labels])
        self.times = EDGE_TIMES if self.step else [None]
        self._oracle = {}

    def hv_at(self, t):
        _, hv = O.hot_values(self.spec, self.c.b_node, self.c.b_ts, self.c.n_nodes, t // NS)
        return hv.astype(np.float64), np.full(self.c.n_nodes, t, np.int64)

    def eval(self, c, t=None):
        return oracle_soa(self.spec, c, hv_override=None if t is None else self.hv_at(t))

    def oracle(self, t=None):
        """(first_fail [P][N], score [P][N], chosen [P]) — read only."""
        if t not in self._oracle:
            self._oracle[t] = self.eval(self.c, t)
            for a in self._oracle[t]:
                a.setflags(write=False)
        return self._oracle[t]

    def best(self, t=None):
        """(chosen node, its score) per pod, -1 where no node is feasible: what a key packs."""
        ff, sc, ch = self.oracle(t)
        feas = (ff < 0) | (self.c.ds[:, None] != 0)
        return ch, np.where(feas.any(1), np.where(feas, sc, -1).max(1), -1)

    def replaced(self, what):
        """The cluster with every edge usage cell at 0.5 (what = "u") or every edge hot value at
        its HOT_CLASSES replacement ("h")."""
        import dataclasses
        c = dataclasses.replace(self.c)
        c.val, c.hv = self.c.val.copy(), self.c.hv.copy()
        rep = {k: r for k, _, r in HOT_CLASSES}
        for n, lab in enumerate(self.labels):
            if lab and what == "u" and lab["u"]:
                c.val[c.metric_names.index(lab["metric"]), n] = 0.5
            if lab and what == "h" and lab["h"]:
                c.hv[n] = rep[lab["h"]]
        return c


SELECT_CASES = [(0, 3), (100, 3), (0, 30), (100, 30)]  # (percentageOfNodesToScore, the Dynamic plugin's weight)


def select_ext(n_nodes, pct):
    """Other plugins' verdicts as test_select_vs_oracle draws them: a filter that passes 90 % of the
    nodes and a coarse weighted score sum, so that totals tie."""
    rng = np.random.default_rng(n_nodes + pct)
    return rng.random(n_nodes) < 0.9, rng.integers(0, 8, n_nodes) * 100


_worlds = {}


def edge_world(name):
    if name not in _worlds:
        _worlds[name] = EdgeWorld(name)
    return _worlds[name]


def keys_node_score(keys):
    """(node, score) per pod of packed keys, -1 for an empty key."""
    k = np.asarray(keys)
    return np.where(k < 0, -1, 0xFFFFFFFF - (k & 0xFFFFFFFF)), np.where(k < 0, -1, k >> 32)


# ---- greedy: 300 nodes x 400 pods.  Nine in ten ordinary nodes are loaded past every limit, so
# the few light ones run down their staircases within the batch and pods then reach the nodes
# that score 0 — among them the edge nodes, every seventh node.
GREEDY_CASES = ("nan", "plain", "overflow", "1e17", "negw")
GREEDY_NOW = T0 + 1234567


def greedy_world(case):
    """(spec, cluster, edge node indices).  nan: a NaN usage (base int(NaN) = INT64_MIN: the score
    is 0 until the penalty reaches 10, then 100) with a few bindings older than a minute on every
    other one; plain: the same cluster without the NaN cells; overflow: 1e300 / +Inf (INT64_MIN
    through overflow); 1e17: base about -1e18, fits; negw: 1e17 on the negative weight, base
    about +1e18.  Usages alternate between a predicate's metric and a priority-only one."""
    spec = edge_policy("negw" if case == "negw" else "default")
    c = synth.make_cluster(spec, 300, 400, n_bindings=1500, seed=8200, ds_frac=0.05, invalid=False)
    rng = np.random.default_rng(8201)
    c.ts[:] = T0 - 60 * NS
    c.val[:] = np.round(0.90 + 0.09 * rng.random(c.val.shape), 5)
    light = rng.random(300) < 0.1
    c.val[:, light] = np.round(0.05 + 0.5 * rng.random((len(c.metric_names), int(light.sum()))), 5)
    edge = np.arange(3, 300, 7)
    c.val[:, edge] = np.round(0.05 + 0.3 * rng.random((len(c.metric_names), len(edge))), 5)
    keep = ~np.isin(c.b_node, edge)
    c.b_node, c.b_ts = c.b_node[keep], c.b_ts[keep]
    if case == "negw":
        rows, vals = ["cpu_usage_max_avg_1d"], [1e17]
    else:
        rows = ["cpu_usage_avg_5m", "cpu_usage_max_avg_1d", "mem_usage_max_avg_1h", "mem_usage_max_avg_1d"]
        vals = {"nan": [NAN], "plain": [], "overflow": [1e300, INF], "1e17": [1e17]}[case]
    for i, n in enumerate(edge):
        if vals:
            c.val[c.metric_names.index(rows[i % len(rows)]), n] = vals[(i // len(rows)) % len(vals)]
    bn, bt = [c.b_node], [c.b_ts]
    for n in edge[::2]:  # older than the 1-minute window: 3 or 4 of the 5-minute window's 5
        k = 3 + int(n) % 2
        bn.append(np.full(k, n, np.int32))
        bt.append(synth.NOW0 - rng.integers(70, 280, k).astype(np.int64))
    bn, bt = np.concatenate(bn), np.concatenate(bt)
    o = np.argsort(bt, kind="stable")
    c.b_node, c.b_ts = bn[o].astype(np.int32), bt[o].astype(np.int64)
    return spec, c, edge


def greedy_oracle(spec, c, P=400, now=GREEDY_NOW):
    return O.greedy(spec, c.metric_names, c.ok, c.val, np.where(c.ok == 1, c.ts, 0), c.b_node, c.b_ts, now, P, c.ds[:P])


def greedy_replay(spec, c, P=400, now=GREEDY_NOW):
    """The greedy loop spelt out with the per-call oracle: before each pod the hot values of the log
    plus the placements so far (each a binding stamped now), then Filter, Score and the first
    maximum.  Returns (chosen [P], score [P][N] as each pod saw it)."""
    N = c.n_nodes
    chosen, seen = np.empty(P, np.int64), np.empty((P, N), np.int64)
    placed = []
    for p in range(P):
        bn = np.concatenate([c.b_node, np.array(placed, np.int32)])
        bt = np.concatenate([c.b_ts, np.full(len(placed), now // NS, np.int64)])
        _, hv = O.hot_values(spec, bn, bt, N, now // NS)
        _, sc, ch = oracle_soa(spec, c, now=np.array([now], np.int64), ds=c.ds[p:p + 1], threads=1,
                               hv_override=(hv.astype(np.float64), np.full(N, now, np.int64)))
        chosen[p], seen[p] = ch[0], sc[0]
        if ch[0] >= 0:
            placed.append(int(ch[0]))
    return chosen, seen
