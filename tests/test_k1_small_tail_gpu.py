"""The streamed node pass's register tail (csrc/step_node.hpp small_scan and its stores,
taken by csrc/k1stream_body.hpp for a block of at most kSmallTail = 32 one-step records per kind,
staged in LDS, in a step without elementary pieces) against the generic tail on both sides of its
gate.  Every snapshot is built by hand: synth.make_cluster without invalid values, every stamp
60 s old (nothing expires near the batch), then chosen nodes get stamps whose expiries (stamp +
period + 5 min, int64 ns) fall inside the batch's range (tmin, tmax] — the pods' times are spread
over 60 s — so the one-step records per block and kind are known, counted on the host with numpy
and asserted.  Block 0 carries the case; block 1 (300 nodes: partial) always has a few records too.
A pod's key is the maximum over all nodes, so the stepping nodes are made the ones that win: every
other node is loaded past every limit (kind 0 infeasible, a low score for kind 1) but three per
block, and the stepping nodes are lightly loaded, a third of them behind a predicate that expires
at their step (infeasible for kind 0 before it, among the best after) — a wrong position, maximum
or range then changes some pod's chosen node.

Cases: 0, 1, 2, 31, 32, 33 (the generic tail) and 129 (past the LDS staging: st.stage) records per
kind in block 0; ties (equal expiries to the ns, two groups of them, and expiries equal to a pod's
time); nodes whose Filter expiry e_fail is in range (kind 0's keys differ from kind 1's), and with a
policy whose first predicate is no priority nodes that step for kind 0 only (32 records against 5);
nodes with two distinct in-range expiries (half-line records and a middle piece); all pods
DaemonSet and none (a kind without pods); 1 pod, 1,025 (two tiles) and 33,793 (34 tiles: three rounds
of item lanes).  Each with engine options k1_tail 0 / 1 / 4 (four-wave and single-wave tails) and
step_rows 1 / 0 (0: K3s reads pm1 / sm0 itself), on a HIP stream (step_keys_async, four batch
times) and on a cd.Queue with step_defer 2 (six batches, two key buffers, exactly one packet per
step from the third on).
References, bit for bit: the same batch on an engine with option k1_stream 0 (the fused record
pass, which keeps the generic tail), and for every pod of the cases of at most 1,025 pods the CPU
oracle's chosen node and score (plugins.go:39-98 + selectHost; hot values binding.go:81-97)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import oracle_soa  # noqa: E402

T0 = int(synth.NOW0_NS)
S = 10**9
SMALL = 32   # kSmallTail (k1stream_body.hpp)
SCAP = 128   # kSCap: one-step records per kind the LDS staging holds
BLK = 256    # nodes per K1 block
SPAN = 60 * S  # the pods' spread: the batch range is (T0, T0 + about SPAN]
TIMES = [T0 + k * 9 * S for k in range(4)]  # batch times (the hot values move; the pods' times stay)
INT64_MIN, INT64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max

CPU5, CPU1H, CPU1D, MEM5, MEM1H, MEM1D = ("cpu_usage_avg_5m", "cpu_usage_max_avg_1h", "cpu_usage_max_avg_1d",
                                          "mem_usage_avg_5m", "mem_usage_max_avg_1h", "mem_usage_max_avg_1d")


def spec_kind0_only():
    """The default policy without its first priority: cpu_usage_avg_5m is a predicate only, so its
    expiry steps kind 0's key alone (DaemonSet pods bypass the Filter)."""
    s = cd.default_policy_spec()
    s["priority"] = [p for p in s["priority"] if p[0] != CPU5]
    return s


class Snapshot:
    """A hand-built cluster, its pods and where its in-range expiries are."""

    def __init__(self, name, n_nodes, n_pods, ds="synth", spec=None, seed=1):
        self.name, self.P = name, n_pods
        self.spec = spec or cd.default_policy_spec()
        self.c = c = synth.make_cluster(self.spec, n_nodes, n_pods, n_bindings=4000, seed=20261100 + seed, invalid=False)
        c.ts[:] = T0 - 60 * S
        self.rng = np.random.default_rng(20261102 + seed)
        c.val[:] = np.round(0.90 + 0.09 * self.rng.random(c.val.shape), 5)  # loaded past every limit
        for b in range(0, n_nodes, BLK):  # three flat nodes per block that compete
            c.val[:, b + self.rng.permutation(min(BLK, n_nodes - b))[:3]] = 0.45
        self.light = set()
        step = SPAN // (n_pods - 1) if n_pods > 1 else 0
        c.now, c.ds = synth.make_pods(n_pods, seed=20261101 + seed, pod_step_ns=step)
        if ds == "all":
            c.ds[:] = 1
        elif ds == "none":
            c.ds[:] = 0
        self.step = step
        self.dur = {n: p + 300 * S for n, p in self.spec["syncPolicy"]}
        self.want = None  # (kind 0, kind 1) one-step records of block 0

    def expire(self, node, metric, at_ns, value=None):
        m = self.c.metric_names.index(metric)
        if node not in self.light:  # a stepping node is lightly loaded: it competes for the maximum
            self.light.add(node)
            self.c.val[:, node] = np.round(0.05 + 0.5 * self.rng.random(len(self.c.metric_names)), 5)
        self.c.ts[m, node] = at_ns - self.dur[metric]
        if value is not None:
            self.c.val[m, node] = value

    def calm(self, node):
        """Every predicate metric of the node under its limit (its e_fail is then what a test sets)."""
        for n, _ in self.spec["predicate"]:
            self.c.val[self.c.metric_names.index(n), node] = 0.3

    def gate(self, node, metric, at_ns, u):
        """The node's only over-limit predicate expires at at_ns (kind 0: infeasible before, feasible
        after); every other metric at usage u."""
        self.expire(node, metric, at_ns)
        self.c.val[:, node] = u
        self.c.val[self.c.metric_names.index(metric), node] = 0.9

    def instants(self, k):
        """k distinct instants inside every batch's range, in no order."""
        return T0 + 30 * S + self.rng.permutation(k).astype(np.int64) * 1_000_003 + 17

    def one_step(self, k, block=0, metric=CPU5):
        """k nodes of the block with one in-range expiry each, at distinct instants."""
        size = min(BLK, self.c.n_nodes - block * BLK)
        nodes = block * BLK + np.sort(self.rng.permutation(size)[:k])
        for i, (n, e) in enumerate(zip(nodes, self.instants(k))):
            if i % 3 == 2 and metric in (CPU5, MEM5, CPU1H, MEM1H):  # (a predicate's metric)
                self.gate(int(n), metric, int(e), round(0.05 + 0.3 * float(self.rng.random()), 5))
            else:
                self.expire(int(n), metric, int(e))
        return nodes

    # ---- host-side count of the step records, as the node pass classifies (step_node.hpp)
    def records(self):
        """[blocks][2] one-step records and [blocks][2] middle pieces per kind."""
        c = self.c
        tmin, tmax = int(c.now.min()), int(c.now.max())
        assert tmax < TIMES[0] + 300 * S, "the hot value's expiry (batch time + 5 min) stays out of range"
        row = c.metric_names.index
        prio = np.stack([c.ts[row(n)] + self.dur[n] for n, _ in self.spec["priority"]])
        pred = np.stack([np.where(c.val[row(n)] > lim, c.ts[row(n)] + self.dur[n], INT64_MIN)
                         for n, lim in self.spec["predicate"]])
        e_fail = pred.max(0)

        def classify(E):
            inr = (E > tmin) & (E <= tmax)
            cnt = inr.sum(0)
            multi = (cnt > 0) & (np.where(inr, E, INT64_MAX).min(0) != np.where(inr, E, INT64_MIN).max(0))
            return np.where(cnt == 0, 0, np.where(multi, 2, 1)), np.where(multi, cnt - 1, 0)

        r0, m0 = classify(np.vstack([prio, e_fail[None]]))
        r1, m1 = classify(prio)
        nb = -(-c.n_nodes // BLK)
        pad = nb * BLK - c.n_nodes
        blk = lambda x: np.pad(x, (0, pad)).reshape(nb, BLK).sum(1)  # noqa: E731
        return np.stack([blk(r0), blk(r1)], 1), np.stack([blk(m0), blk(m1)], 1)


def _records(k):
    def make(s):
        s.one_step(k)
        s.one_step(3, block=1, metric=MEM5)
        s.want = (k, k)
    return make


def _ties(s):
    """Gated nodes (the later the step, the lighter the node: each wins from its own step on):
    three stepping at one instant and two at another (to the ns), and one each at the time of the
    last pod of either kind in tile 0, of the first DaemonSet pod and of the batch's last pod (a
    tile bound equal to a step: bp <= v); two plain ones; spread over the block's waves."""
    now, ds = s.c.now, s.c.ds
    k0, k1 = np.flatnonzero(ds[:1024] == 0), np.flatnonzero(ds[:1024] == 1)
    a, b = T0 + 41 * S + 123_456_789, T0 + 33 * S + 5
    at = {7: a, 70: a, 200: a, 130: b, 66: b, 3: int(now[k0[-1]]), 255: int(now[k1[-1]]), 129: int(now[k1[0]]),
          64: int(now[-1])}
    assert len(set(at.values())) == 6 and min(at.values()) > now[0]
    for n, e in at.items():
        s.gate(n, CPU5 if n % 2 else MEM5, e, round(0.5 - 0.45 * (e - T0) / SPAN, 5))
    s.expire(100, CPU1H, T0 + 50 * S)
    s.expire(101, MEM1D, T0 + 31 * S)
    s.one_step(4, block=1)
    s.one_step(32, block=2)
    s.one_step(33, block=3, metric=MEM1H)
    s.want = (11, 11)


def _efail(s):
    """Five nodes whose only over-limit predicate expires in range (kind 0: infeasible before the
    step, kind 1 feasible throughout) among five plain ones."""
    nodes = s.one_step(10, metric=MEM1D)  # (no predicate's metric: none gated yet)
    for n in nodes:
        s.calm(int(n))
    for i, n in enumerate(nodes[::2]):
        s.gate(int(n), CPU5, T0 + (36 + 4 * i) * S + i, 0.3 - 0.05 * i)
    for n in nodes[::2]:  # (one expiry each: the first one back out of range)
        s.c.ts[s.c.metric_names.index(MEM1D), n] = T0 - 60 * S
    s.one_step(2, block=1)
    s.want = (10, 10)


def _kind0_only(s):
    """(spec_kind0_only) 27 nodes whose e_fail alone is in range and 5 that step for both kinds."""
    nodes = BLK - 1 - np.sort(s.rng.permutation(BLK)[:27])
    for i, (n, e) in enumerate(zip(nodes, s.instants(27))):
        s.gate(int(n), CPU5, int(e), round(0.05 + 0.01 * i, 5))
    free = np.setdiff1d(np.arange(BLK), nodes)[:5]
    for n, e in zip(free, s.instants(5)):
        s.expire(int(n), MEM1D, int(e) + 7 * S)
    s.one_step(3, block=1, metric=MEM1H)
    s.want = (32, 5)


def _multi(s):
    """Three nodes with two metrics expiring at distinct in-range instants (two half-line records
    and a middle piece each), four one-step nodes."""
    nodes = s.one_step(7)
    for i, n in enumerate(nodes[:3]):
        s.calm(int(n))  # (no e_fail: a repeated expiry would reserve an empty piece more)
        s.expire(int(n), MEM1D, T0 + (45 + i) * S + i)
    s.one_step(2, block=1)
    s.want = (10, 10)


SNAPSHOTS = {
    "rec0": (300, 1025, "synth", None, lambda s: setattr(s, "want", (0, 0))),
    "rec1": (300, 1025, "synth", None, _records(1)),
    "rec2": (300, 1025, "synth", None, _records(2)),
    "rec31": (300, 1025, "synth", None, _records(SMALL - 1)),
    "rec32": (300, 1025, "synth", None, _records(SMALL)),
    "rec33": (300, 1025, "synth", None, _records(SMALL + 1)),
    "rec129": (300, 1025, "synth", None, _records(SCAP + 1)),
    "ties": (1000, 1025, "synth", None, _ties),
    "efail": (300, 1025, "synth", None, _efail),
    "kind0_only": (300, 1025, "synth", spec_kind0_only, _kind0_only),
    "multi": (300, 1025, "synth", None, _multi),
    "ds_all": (300, 1025, "all", None, _records(5)),
    "ds_none": (300, 1025, "none", None, _records(5)),
    "pod1": (300, 1, "synth", None, lambda s: (s.one_step(5), setattr(s, "want", (0, 0)))),
    "tiles34": (1000, 33793, "synth", None, _records(12)),
}


def _engine(w, opts=()):
    e = cd.Engine(cd.Policy(w.spec), 0)
    for k, v in opts:
        e.set_option(k, v)
    val, ts, _ = w.c.rows(e.metric_names)
    e.upload_nodes(val, ts, w.c.hv, w.c.hv_ts)
    e.upload_bindings(w.c.b_node, w.c.b_ts)
    return e


class World(Snapshot):
    """A snapshot on the device with its references per batch time, each computed once: the keys
    of the fused record pass (engine option k1_stream 0) and the oracle's choice and score."""

    def __init__(self, name):
        import torch
        n_nodes, n_pods, ds, spec, place = SNAPSHOTS[name]
        super().__init__(name, n_nodes, n_pods, ds, spec() if spec else None, seed=sorted(SNAPSHOTS).index(name))
        place(self)
        self.dev = torch.device("cuda", 0)
        self.st = torch.cuda.Stream(self.dev)
        self.d_now = torch.from_numpy(self.c.now).to(self.dev)
        self.d_flags = torch.from_numpy(self.c.ds).to(self.dev)
        self.fused = self.stream_keys((("k1_stream", 0),))
        self.oracle = {}
        if n_pods <= 1025:
            for t in TIMES:
                from oracle import oracle as O
                _, hv = O.hot_values(self.spec, self.c.b_node, self.c.b_ts, self.c.n_nodes, t // S)
                ff, sc, och = oracle_soa(self.spec, self.c, hv_override=(hv.astype(np.float64),
                                                                         np.full(self.c.n_nodes, t, np.int64)))
                feas = (ff < 0) | (self.c.ds[:, None] != 0)
                self.oracle[t] = (och, np.where(feas.any(1), np.where(feas, sc, -1).max(1), -1))

    def stream_keys(self, opts, names=None):
        """The four batches on a HIP stream: keys per batch time."""
        import torch
        eng = _engine(self, opts)
        out = {}
        torch.cuda.synchronize()
        for t in TIMES:
            k = torch.empty(self.P, dtype=torch.int64, device=self.dev)
            if names is not None:
                eng.set_profiling(t == TIMES[-1])
            eng.step_keys_async(t, t, self.d_now, self.d_flags, k, self.st.cuda_stream)
            self.st.synchronize()
            out[t] = k
        if names is not None:
            names.extend(n for n, _ in eng.stage_times())
        eng.close()
        return out

    def check(self, t, keys, what):
        import torch
        assert torch.equal(keys, self.fused[t]), f"{self.name} {what}: keys differ from the fused pass's"
        if t in self.oracle:
            k = keys.cpu().numpy()
            och, best = self.oracle[t]
            assert np.array_equal(np.where(k < 0, -1, 0xFFFFFFFF - (k & 0xFFFFFFFF)), och), f"{self.name} {what}: node"
            assert np.array_equal(np.where(k < 0, -1, k >> 32), best), f"{self.name} {what}: score"


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(name):
        if name not in made:
            made[name] = World(name)
        return made[name]

    return get


@pytest.mark.parametrize("name", sorted(SNAPSHOTS))
def test_snapshots_hold_the_records_they_claim(name):
    """Block 0's one-step records per kind are what the case says (counted on the host as the node
    pass classifies), on the side of the gate it is meant for; block 1 has some too."""
    n_nodes, n_pods, ds, spec, place = SNAPSHOTS[name]
    s = Snapshot(name, n_nodes, n_pods, ds, spec() if spec else None, seed=sorted(SNAPSHOTS).index(name))
    place(s)
    rec, mid = s.records()
    assert tuple(rec[0]) == s.want, (rec, s.want)
    if name not in ("rec0", "pod1"):
        assert rec[1].min() > 0 and rec[1].max() <= SMALL, rec
    if name == "multi":
        assert tuple(mid[0]) == (3, 3), mid
    else:
        assert mid.sum() == 0, mid
    if name == "ties":
        assert tuple(rec[2]) == (SMALL, SMALL) and tuple(rec[3]) == (SMALL + 1, SMALL + 1), rec
    if name == "kind0_only":
        assert len(s.spec["priority"]) == 5
    if name in ("ds_all", "ds_none"):
        assert s.c.ds.min() == s.c.ds.max() == (name == "ds_all")
    else:
        assert n_pods == 1 or 0 < s.c.ds.sum() < n_pods, "both kinds have pods"
    assert -(-n_pods // 1024) == {1: 1, 1025: 2, 33793: 34}[n_pods]


def test_fused_reference_matches_oracle(worlds):
    """The reference itself: the fused pass's keys give the oracle's node and score for every pod."""
    for name in ("rec32", "ties", "kind0_only"):
        w = worlds(name)
        for t in TIMES:
            w.check(t, w.fused[t], "fused")


def test_stream_route_runs_the_streamed_pass(worlds):
    """With kernel timing on, the step's node pass on a stream is k1_stream_steps (the pass under
    test), not the fused pass."""
    names = []
    w = worlds("rec2")
    keys = w.stream_keys((), names)
    assert "k1_stream_steps" in names and "k1_node_pass+k3a_steps" not in names, names
    w.check(TIMES[-1], keys[TIMES[-1]], "profiled")


@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("tail", [0, 1, 4])
@pytest.mark.parametrize("name", sorted(SNAPSHOTS))
def test_stream(worlds, name, tail, rows):
    """step_keys_async at the four batch times: every batch's keys equal both references."""
    w = worlds(name)
    keys = w.stream_keys((("k1_tail", tail), ("step_rows", rows)))
    for t in TIMES:
        w.check(t, keys[t], f"stream k1_tail {tail} step_rows {rows} t {(t - T0) // S}")


@pytest.mark.parametrize("rows", [1, 0])
@pytest.mark.parametrize("tail", [0, 1, 4])
@pytest.mark.parametrize("name", sorted(SNAPSHOTS))
def test_queue_one_launch(worlds, name, tail, rows):
    """Six batches on a dispatch queue with step_defer 2 into two alternating key buffers: each
    step from the third on is one packet (step_one_launch, the pass beside K3s and K2 + K3p), and
    the last two batches' keys equal both references."""
    import torch
    w = worlds(name)
    eng = _engine(w, (("step_defer", 2), ("k1_tail", tail), ("step_rows", rows)))
    q = cd.Queue(0)
    two = [torch.empty(w.P, dtype=torch.int64, device=w.dev) for _ in range(2)]
    times = [TIMES[b % 4] for b in range(6)]
    torch.cuda.synchronize()
    packets = []
    for b, t in enumerate(times):
        before = q.packets()
        eng.step_keys_queue(t, t, w.d_now, w.d_flags, two[b % 2], q)
        packets.append(q.packets() - before)
    eng.step_flush()
    q.wait()
    assert packets[2:] == [1] * 4, packets
    for b in (4, 5):
        w.check(times[b], two[b % 2], f"queue k1_tail {tail} step_rows {rows} batch {b}")
    eng.close()
    q.close()
