"""Filter diagnosis (crane_dyn_filter_counts, csrc/diagnose.hip): per pod, the nodes counted by first
failing predicate (policy order) and, last, the nodes that pass — what kube-scheduler's FitError
prints for a pod that stays Pending.  Everywhere the expected rows are the histogram of the CPU
oracle's first-fail matrix, and they must match exactly.
Reference: pkg/plugins/dynamic/plugins.go:39-69 (Filter, DaemonSet bypass :41-43, the overloaded
predicate as the reason :59-66)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import engine_for, oracle_soa  # noqa: E402

CRANE_E_STATE = -3


def expected(off, n_pred):
    """Rows from a first-fail matrix [P][N]: columns 0 .. n_pred-1 by predicate, then the feasible nodes."""
    cols = [(off == j).sum(axis=1) for j in range(n_pred)] + [(off < 0).sum(axis=1)]
    return np.stack(cols, axis=1).astype(np.int32)


def oracle_counts(spec, c, now=None, ds=None):
    off, _, _ = oracle_soa(spec, c, now=now, ds=ds)
    return expected(off, len(spec["predicate"]))


def expiry_pods(spec, c, n_pick, rng):
    """Pod times exactly on, and 1 ns either side of, the predicate metrics' expiries
    (ts + period + 5m), shuffled; 2 % DaemonSet."""
    dur = {n: p + 300 * 10**9 for n, p in spec["syncPolicy"]}
    exp = []
    for name in sorted({n for n, _ in spec["predicate"]}):
        m = c.metric_names.index(name)
        exp.append(c.ts[m][c.ok[m] == 1] + dur[name])
    pick = rng.choice(np.concatenate(exp), n_pick)
    now = np.concatenate([pick, pick - 1, pick + 1]).astype(np.int64)
    rng.shuffle(now)
    ds = (rng.random(len(now)) < 0.02).astype(np.uint8)
    return now, ds


@pytest.fixture(scope="module")
def on_expiries():
    """Case 2's inputs and their oracle rows, computed once."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 2000, 1, seed=21)
    now, ds = expiry_pods(spec, c, 1500, np.random.default_rng(3))
    return spec, c, now, ds, oracle_counts(spec, c, now, ds)


@pytest.mark.parametrize("n_nodes,n_pods,seed", [(1, 1, 1), (257, 33, 3), (3000, 1025, 5)])
def test_shapes(n_nodes, n_pods, seed):
    """One node and pod; a partial second node block and a partial tile; two pod tiles, shuffled."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, n_nodes, n_pods, seed=seed, pod_step_ns=1_700_000_000)
    now, ds = c.now.copy(), c.ds.copy()
    if n_pods > 1000:
        perm = np.random.default_rng(seed).permutation(n_pods)
        now, ds = now[perm], ds[perm]
    eng = engine_for(spec, c)
    assert eng.n_pred == len(spec["predicate"])
    got = eng.filter_counts(now, ds)
    assert got.dtype == np.int32 and got.shape == (n_pods, eng.n_pred + 1)
    assert np.array_equal(got, oracle_counts(spec, c, now, ds))
    assert (got.sum(axis=1) == n_nodes).all()
    assert (got[ds == 1, -1] == n_nodes).all()
    eng.close()


def test_pod_times_on_expiries(on_expiries):
    """The strict `now < expiry` and the lower bound among the sorted pod times."""
    spec, c, now, ds, want = on_expiries
    eng = engine_for(spec, c)
    assert np.array_equal(eng.filter_counts(now, ds), want)
    eng.close()


def test_unsorted_duplicate_times():
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 5000, 1, seed=22)
    rng = np.random.default_rng(4)
    base = synth.NOW0_NS + rng.integers(-600, 600, 300) * 10**9
    now = np.repeat(base, 4).astype(np.int64)
    rng.shuffle(now)
    ds = (rng.random(len(now)) < 0.3).astype(np.uint8)
    eng = engine_for(spec, c)
    assert np.array_equal(eng.filter_counts(now, ds), oracle_counts(spec, c, now, ds))
    eng.close()


def _policy_shapes():
    m = 60 * 10**9
    base = cd.default_policy_spec()
    # test_policy_variants' first shape: a limit of 0 (active, never overloaded) and a predicate that
    # is not synced (no active duration): both columns stay zero, the others keep the policy's order
    s1 = dict(base)
    s1["predicate"] = base["predicate"] + [("cpu_usage_max_avg_1d", 0.5), ("mem_usage_max_avg_1d", 0.0),
                                           ("not_synced", 0.1), ("mem_usage_avg_5m", 0.3)]
    # its second: 11 predicates, 10 of them active — the 16-predicate instance (512-pod tiles)
    s2 = dict(base)
    s2["syncPolicy"] = base["syncPolicy"] + [("m%d" % i, (i + 1) * m) for i in range(10)] + [("zero", 0), ("neg5", -5 * m)]
    s2["priority"] = base["priority"] + [("m%d" % i, 0.1 * (i + 1)) for i in range(10)] + [("zero", 1.0), ("neg5", 2.0)]
    s2["predicate"] = [("m%d" % i, 0.4 + 0.05 * i) for i in range(10)] + [("neg5", 0.5)]
    s3 = dict(base)
    s3["predicate"] = []
    return [s1, s2, s3]


@pytest.mark.parametrize("i", [0, 1, 2])
def test_policy_shapes(i):
    spec = _policy_shapes()[i]
    c = synth.make_cluster(spec, 777, 40, seed=100 + i, pod_step_ns=20_000_000_000)
    eng = engine_for(spec, c)
    got = eng.filter_counts(c.now, c.ds)
    assert got.shape == (40, len(spec["predicate"]) + 1)
    assert np.array_equal(got, oracle_counts(spec, c))
    if i == 0:
        assert (got[:, 5] == 0).all() and (got[:, 6] == 0).all()  # limit 0, not synced
        assert got[:, 7].any() and got[:, 4].any()                # the predicates around them are counted
    if i == 1:
        assert (got[:, 10] == 0).all() and got[:, :10].any(axis=0).sum() >= 8
    if i == 2:
        assert np.array_equal(got, np.full((40, 1), 777, np.int32))
    eng.close()


def test_forced_slices():
    """Several node slices per pod tile (atomic adds into the zeroed output) against one slice
    (plain stores): 777 nodes = 4 blocks, so 3 slices and 1000 (clamped to 4); 1100 pods = two tiles."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 777, 1100, seed=31, pod_step_ns=900_000_000)
    perm = np.random.default_rng(31).permutation(1100)
    now, ds = c.now[perm], c.ds[perm]
    want = oracle_counts(spec, c, now, ds)
    eng = engine_for(spec, c)
    got = {}
    for s in (1, 3, 1000):
        eng.set_option("diag_slices", s)
        got[s] = eng.filter_counts(now, ds)
        got[s] = eng.filter_counts(now, ds)  # (again: the output is zeroed by every call)
    for s in (1, 3, 1000):
        assert np.array_equal(got[s], want), s
    eng.close()


def test_agrees_with_the_keys():
    """The feasible column is 0 exactly where the keys say -1.  Case 2's cluster gives every pod a
    feasible node, so here every node is overloaded on the first predicate with a fresh stamp: pods
    before the earliest of those expiries have none (one of them 1 ns before it, not a DaemonSet pod)."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 2000, 1, seed=21)
    rng = np.random.default_rng(6)
    m0 = c.metric_names.index(spec["predicate"][0][0])
    c.ok[m0] = 1
    c.val[m0] = 0.99
    c.ts[m0] = (synth.NOW0 - rng.integers(0, 400, 2000)).astype(np.int64) * 10**9
    e_min = int(c.ts[m0].min()) + dict(spec["syncPolicy"])[spec["predicate"][0][0]] + 300 * 10**9
    now, ds = expiry_pods(spec, c, 1500, rng)
    now[:3] = [e_min - 1, e_min, e_min + 1]
    ds[:3] = 0
    want = oracle_counts(spec, c, now, ds)
    eng = engine_for(spec, c)
    got = eng.filter_counts(now, ds)
    assert np.array_equal(got, want)
    _, _, chosen, _ = eng.eval(now, ds)
    assert np.array_equal(got[:, -1] == 0, chosen == -1)
    assert (chosen == -1).sum() >= 1
    assert got[0, 0] == 2000 and got[0, -1] == 0 and got[1, 0] < 2000  # 1 ns before / on the earliest expiry
    eng.close()


def test_state_changes():
    """After update_nodes of 50 nodes and after resize_nodes to 2/3 and back up, the rows are a
    fresh engine's on the same data (and the oracle's)."""
    spec = cd.default_policy_spec()
    N = 1500
    c = synth.make_cluster(spec, N, 200, seed=41, pod_step_ns=3_000_000_000)
    c2 = synth.make_cluster(spec, N, 1, seed=42)
    eng = engine_for(spec, c)
    eng.filter_counts(c.now, c.ds)
    idx = np.random.default_rng(43).choice(N, 50, replace=False).astype(np.int64)
    v2, t2, _ = c2.rows(eng.metric_names)  # (the engine's metric order)
    eng.update_nodes(idx, v2[:, idx], t2[:, idx], c2.hv[idx], c2.hv_ts[idx])
    for f in ("val", "ts", "ok"):
        getattr(c, f)[:, idx] = getattr(c2, f)[:, idx]
    c.hv[idx], c.hv_ts[idx] = c2.hv[idx], c2.hv_ts[idx]
    fresh = engine_for(spec, c)
    want = fresh.filter_counts(c.now, c.ds)
    fresh.close()
    assert np.array_equal(want, oracle_counts(spec, c))
    assert np.array_equal(eng.filter_counts(c.now, c.ds), want)
    # shrink, then nodes join again without annotations
    n2 = 2 * N // 3
    eng.resize_nodes(n2)
    small = c.node_slice(0, n2)
    assert np.array_equal(eng.filter_counts(c.now, c.ds), oracle_counts(spec, small, c.now, c.ds))
    eng.resize_nodes(N)
    c.val[:, n2:], c.ts[:, n2:], c.ok[:, n2:] = 0.0, synth.TS_INVALID, 0
    c.hv[n2:], c.hv_ts[n2:] = 0.0, synth.TS_INVALID
    fresh = engine_for(spec, c)
    want = fresh.filter_counts(c.now, c.ds)
    fresh.close()
    assert np.array_equal(want, oracle_counts(spec, c))
    assert np.array_equal(eng.filter_counts(c.now, c.ds), want)
    assert (want[c.ds == 0, -1] >= N - n2).all()  # a node without annotations passes the Filter
    eng.close()


def test_between_queue_steps_keys_unchanged():
    """A filter_counts call between two steps of the pipelined queue step (two batches pending):
    after the flush every batch's keys equal a run without the call."""
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 5000, 1500, n_bindings=40000, seed=51)
    dev = torch.device("cuda", 0)
    t0 = int(synth.NOW0_NS)
    times = [t0 + (k % 4) * 9_000_000_000 for k in range(5)]
    d_flags = torch.from_numpy(c.ds).to(dev)
    d_now = [torch.from_numpy(c.now + (t - t0)).to(dev) for t in times]
    torch.cuda.synchronize()
    keys, counts = {}, None
    for call in (False, True):
        eng = engine_for(spec, c, opts={"step_defer": 2})
        eng.upload_bindings(c.b_node, c.b_ts)
        q = cd.Queue(0)
        bufs = [torch.empty(1500, dtype=torch.int64, device=dev) for _ in times]
        for b, t in enumerate(times):
            if call and b == 3:
                counts = eng.filter_counts(c.now, c.ds)
            eng.step_keys_queue(t, t, d_now[b], d_flags, bufs[b], q)
        eng.step_flush()
        q.wait()
        keys[call] = [k.cpu().numpy() for k in bufs]
        eng.close()
        q.close()
    for b in range(len(times)):
        assert np.array_equal(keys[True][b], keys[False][b]), b
    assert np.array_equal(counts, oracle_counts(spec, c))


def test_group_equals_one_engine():
    """Three shards on device 0: the summed rows equal one engine over the whole cluster and the oracle."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 1000, 70, seed=61, pod_step_ns=7_000_000_000)
    g = cd.Group(cd.Policy(spec), devices=[0] * 3, depth=1)
    g.set_option("collective", 0)
    val, ts, _ = c.rows(g.metric_names)
    g.upload_nodes(val, ts, c.hv, c.hv_ts)
    got = g.filter_counts(c.now, c.ds)
    eng = engine_for(spec, c)
    one = eng.filter_counts(c.now, c.ds)
    eng.close()
    g.close()
    assert got.dtype == np.int32 and np.array_equal(got, one)
    assert np.array_equal(got, oracle_counts(spec, c))


def test_argument_checks():
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 300, 8, seed=71)
    eng = cd.Engine(cd.Policy(spec), 0)
    with pytest.raises(cd.CraneError) as ei:
        eng.filter_counts(c.now, c.ds)
    assert ei.value.code == CRANE_E_STATE
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts)
    empty = eng.filter_counts(np.zeros(0, np.int64))
    assert empty.shape == (0, eng.n_pred + 1)
    # the device form: a good call, then dtype / shape / contiguity mismatches
    dev = torch.device("cuda", 0)
    d_now = torch.from_numpy(c.now).to(dev)
    d_flags = torch.from_numpy(c.ds).to(dev)
    d_counts = torch.empty((8, eng.n_pred + 1), dtype=torch.int32, device=dev)
    eng.filter_counts_async(d_now, d_flags, d_counts)
    torch.cuda.synchronize()
    eng.filter_counts_async(d_now, None, d_counts)  # (no flags: no DaemonSet pod)
    want = eng.filter_counts(c.now, None)  # (synchronous on the engine stream: the call above is done)
    assert np.array_equal(d_counts.cpu().numpy(), want)
    assert np.array_equal(want, oracle_counts(spec, c, c.now, np.zeros(8, np.uint8)))
    with pytest.raises(ValueError):
        eng.filter_counts_async(d_now.to(torch.float64), d_flags, d_counts)
    with pytest.raises(ValueError):
        eng.filter_counts_async(d_now, d_flags, d_counts.to(torch.int64))
    with pytest.raises(ValueError):
        eng.filter_counts_async(d_now, d_flags, torch.empty((8, eng.n_pred + 2), dtype=torch.int32, device=dev)[:, 1:])
    with pytest.raises(ValueError):
        eng.filter_counts_async(d_now, d_flags, torch.empty((8, eng.n_pred), dtype=torch.int32, device=dev))
    with pytest.raises(ValueError):
        eng.filter_counts_async(d_now, d_flags.cpu(), d_counts)
    with pytest.raises(ValueError):
        eng.filter_counts(c.now, c.ds[:3])
    eng.close()
