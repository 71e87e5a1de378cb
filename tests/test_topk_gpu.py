"""Top-k candidates (crane_dyn_topk, csrc/topk.hip): per pod the k best feasible nodes as packed
keys, (score << 32) | (0xFFFFFFFF - global node), best first (highest score, lowest index on ties),
-1 where the pod has fewer than k feasible nodes.  Everywhere the expected rows come from the CPU
oracle's first-fail and score matrices and nothing else, and they must match exactly.
Reference: pkg/plugins/dynamic/plugins.go:39-98 (Filter, DaemonSet bypass :41-43, Score)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import engine_for, oracle_soa  # noqa: E402
from oracle import oracle as O  # noqa: E402
from test_filter_counts_gpu import _policy_shapes, expiry_pods  # noqa: E402

CRANE_E_INVALID = -1
CRANE_E_STATE = -3


def want_rows(spec, c, now, ds, k, node_offset=0, hv_override=None):
    off, sc, _ = oracle_soa(spec, c, now, ds, hv_override=hv_override)
    N = off.shape[1]
    feas = (off < 0) | (np.asarray(ds)[:, None] == 1)
    key = np.where(feas, (sc.astype(np.int64) << 32) | (0xFFFFFFFF - (node_offset + np.arange(N))), -1)
    want = -np.sort(-key, axis=1)[:, :k]
    if N < k:
        want = np.concatenate([want, np.full((len(want), k - N), -1, np.int64)], axis=1)
    return want


def decode(row):
    return [cd.key_node(int(x)) for x in row]


@pytest.mark.parametrize("n_nodes,n_pods,k,seed", [(1, 1, 1, 1), (1, 1, 16, 1), (257, 65, 3, 3), (3000, 1025, 16, 5)])
def test_shapes(n_nodes, n_pods, k, seed):
    """One node and pod, with 15 pads at k = 16; a partial second node block and a partial second
    64-pod sub-chunk; several pod chunks of shuffled pods with heavy score ties."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, n_nodes, n_pods, seed=seed, pod_step_ns=1_700_000_000)
    now, ds = c.now.copy(), c.ds.copy()
    if n_pods > 1000:
        perm = np.random.default_rng(seed).permutation(n_pods)
        now, ds = now[perm], ds[perm]
    want = want_rows(spec, c, now, ds, k)
    eng = engine_for(spec, c)
    got = eng.topk(now, ds, k=k)
    assert got.dtype == np.int64 and got.shape == (n_pods, k)
    assert np.array_equal(got, want)
    if n_nodes == 1 and k == 16:
        assert (got[:, 1:] == -1).all()
    if k == 16:
        assert np.array_equal(eng.topk(now, ds, k=5), got[:, :5])
    if n_pods > 1000:
        assert len(np.unique(want, axis=0)) > 100  # (the oracle: 131 distinct rows)
    eng.close()


@pytest.fixture(scope="module")
def few_feasible():
    """Every node overloaded on the first predicate with a fresh stamp: pods before the earliest of
    those expiries have no feasible node, pods on the next few expiries a handful."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 2000, 1, seed=21)
    rng = np.random.default_rng(6)
    name = spec["predicate"][0][0]
    m0 = c.metric_names.index(name)
    c.ok[m0] = 1
    c.val[m0] = 0.99
    c.ts[m0] = (synth.NOW0 - rng.integers(0, 400, 2000)).astype(np.int64) * 10**9
    exp = np.sort(c.ts[m0] + dict(spec["syncPolicy"])[name] + 300 * 10**9)[:40]
    now = np.concatenate([exp, exp - 1, exp + 1]).astype(np.int64)
    rng.shuffle(now)
    ds = (rng.random(len(now)) < 0.05).astype(np.uint8)
    return spec, c, now, ds, want_rows(spec, c, now, ds, 16)


def test_fewer_than_k_feasible(few_feasible):
    import torch
    spec, c, now, ds, want = few_feasible
    n_want = (want >= 0).sum(axis=1)
    assert (n_want == 0).any() and ((n_want > 0) & (n_want < 16)).any() and (n_want == 16).any()
    eng = engine_for(spec, c)
    got = eng.topk(now, ds, k=16)
    assert np.array_equal(got, want)
    counts = eng.filter_counts(now, ds)
    assert np.array_equal((got >= 0).sum(axis=1), np.minimum(16, counts[:, -1]))
    dev = torch.device("cuda", 0)
    d_keys = torch.empty(len(now), dtype=torch.int64, device=dev)
    eng.eval_keys_async(torch.from_numpy(now).to(dev), torch.from_numpy(ds).to(dev), d_keys)
    torch.cuda.synchronize()
    assert np.array_equal(got[:, 0], d_keys.cpu().numpy())
    eng.close()


@pytest.mark.parametrize("node_offset", [0, 1000])
def test_pure_tie_break(node_offset):
    """600 identical nodes: the index alone orders them, within one slice and across three."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 600, 4, seed=11)
    stamp = (synth.NOW0 - 10) * 10**9
    c.ok[:], c.val[:], c.ts[:] = 1, 0.3, stamp
    c.malformed[:] = False
    c.hv[:], c.hv_ts[:] = 2.0, stamp
    ds = np.array([0, 1, 0, 1], np.uint8)
    want = want_rows(spec, c, c.now, ds, 16, node_offset=node_offset)
    for slices in (1, 3):
        eng = cd.Engine(cd.Policy(spec), 0)
        eng.set_option("topk_slices", slices)
        val, ts, _ = c.rows(eng.metric_names)
        eng.upload_nodes(val, ts, c.hv, c.hv_ts, node_offset=node_offset)
        got = eng.topk(c.now, ds, k=16)
        eng.close()
        assert np.array_equal(got, want), slices
        for row in got:
            nodes, scores = zip(*decode(row))
            assert list(nodes) == list(range(node_offset, node_offset + 16))
            assert len(set(scores)) == 1


def test_forced_slices():
    """One slice (plain stores to the output) against several (partial rows and the second phase):
    777 nodes = 4 blocks, so 3 slices and 1000 (clamped to 4); 1100 pods = several chunks."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 777, 1100, seed=31, pod_step_ns=900_000_000)
    perm = np.random.default_rng(31).permutation(1100)
    now, ds = c.now[perm], c.ds[perm]
    want = want_rows(spec, c, now, ds, 8)
    eng = engine_for(spec, c)
    got = {}
    for s in (1, 3, 1000):
        eng.set_option("topk_slices", s)
        got[s] = [eng.topk(now, ds, k=8), eng.topk(now, ds, k=8)]
    for s in (1, 3, 1000):
        for g in got[s]:
            assert np.array_equal(g, want), s
    eng.close()


def test_pod_times_on_expiries():
    """The strict `now < expiry`: pod times on the predicates' expiries and 1 ns either side."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 2000, 1, seed=21)
    now, ds = expiry_pods(spec, c, 1500, np.random.default_rng(3))
    eng = engine_for(spec, c)
    assert np.array_equal(eng.topk(now, ds, k=4), want_rows(spec, c, now, ds, 4))
    eng.close()


def test_hot_values_from_bindings():
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 3000, 200, n_bindings=20000, seed=81, pod_step_ns=2_000_000_000)
    t = int(synth.NOW0_NS)
    eng = engine_for(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    eng.refresh_hot_values(t, t)
    got = eng.topk(c.now, c.ds, k=8)
    eng.close()
    _, hv = O.hot_values(spec, c.b_node, c.b_ts, c.n_nodes, t // 10**9)
    want = want_rows(spec, c, c.now, c.ds, 8, hv_override=(hv.astype(np.float64), np.full(c.n_nodes, t, np.int64)))
    assert np.array_equal(got, want)


def _specs():
    s4 = dict(cd.default_policy_spec())
    s4["priority"] = []
    return _policy_shapes() + [s4]


@pytest.mark.parametrize("i", [0, 1, 2, 3])
def test_policy_shapes(i):
    """8 predicates, 11 predicates (the 16 x 16 record shape), no predicates, no priorities."""
    spec = _specs()[i]
    c = synth.make_cluster(spec, 777, 40, seed=100 + i, pod_step_ns=20_000_000_000)
    eng = engine_for(spec, c)
    got = eng.topk(c.now, c.ds, k=6)
    eng.close()
    assert np.array_equal(got, want_rows(spec, c, c.now, c.ds, 6))
    if i == 3:
        assert all(s == 0 for row in got for _, s in decode(row[row >= 0]))  # no priorities: score 0


def test_state_changes():
    """After update_nodes of 50 nodes and after resize_nodes to 2/3 and back up, the rows are a
    fresh engine's on the same data and the oracle's."""
    spec = cd.default_policy_spec()
    N = 1500
    c = synth.make_cluster(spec, N, 200, seed=41, pod_step_ns=3_000_000_000)
    c2 = synth.make_cluster(spec, N, 1, seed=42)
    eng = engine_for(spec, c)
    eng.topk(c.now, c.ds, k=8)
    idx = np.random.default_rng(43).choice(N, 50, replace=False).astype(np.int64)
    v2, t2, _ = c2.rows(eng.metric_names)  # (the engine's metric order)
    eng.update_nodes(idx, v2[:, idx], t2[:, idx], c2.hv[idx], c2.hv_ts[idx])
    for f in ("val", "ts", "ok"):
        getattr(c, f)[:, idx] = getattr(c2, f)[:, idx]
    c.hv[idx], c.hv_ts[idx] = c2.hv[idx], c2.hv_ts[idx]

    def fresh_rows(cl):
        fresh = engine_for(spec, cl)
        rows = fresh.topk(c.now, c.ds, k=8)
        fresh.close()
        return rows

    want = want_rows(spec, c, c.now, c.ds, 8)
    assert np.array_equal(fresh_rows(c), want)
    assert np.array_equal(eng.topk(c.now, c.ds, k=8), want)
    n2 = 2 * N // 3
    eng.resize_nodes(n2)
    assert np.array_equal(eng.topk(c.now, c.ds, k=8), want_rows(spec, c.node_slice(0, n2), c.now, c.ds, 8))
    eng.resize_nodes(N)  # nodes join again without annotations
    c.val[:, n2:], c.ts[:, n2:], c.ok[:, n2:] = 0.0, synth.TS_INVALID, 0
    c.hv[n2:], c.hv_ts[n2:] = 0.0, synth.TS_INVALID
    want = want_rows(spec, c, c.now, c.ds, 8)
    assert np.array_equal(fresh_rows(c), want)
    assert np.array_equal(eng.topk(c.now, c.ds, k=8), want)
    eng.close()


def test_between_queue_steps_keys_unchanged():
    """A topk call between two steps of the pipelined queue step (two batches pending): after the
    flush every batch's keys equal a run without the call, and the call's rows are the oracle's for
    the hot values of the engine's last refresh before it (the step before the call)."""
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 5000, 1500, n_bindings=40000, seed=51)
    dev = torch.device("cuda", 0)
    t0 = int(synth.NOW0_NS)
    times = [t0 + (k % 4) * 9_000_000_000 for k in range(5)]
    d_flags = torch.from_numpy(c.ds).to(dev)
    d_now = [torch.from_numpy(c.now + (t - t0)).to(dev) for t in times]
    torch.cuda.synchronize()
    keys, rows = {}, None
    for call in (False, True):
        eng = engine_for(spec, c, opts={"step_defer": 2})
        eng.upload_bindings(c.b_node, c.b_ts)
        q = cd.Queue(0)
        bufs = [torch.empty(1500, dtype=torch.int64, device=dev) for _ in times]
        for b, t in enumerate(times):
            if call and b == 3:
                rows = eng.topk(c.now, c.ds, k=8)
            eng.step_keys_queue(t, t, d_now[b], d_flags, bufs[b], q)
        eng.step_flush()
        q.wait()
        keys[call] = [k.cpu().numpy() for k in bufs]
        eng.close()
        q.close()
    for b in range(len(times)):
        assert np.array_equal(keys[True][b], keys[False][b]), b
    _, hv = O.hot_values(spec, c.b_node, c.b_ts, c.n_nodes, times[2] // 10**9)
    want = want_rows(spec, c, c.now, c.ds, 8,
                     hv_override=(hv.astype(np.float64), np.full(c.n_nodes, times[2], np.int64)))
    assert np.array_equal(rows, want)


def test_group_equals_one_engine_and_the_merge():
    """Three shards on device 0: the merged rows equal one engine over the whole cluster, the oracle,
    and cd.topk_merge of three engines created with the shards' node offsets."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 1000, 70, seed=61, pod_step_ns=7_000_000_000)
    g = cd.Group(cd.Policy(spec), devices=[0] * 3, depth=1)
    g.set_option("collective", 0)
    val, ts, _ = c.rows(g.metric_names)
    g.upload_nodes(val, ts, c.hv, c.hv_ts)
    got = g.topk(c.now, c.ds, k=8)
    shards = [g.shard(i) for i in range(3)]
    g.close()
    eng = engine_for(spec, c)
    one = eng.topk(c.now, c.ds, k=8)
    eng.close()
    assert got.dtype == np.int64 and np.array_equal(got, one)
    assert np.array_equal(got, want_rows(spec, c, c.now, c.ds, 8))
    parts = []
    for _, lo, hi in shards:
        e = cd.Engine(cd.Policy(spec), 0)
        v, t, _ = c.rows(e.metric_names)
        e.upload_nodes(v[:, lo:hi], t[:, lo:hi], c.hv[lo:hi], c.hv_ts[lo:hi], node_offset=lo)
        parts.append(e.topk(c.now, c.ds, k=8))
        e.close()
    assert np.array_equal(cd.topk_merge(parts), got)


def test_argument_checks():
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 300, 8, seed=71)
    eng = cd.Engine(cd.Policy(spec), 0)
    with pytest.raises(cd.CraneError) as ei:
        eng.topk(c.now, c.ds, k=4)
    assert ei.value.code == CRANE_E_STATE
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts)
    for k in (0, 17):
        with pytest.raises(cd.CraneError) as ei:
            eng.topk(c.now, c.ds, k=k)
        assert ei.value.code == CRANE_E_INVALID
    empty = eng.topk(np.zeros(0, np.int64), k=5)
    assert empty.shape == (0, 5) and empty.dtype == np.int64
    # the device form: a good call, then dtype / shape / contiguity / device mismatches
    dev = torch.device("cuda", 0)
    d_now = torch.from_numpy(c.now).to(dev)
    d_flags = torch.from_numpy(c.ds).to(dev)
    d_keys = torch.empty((8, 4), dtype=torch.int64, device=dev)
    eng.topk_async(d_now, d_flags, d_keys)
    want = eng.topk(c.now, c.ds, k=4)  # (synchronous on the engine stream: the call above is done)
    assert np.array_equal(d_keys.cpu().numpy(), want)
    assert np.array_equal(want, want_rows(spec, c, c.now, c.ds, 4))
    eng.topk_async(d_now, None, d_keys)  # (no flags: no DaemonSet pod)
    want = eng.topk(c.now, None, k=4)
    assert np.array_equal(d_keys.cpu().numpy(), want)
    assert np.array_equal(want, want_rows(spec, c, c.now, np.zeros(8, np.uint8), 4))
    with pytest.raises(cd.CraneError) as ei:
        eng.topk_async(d_now, d_flags, torch.empty((8, 17), dtype=torch.int64, device=dev))
    assert ei.value.code == CRANE_E_INVALID
    with pytest.raises(ValueError):
        eng.topk_async(d_now.to(torch.float64), d_flags, d_keys)
    with pytest.raises(ValueError):
        eng.topk_async(d_now, d_flags, d_keys.to(torch.int32))
    with pytest.raises(ValueError):
        eng.topk_async(d_now, d_flags, torch.empty((8, 5), dtype=torch.int64, device=dev)[:, 1:])
    with pytest.raises(ValueError):
        eng.topk_async(d_now, d_flags, torch.empty((7, 4), dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        eng.topk_async(d_now, d_flags, torch.empty(32, dtype=torch.int64, device=dev))
    with pytest.raises(ValueError):
        eng.topk_async(d_now, d_flags.cpu(), d_keys)
    with pytest.raises(ValueError):
        eng.topk(c.now, c.ds[:3], k=4)
    eng.close()
