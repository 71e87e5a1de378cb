"""Sequential greedy at per-pod times (crane_dyn_greedy_times, csrc/greedy_times.hip) against the
reference composed from the oracle (greedy_times_ref.ref): pod p is one greedy placement at
now[p] over the uploaded log plus the earlier placements, each stamped its own second.  Between
two pods annotations go stale (stats.go:42-48), log bindings leave the hotValue windows
(binding.go:85-91) and, past a window's length, so do the batch's own placements.  Every result is
bit-exact.  Each targeted case also differs from the frozen-time greedy at now[0], so a build that
ignored its event class could not pass.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import engine_for, oracle_soa  # noqa: E402
import greedy_times_ref as R  # noqa: E402

CRANE_E_INVALID = -1
CRANE_E_STATE = -3
NS = R.NS


def _run(spec, c, now, ds, opts=None, log="upload"):
    eng = engine_for(spec, c, opts=opts)
    if log == "upload":
        eng.upload_bindings(c.b_node, c.b_ts)
    elif log == "heap":
        eng.binding_records(len(c.b_node) + 7, 3600 * NS)  # evicts nothing
        eng.add_bindings(c.b_node, c.b_ts)
    got = eng.greedy_times(now, ds)
    eng.close()
    return got


def _same(got, want):
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (diff[:5], got[diff[:5]], want[diff[:5]])


@pytest.mark.parametrize("name", list(R.CASES))
def test_targeted(name):
    spec, c, now, ds, want, frozen = R.case(name)
    got = _run(spec, c, now, ds)
    assert got.dtype == np.int64 and got.shape == want.shape
    _same(got, want)
    assert (want != frozen).any()
    assert got[0] == frozen[0]  # pod 0 is crane_dyn_greedy's first placement at now[0]


@pytest.mark.parametrize("edit", [dict(priority=[]), dict(hotValue=[])])
def test_policy_edges(edit):
    spec = dict(cd.default_policy_spec(), **edit)
    c = synth.make_cluster(spec, 300, 200, n_bindings=5000, seed=41, ds_frac=0.1)
    now = R.times(200, 2 * NS)
    _same(_run(spec, c, now, c.ds), R.ref(spec, c, now, c.ds))


def test_no_feasible_node():
    """Every node overloaded and fresh: non-DaemonSet pods get -1, DaemonSet pods still place."""
    spec = dict(cd.default_policy_spec(), predicate=[("cpu_usage_avg_5m", 1e-9)])
    N, P = 200, 300
    c = synth.make_cluster(spec, N, P, n_bindings=2000, seed=62, ds_frac=0.2, invalid=False)
    c.ts[:] = synth.NOW0_NS
    now = int(synth.NOW0_NS) + np.arange(P, dtype=np.int64) * NS
    got = _run(spec, c, now, c.ds)
    _same(got, R.ref(spec, c, now, c.ds))
    assert (got[c.ds == 0] == -1).all() and (got[c.ds == 1] >= 0).all() and c.ds.sum() > 10


@pytest.mark.parametrize("N,P", [(1, 5), (70, 1)])
def test_tiny_shapes(N, P):
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, N, P, n_bindings=40, seed=3, ds_frac=0.3)
    now = R.times(P, 40 * NS)
    _same(_run(spec, c, now, c.ds), R.ref(spec, c, now, c.ds))


def test_no_pods_is_a_noop():
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 30, 4, n_bindings=40, seed=3)
    eng = engine_for(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    got = eng.greedy_times(np.zeros(0, np.int64), np.zeros(0, np.uint8))
    assert got.shape == (0,)
    assert eng.greedy_times(np.zeros(0, np.int64)).shape == (0,)
    now = R.times(4, NS)
    _same(eng.greedy_times(now, c.ds), R.ref(spec, c, now, c.ds))
    eng.close()


def test_pod_times_on_the_edges():
    """Pod times 1 ns before, on and 1 ns after an annotation's expiry (the compare is strict:
    fresh iff now < ts + period + 5 min), and around the whole second at which a log binding
    leaves the 1m window (counted iff ts > unix - 60), with runs of equal times in between."""
    spec = cd.default_policy_spec()
    N = 50
    c = synth.make_cluster(spec, N, 64, n_bindings=600, seed=23, ds_frac=0.1)
    t0 = int(synth.NOW0_NS)
    e_fail, e_prio, _, _ = R.records(spec, c)
    exp = np.concatenate([e_fail] + e_prio)
    edges = []
    for e in np.sort(exp[exp > t0 + 130 * NS])[:3]:  # three (node, metric) expiries after the log part
        edges += [int(e) - 1, int(e), int(e) + 1]
    for ts in np.unique(c.b_ts[c.b_ts > synth.NOW0 - 50])[:3]:  # bindings that leave the 1m window soon
        s = (int(ts) + 60) * NS
        edges += [s - 1, s, s + 1]
    assert len(edges) == 18
    now = np.sort(np.array([t0] * 3 + [t for t in edges for _ in range(3)], np.int64))
    ds = (np.arange(len(now)) % 7 == 3).astype(np.uint8)
    want = R.ref(spec, c, now, ds)
    _same(_run(spec, c, now, ds), want)
    assert (want != R.frozen(spec, c, now, ds)).any()


def test_equal_times_equal_greedy_in_both_forms():
    spec = cd.default_policy_spec()
    N, P = 1000, 3000
    c = synth.make_cluster(spec, N, P, n_bindings=20000, seed=3, ds_frac=0.05)
    now = R.T0
    eng = engine_for(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    got = eng.greedy_times(np.full(P, now, np.int64), c.ds)
    for form in (0, 1):
        eng.set_option("greedy_form", form)
        _same(got, eng.greedy(P, now, c.ds))
    _same(got, eng.greedy_times(np.full(P, now, np.int64), c.ds))
    eng.close()
    assert len(np.unique(got)) > 100


def test_errors():
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 40, 8, n_bindings=100, seed=3)
    eng = cd.Engine(cd.Policy(spec), 0)
    now = R.times(8, NS)
    with pytest.raises(cd.CraneError) as ei:
        eng.greedy_times(now, c.ds)  # no nodes yet
    assert ei.value.code == CRANE_E_STATE
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts)
    eng.upload_bindings(c.b_node, c.b_ts)
    for bad in ([3], [7], [1, 5]):
        t = now.copy()
        t[bad] -= 2 * NS + 1
        with pytest.raises(cd.CraneError) as ei:
            eng.greedy_times(t, c.ds)
        assert ei.value.code == CRANE_E_INVALID, bad
    rc = cd.lib.crane_dyn_greedy_times(eng.h, 8, None, None, None)
    assert rc == CRANE_E_INVALID
    _same(eng.greedy_times(now, c.ds), R.ref(spec, c, now, c.ds))  # the engine still works
    eng.close()


def test_heap_log_and_unordered_log():
    """The heap's slot log (binding_records + add_bindings, nothing evicted) and a shuffled
    uploaded log give the placements of the time-ordered uploaded log."""
    spec, c, now, ds, want, _ = R.case("log_leaves")
    _same(_run(spec, c, now, ds, log="heap"), want)
    import dataclasses
    perm = np.random.default_rng(5).permutation(len(c.b_node))
    cs = dataclasses.replace(c, b_node=c.b_node[perm], b_ts=c.b_ts[perm])
    assert not (np.diff(cs.b_ts) >= 0).all()
    _same(_run(spec, cs, now, ds), want)


def test_engine_left_usable():
    """The binding log is unchanged (hot values at a fixed time as before the call), and an eval
    after re-uploading the nodes recomputes the records."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 500, 50, n_bindings=3000, seed=8)
    eng = engine_for(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    t = int(synth.NOW0_NS) + 30 * NS
    eng.refresh_hot_values(t)
    before = eng.hot_values()
    now = R.times(50, 3 * NS)
    assert (eng.greedy_times(now, c.ds) >= 0).all()
    eng.refresh_hot_values(t)
    assert np.array_equal(eng.hot_values(), before) and before.any()
    eng.upload_nodes(*c.rows(eng.metric_names)[:2], c.hv, c.hv_ts)
    _, _, ch, _ = eng.eval(c.now, c.ds)
    assert np.array_equal(ch, oracle_soa(spec, c, want_matrix=False)[2])
    eng.close()


def test_shard_engine_returns_global_indices():
    spec, c, now, ds, want, _ = R.case("expiries_feedback")
    eng = cd.Engine(cd.Policy(spec), 0)
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts, node_offset=100000)
    got = eng.greedy_times(now, ds)
    eng.close()
    _same(got, np.where(want >= 0, want + 100000, -1))
    assert (want >= 0).any()


def test_between_queue_steps_keys_unchanged():
    """A greedy_times call between two steps of the pipelined queue step (two batches pending):
    after the flush every batch's keys equal a run without the call, and the call's placements
    are the reference's."""
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 5000, 1500, n_bindings=40000, seed=51)
    dev = torch.device("cuda", 0)
    t0 = int(synth.NOW0_NS)
    times = [t0 + (k % 4) * 9_000_000_000 for k in range(5)]
    d_flags = torch.from_numpy(c.ds).to(dev)
    d_now = [torch.from_numpy(c.now + (t - t0)).to(dev) for t in times]
    torch.cuda.synchronize()
    gnow, gds = R.times(64, 2 * NS), c.ds[:64]
    keys, placed = {}, None
    for call in (False, True):
        eng = engine_for(spec, c, opts={"step_defer": 2})
        eng.upload_bindings(c.b_node, c.b_ts)
        q = cd.Queue(0)
        bufs = [torch.empty(1500, dtype=torch.int64, device=dev) for _ in times]
        for b, t in enumerate(times):
            if call and b == 3:
                placed = eng.greedy_times(gnow, gds)
            eng.step_keys_queue(t, t, d_now[b], d_flags, bufs[b], q)
        eng.step_flush()
        q.wait()
        keys[call] = [k.cpu().numpy() for k in bufs]
        eng.close()
        q.close()
    for b in range(len(times)):
        assert np.array_equal(keys[True][b], keys[False][b]), b
    _same(placed, R.ref(spec, c, gnow, gds))
