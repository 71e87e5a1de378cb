"""Sequential-greedy placement (crane_dyn_greedy) vs the oracle's or_greedy.

Each placement is a Binding{Timestamp: now} on the chosen node, which raises
its window counts / hot value (binding.go:81-97, node.go:113-121) before the
next pod is scored (plugins.go:73-98).  Bit-exact chosen nodes.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import engine_for  # noqa: E402
from oracle import oracle as O  # noqa: E402


_OPTS = {}


@pytest.fixture(autouse=True, params=["merge", "seq"])
def greedy_mode(request):
    """merge: merge.hip (default); seq: the one-workgroup sequential kernel (greedy.hip)."""
    _OPTS["greedy_form"] = 0 if request.param == "merge" else 1
    yield request.param
    _OPTS.clear()


def _engine(spec, c=None):
    return engine_for(spec, c, opts=_OPTS)


def _oracle(spec, c, P, now):
    return O.greedy(spec, c.metric_names, c.ok, c.val, np.where(c.ok == 1, c.ts, 0), c.b_node, c.b_ts, now, P,
                    c.ds[:P])


@pytest.mark.parametrize("N,P,B,seed", [(1, 5, 0, 1), (64, 200, 1000, 2), (1000, 3000, 20000, 3),
                                        (4097, 2000, 50000, 4), (20000, 5000, 200000, 5),
                                        (262145, 300, 100000, 6)])
def test_greedy_vs_oracle(N, P, B, seed):
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, N, P, n_bindings=B, seed=seed, ds_frac=0.05)
    now = int(synth.NOW0_NS) + 1234567
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    ch = eng.greedy(P, now, c.ds)
    och = _oracle(spec, c, P, now)
    assert np.array_equal(ch, och)


def test_greedy_global_leaves():
    """N above the LDS leaf capacity: leaves stay in global memory."""
    spec = cd.default_policy_spec()
    N, P = 200_000, 3000
    c = synth.make_cluster(spec, N, P, n_bindings=100_000, seed=9)
    now = int(synth.NOW0_NS)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    ch = eng.greedy(P, now, c.ds)
    assert np.array_equal(ch, _oracle(spec, c, P, now))


def test_greedy_edge_policies():
    m = 60 * 10**9
    base = cd.default_policy_spec()
    specs = [dict(base, priority=[]), dict(base, hotValue=[]), dict(base, hotValue=[(0, 1), (-60 * m, 2), (30 * m, -3)])]
    for i, spec in enumerate(specs):
        c = synth.make_cluster(spec, 300, 400, n_bindings=5000, seed=40 + i)
        now = int(synth.NOW0_NS)
        eng = _engine(spec, c)
        eng.upload_bindings(c.b_node, c.b_ts)
        ch = eng.greedy(400, now, c.ds)
        assert np.array_equal(ch, _oracle(spec, c, 400, now)), i


def test_greedy_then_eval_consistent():
    """greedy leaves the engine usable: a later eval recomputes node records."""
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 500, 50, n_bindings=3000, seed=8)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    eng.greedy(50, int(c.now[0]), c.ds)
    eng.upload_nodes(*c.rows(eng.metric_names)[:2], c.hv, c.hv_ts)
    _, _, ch, _ = eng.eval(c.now, c.ds)
    from helpers import oracle_soa
    want = oracle_soa(spec, c, want_matrix=False)[2]
    if not np.array_equal(ch, want):
        # diagnostics (a mismatch seen once was the first-batch state race that
        # test_first_step_batch_of_fresh_engines covers): does it persist, in which path?
        _, _, ch2, _ = eng.eval(c.now, c.ds)
        eng.set_option("keys_path", 1)
        _, _, ch3, _ = eng.eval(c.now, c.ds)
        pytest.fail(f"eval after greedy: got {ch[:4]} want {want[:4]}; again {ch2[:4]}; matrix path {ch3[:4]}")


@pytest.mark.parametrize("ds_frac,feas_all", [(0.0, False), (1.0, False), (0.3, False), (0.02, True)])
def test_greedy_daemonset_mixes(ds_frac, feas_all):
    """DaemonSet pods take the best of the feasible (F) and infeasible (I) streams."""
    spec = cd.default_policy_spec()
    if feas_all:
        spec = dict(spec, predicate=[])
    N, P = 3000, 4000
    c = synth.make_cluster(spec, N, P, n_bindings=30000, seed=61, ds_frac=ds_frac)
    now = int(synth.NOW0_NS)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    assert np.array_equal(eng.greedy(P, now, c.ds), _oracle(spec, c, P, now))


def test_greedy_no_feasible_node():
    """Every node overloaded: non-DaemonSet pods get -1, DaemonSet pods still place."""
    spec = dict(cd.default_policy_spec(), predicate=[("cpu_usage_avg_5m", 1e-9)])
    N, P = 200, 500
    c = synth.make_cluster(spec, N, P, n_bindings=2000, seed=62, ds_frac=0.2, invalid=False)
    c.ts[:] = synth.NOW0_NS  # all fresh, so every node is over the tiny limit
    now = int(synth.NOW0_NS)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    ch = eng.greedy(P, now, c.ds)
    assert np.array_equal(ch, _oracle(spec, c, P, now))
    assert (ch[c.ds[:P] == 0] == -1).all()


def test_greedy_many_pods_per_node():
    """P >> N: every node runs down its staircase to score 0."""
    spec = cd.default_policy_spec()
    N, P = 37, 3000
    c = synth.make_cluster(spec, N, P, n_bindings=500, seed=63, ds_frac=0.05)
    now = int(synth.NOW0_NS)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    assert np.array_equal(eng.greedy(P, now, c.ds), _oracle(spec, c, P, now))


def test_greedy_windows_shapes():
    """Zero-length window (bindings stamped now never count), several counts, one window."""
    m = 60 * 10**9
    base = cd.default_policy_spec()
    for i, hot in enumerate([[(0, 2), (5 * m, 5)], [(5 * m, 3), (1 * m, 7), (10 * m, 1)], [(2 * m, 1)]]):
        spec = dict(base, hotValue=hot)
        c = synth.make_cluster(spec, 800, 1500, n_bindings=20000, seed=70 + i, ds_frac=0.05)
        now = int(synth.NOW0_NS)
        eng = _engine(spec, c)
        eng.upload_bindings(c.b_node, c.b_ts)
        assert np.array_equal(eng.greedy(1500, now, c.ds), _oracle(spec, c, 1500, now)), i


@pytest.mark.slow
def test_greedy_config5_merge_equals_sequential(greedy_mode):
    """BASELINE config 5 size (100k nodes x 50k pods): merge form == sequential kernel, bit for bit."""
    if greedy_mode != "merge":
        pytest.skip("compares both modes itself")
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 100_000, 50_000, n_bindings=1_000_000, seed=20255215)
    now = int(synth.NOW0_NS)
    eng = _engine(spec, c)
    eng.upload_bindings(c.b_node, c.b_ts)
    a = eng.greedy(50_000, now, c.ds)
    eng.set_option("greedy_form", 1)
    b = eng.greedy(50_000, now, c.ds)
    assert np.array_equal(a, b)
    assert (a >= 0).all()
    # placement i depends only on placements < i: the first 2,000 of the full run equal the
    # oracle's sequential loop over the same cluster cut at 2,000 pods
    assert np.array_equal(a[:2000], _oracle(spec, c, 2000, now))


def test_first_step_batch_of_fresh_engines():
    """The step path's batch state ({tmin, tmax, tile counter}) is zeroed on the engine stream
    and waited for before the first K3p: a null-stream memset raced the first batch once (every
    pod then scored as at time 0).  Forty fresh engines, each checked on its first batch."""
    spec = cd.default_policy_spec()
    for i in range(40):
        c = synth.make_cluster(spec, 500, 50, n_bindings=0, seed=100 + i)
        eng = _engine(spec, c)
        _, _, ch, _ = eng.eval(c.now, c.ds)
        from helpers import oracle_soa
        assert np.array_equal(ch, oracle_soa(spec, c, want_matrix=False)[2]), i
