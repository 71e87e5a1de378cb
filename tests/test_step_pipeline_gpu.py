"""The pipelined queue step (engine option step_defer 2, the group's default "defer" 2;
csrc/step.hip step_one_launch): a step on a dispatch queue is one launch holding this batch's K2 +
K3p, the previous batch's K1 and the K3s of the batch before, so two batches stay pending on the
engine.  Every test compares a batch's keys bit for bit (torch.equal) with the same batch stepped
by a second engine on a HIP stream (the path the oracle tests pin): through filling, steady state
and draining of the pipeline, the key-buffer patterns, the first launches that cannot take the
form, state changes and batch-size changes in between, and the group.  Seven scenarios also pin the
packets each step wrote (PARENT_PACKETS): which launches a step takes, not only what they compute.
Shapes: 5,000 nodes = 20 K1 blocks (the last partial, >= 8 so K3s's XCD grouping is on), 1,500
pods = two pod tiles (the second partial), 40,000 bindings, the default policy.
Reference: plugins.go:39-98 + selectHost; binding.go:81-97."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import shard, synth  # noqa: E402
from helpers import oracle_soa  # noqa: E402
from oracle import oracle as O  # noqa: E402

N_NODES, N_PODS, N_BIND = 5000, 1500, 40000
T0 = int(synth.NOW0_NS)
STEP_NS = 9_000_000_000


def _engine(spec, c, opts=()):
    e = cd.Engine(cd.Policy(spec), 0)
    for k, v in opts:
        e.set_option(k, v)
    val, ts, _ = c.rows(e.metric_names)
    e.upload_nodes(val, ts, c.hv, c.hv_ts)
    e.upload_bindings(c.b_node, c.b_ts)
    return e


@pytest.fixture(scope="module")
def world():
    """The cluster, the pods (2,500: tests take prefixes) and a cache of reference keys per
    (batch time, pod count), each stepped once by one stream engine and never changed."""
    import torch
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, N_NODES, 2500, n_bindings=N_BIND, seed=20251020)
    c.now, c.ds = synth.make_pods(2500, seed=20251021)
    dev = torch.device("cuda", 0)
    eng = _engine(spec, c)
    st = torch.cuda.Stream(dev)
    d_flags = torch.from_numpy(c.ds).to(dev)
    cache = {}

    def now_dev(t, P=N_PODS):
        return torch.from_numpy(c.now[:P] + (t - T0)).to(dev)

    def ref(t, P=N_PODS):
        if (t, P) not in cache:
            d_now = now_dev(t, P)
            k = torch.empty(P, dtype=torch.int64, device=dev)
            torch.cuda.synchronize()
            eng.step_keys_async(t, t, d_now, d_flags[:P], k, st.cuda_stream)
            st.synchronize()
            cache[(t, P)] = k
        return cache[(t, P)]

    class W:
        pass
    w = W()
    w.spec, w.c, w.dev, w.d_flags, w.now_dev, w.ref = spec, c, dev, d_flags, now_dev, ref
    yield w
    eng.close()


def _times(n):
    return [T0 + (k % 4) * STEP_NS for k in range(n)]


# Packets written per step, recorded from the parent of the change that gathered the queue step's
# pending state and launch choice in one place (commit b375471), on an MI355X: the literals are
# that commit's, not the code under test's, so a drift in which launches a step takes fails here.
PARENT_PACKETS = {
    "fill_steady_drain_9": [4, 1, 1, 1, 1, 1, 1, 1, 1],
    "same_buffer_twice_running": [4, 1, 1, 1, 1, 3, 1, 1, 1],
    "other_first_launches_k2_form": [4, 5, 5, 5, 5, 5],
    "other_first_launches_k2_delta": [2, 3, 3, 3, 3, 3],
    "step_defer_1_two_alternating_buffers": [4, 2, 2, 2, 2, 2],
    "reanchor_and_upload_between_steps": [4, 1, 1, 1, 6, 1, 4, 1, 4, 1],
    "batch_size_changes_on_one_queue": [4, 1, 1, 3, 1, 1, 3, 1, 1, 3, 1],
}


def _pinned(name, packets):
    print(f"packets[{name!r}] = {packets}")
    assert packets == PARENT_PACKETS[name], (name, packets)


def _run(w, eng, q, times, bufs, P=N_PODS, between=None):
    """Batch b at times[b] into bufs[b] on the queue; between(b) runs before batch b's step."""
    import torch
    d_now = [w.now_dev(t, P) for t in times]
    torch.cuda.synchronize()
    packets = []
    for b, t in enumerate(times):
        if between:
            between(b)
        before = q.packets()
        eng.step_keys_queue(t, t, d_now[b], w.d_flags[:P], bufs[b], q)
        packets.append(q.packets() - before)
    return packets


@pytest.mark.parametrize("n", [1, 2, 3, 4, 9])
def test_fill_steady_drain(world, n):
    """n batches at advancing times, each with its own key buffer, then step_flush + wait: the
    pipeline only fills (1, 2), reaches its steady state (3, 4, 9) and drains; every batch equals
    the stream engine's."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    times = _times(n)
    bufs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]
    packets = _run(w, eng, q, times, bufs)
    eng.step_flush()
    q.wait()
    for b, t in enumerate(times):
        assert torch.equal(bufs[b], w.ref(t)), f"batch {b} of {n}"
    if n == 9:
        _pinned("fill_steady_drain_9", packets)
    eng.close()
    q.close()


def test_two_alternating_buffers_one_packet_per_step(world):
    """The bench's pattern: two key buffers in alternation on one queue over 9 batches.  The last
    two batches' buffers equal the reference, and from the third batch on each step wrote exactly
    one packet (no drain: the keys' reset moved out of K3p)."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    times = _times(9)
    two = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in range(2)]
    bufs = [two[b % 2] for b in range(9)]
    packets = _run(w, eng, q, times, bufs)
    eng.step_flush()
    q.wait()
    assert torch.equal(bufs[7], w.ref(times[7]))
    assert torch.equal(bufs[8], w.ref(times[8]))
    assert packets[2:] == [1] * 7, packets
    eng.close()
    q.close()


def test_same_buffer_twice_running(world):
    """Batch 5 reuses batch 4's buffer (what is pending runs alone first): batch 5's keys come out
    whole, every other batch but the overwritten 4 equals the reference."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    times = _times(9)
    bufs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]
    bufs[5] = bufs[4]
    packets = _run(w, eng, q, times, bufs)
    eng.step_flush()
    q.wait()
    for b, t in enumerate(times):
        if b != 4:
            assert torch.equal(bufs[b], w.ref(t)), f"batch {b}"
    _pinned("same_buffer_twice_running", packets)
    eng.close()
    q.close()


@pytest.mark.parametrize("opts", [(("k2_form", 3),), (("k2_delta", 0),)], ids=["large", "dedupe"])
def test_other_first_launches_fall_back(world, opts):
    """First launches that are not the delta form, with step_defer 2: the two-launch form."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, opts + (("step_defer", 2),))
    q = cd.Queue(0)
    times = _times(6)
    bufs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]
    packets = _run(w, eng, q, times, bufs)
    eng.step_flush()
    q.wait()
    for b, t in enumerate(times):
        assert torch.equal(bufs[b], w.ref(t)), f"batch {b}"
    _pinned("other_first_launches_" + opts[0][0], packets)
    eng.close()
    q.close()


def test_step_defer_1_two_alternating_buffers(world):
    """Option step_defer 1 (a step leaves only its K3s to the next one's first launch): six batches
    on one queue into two key buffers in alternation.  The last two batches' buffers equal the
    reference, and the packets per step are the recorded ones."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 1),))
    q = cd.Queue(0)
    times = _times(6)
    two = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in range(2)]
    bufs = [two[b % 2] for b in range(6)]
    packets = _run(w, eng, q, times, bufs)
    eng.step_flush()
    q.wait()
    assert torch.equal(bufs[4], w.ref(times[4]))
    assert torch.equal(bufs[5], w.ref(times[5]))
    _pinned("step_defer_1_two_alternating_buffers", packets)
    eng.close()
    q.close()


def test_reanchor_and_upload_between_steps(world):
    """Time jumps while two batches are pending: + 120 s forces the delta form to re-anchor (batch
    4: the bindings' stamps span 600 s, so the changed ones pass half the widest window's suffix),
    + 3,000 s leaves no binding in any window (batch 6: K1 reads the adjustments as the anchor),
    and back (batch 7 re-anchors again); then an upload_nodes between two steps (before batch 8).
    Every batch equals the reference."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    times = _times(10)
    times[4] = times[5] = T0 + 120 * 10**9
    times[6] = T0 + 3000 * 10**9
    bufs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]

    def between(b):
        if b == 8:
            val, ts, _ = w.c.rows(eng.metric_names)
            eng.upload_nodes(val, ts, w.c.hv, w.c.hv_ts)
    packets = _run(w, eng, q, times, bufs, between=between)
    eng.step_flush()
    q.wait()
    for b, t in enumerate(times):
        assert torch.equal(bufs[b], w.ref(t)), f"batch {b}"
    _pinned("reanchor_and_upload_between_steps", packets)
    eng.close()
    q.close()


def test_batch_size_changes_on_one_queue(world):
    """P = 700, 1,500, 2,500 (1 -> 2 -> 3 pod tiles), then back to 700, on one queue with no flush
    by the caller in between: the stages pending for the old size run before the plan for the new
    one may reallocate the buffers they point into.  All batches equal the reference."""
    import torch
    w = world
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    sizes = [700, 700, 700, 1500, 1500, 1500, 2500, 2500, 2500, 700, 700]
    times = _times(len(sizes))
    d_now = [w.now_dev(t, P) for t, P in zip(times, sizes)]
    bufs = [torch.empty(P, dtype=torch.int64, device=w.dev) for P in sizes]
    torch.cuda.synchronize()
    packets = []
    for b, (t, P) in enumerate(zip(times, sizes)):
        before = q.packets()
        eng.step_keys_queue(t, t, d_now[b], w.d_flags[:P], bufs[b], q)
        packets.append(q.packets() - before)
    eng.step_flush()
    q.wait()
    for b, (t, P) in enumerate(zip(times, sizes)):
        assert torch.equal(bufs[b], w.ref(t, P)), f"batch {b} (P={P})"
    _pinned("batch_size_changes_on_one_queue", packets)
    eng.close()
    q.close()


def test_group_default_defer(world):
    """The group, depth 4 on one device with its default options (defer 2): 13 batches over a
    6-time cycle into 2 x depth key buffers as the bench hands them out, then sync.  The last
    2 x depth batches equal the stream engine's, and a 32-pod sample of the last batch equals the
    oracle with the binding log's hot values at that batch's time."""
    import torch
    w, c = world, world.c
    depth = 4
    g = cd.Group(cd.Policy(w.spec), devices=[0], depth=depth)
    g.set_option("collective", 0)
    val, ts, _ = c.rows(g.metric_names)
    g.upload_nodes(val, ts, c.hv, c.hv_ts)
    g.upload_bindings(c.b_node, c.b_ts)
    times = [T0 + (k % 6) * STEP_NS for k in range(13)]
    d_now = [w.now_dev(t) for t in times]
    d_flags = [w.d_flags[:N_PODS].clone()]
    kb = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in range(2 * depth)]
    torch.cuda.synchronize()
    for b, t in enumerate(times):
        g.step_keys_async(t, t, [d_now[b]], d_flags, [kb[b % (2 * depth)]])
    g.sync()
    for b in range(len(times) - 2 * depth, len(times)):
        assert torch.equal(kb[b % (2 * depth)], w.ref(times[b])), f"batch {b}"
    b = len(times) - 1
    got = kb[b % (2 * depth)].cpu().numpy()
    smp = np.unique(np.concatenate([np.linspace(0, N_PODS - 1, 24).astype(int), np.flatnonzero(c.ds[:N_PODS])[:8]]))
    _, hv = O.hot_values(w.spec, c.b_node, c.b_ts, c.n_nodes, times[b] // 10**9)
    off, osc, och = oracle_soa(w.spec, c, now=(c.now[:N_PODS] + (times[b] - T0))[smp], ds=c.ds[smp],
                               hv_override=(hv.astype(np.float64), np.full(c.n_nodes, times[b], np.int64)))
    node, score = shard.unpack_keys(got[smp])
    assert np.array_equal(node, och)
    for i in range(len(smp)):
        feas = (off[i] < 0) | (c.ds[smp[i]] != 0)
        assert score[i] == (osc[i][feas].max() if feas.any() else -1), i
    g.close()


def test_option_plumbing(world):
    """step_defer 0 / 1 / 2 on the engine and defer 0 / 1 / 2 on the group: one batch followed by
    the flush / sync gives the same keys in all three."""
    import torch
    w, c = world, world.c
    t = T0 + STEP_NS
    d_now = w.now_dev(t)
    torch.cuda.synchronize()
    for v in (0, 1, 2):
        eng = _engine(w.spec, c, (("step_defer", v),))
        q = cd.Queue(0)
        k = torch.empty(N_PODS, dtype=torch.int64, device=w.dev)
        eng.step_keys_queue(t, t, d_now, w.d_flags[:N_PODS], k, q)
        eng.step_flush()
        q.wait()
        assert torch.equal(k, w.ref(t)), f"engine step_defer {v}"
        eng.close()
        q.close()
        g = cd.Group(cd.Policy(w.spec), devices=[0], depth=2)
        g.set_option("collective", 0)
        g.set_option("defer", v)
        val, ts, _ = c.rows(g.metric_names)
        g.upload_nodes(val, ts, c.hv, c.hv_ts)
        g.upload_bindings(c.b_node, c.b_ts)
        k = torch.empty(N_PODS, dtype=torch.int64, device=w.dev)
        g.step_keys_async(t, t, [d_now], [w.d_flags[:N_PODS].clone()], [k])
        g.sync()
        assert torch.equal(k, w.ref(t)), f"group defer {v}"
        g.close()
    with pytest.raises(cd.CraneError):
        _engine(w.spec, c, (("step_defer", 3),))


def test_policy_with_fewer_terms(world):
    """A policy of 4 predicates and 5 priorities takes the kernel's instance for any policy of the
    4 x 6 record shape (the default policy has one of its own): fill, steady state with two
    alternating buffers, drain, against a stream engine with the same policy."""
    import torch
    w = world
    spec = cd.default_policy_spec()
    spec["priority"] = spec["priority"][:5]
    c = synth.make_cluster(spec, N_NODES, N_PODS, n_bindings=N_BIND, seed=20251022)
    c.now, c.ds = synth.make_pods(N_PODS, seed=20251023)
    ref_eng, eng = _engine(spec, c), _engine(spec, c, (("step_defer", 2),))
    q = cd.Queue(0)
    st = torch.cuda.Stream(w.dev)
    times = _times(6)
    d_flags = torch.from_numpy(c.ds).to(w.dev)
    d_now = [torch.from_numpy(c.now + (t - T0)).to(w.dev) for t in times]
    bufs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]
    refs = [torch.empty(N_PODS, dtype=torch.int64, device=w.dev) for _ in times]
    torch.cuda.synchronize()
    packets = []
    for b, t in enumerate(times):
        ref_eng.step_keys_async(t, t, d_now[b], d_flags, refs[b], st.cuda_stream)
        before = q.packets()
        eng.step_keys_queue(t, t, d_now[b], d_flags, bufs[b], q)
        packets.append(q.packets() - before)
    st.synchronize()
    eng.step_flush()
    q.wait()
    for b in range(len(times)):
        assert torch.equal(bufs[b], refs[b]), f"batch {b}"
    assert packets[2:] == [1] * 4, packets
    for e in (ref_eng, eng):
        e.close()
    q.close()
