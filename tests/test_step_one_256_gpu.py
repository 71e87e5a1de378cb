"""The one-launch queue step in 256-lane workgroups (csrc/step.hip step_one_launch): K3s at four
pods per lane with its item lists and its final pass in two halves, K3p at four pods per lane,
the delta form in chunks of 512 changed bindings (2,048 hash slots, csrc/lds_hash.hpp), and the
keys of K1's batch reset by workgroups of their own.  As tests/test_step_pipeline_gpu.py: every
batch's keys are compared bit for bit (torch.equal) with the same batch stepped by a second engine
on a HIP stream; engine option step_defer 2 on a cd.Queue, two key buffers in alternation over 6
batches, and exactly one packet per step from the third batch on (the one-launch form ran, not
the two-launch fallback).
Shapes: 1, 255, 257, 700, 1,024, 1,025, 2,500 pods (lanes with 0 to 4 live pods, an exact tile, a
partial second and third tile; DaemonSet pods as synth.make_pods makes them); 300 nodes (two K1
blocks, the last partial) and 1,000 (four: fewer than 8, no XCD grouping) — the older tests run
5,000 (20 blocks); binding logs of 4,000 and 40,000 stamps over 600 s: with batch times 9 s apart
the changed bindings per step stay below one 512-binding chunk in the first and pass two chunks
in the second (counted on the host as bench.delta_changed does, and asserted).
Reference: plugins.go:39-98 + selectHost; binding.go:81-97."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402

T0 = int(synth.NOW0_NS)
STEP_NS = 9_000_000_000
CHUNK = 512  # changed bindings per delta workgroup of the one-launch step (kStepOneDeltaChunk)
PODS = [1, 255, 257, 700, 1024, 1025, 2500]
NODES = [300, 1000]
BINDINGS = [4000, 40000]
MAX_PODS = 2500


def _engine(spec, c, opts=()):
    e = cd.Engine(cd.Policy(spec), 0)
    for k, v in opts:
        e.set_option(k, v)
    val, ts, _ = c.rows(e.metric_names)
    e.upload_nodes(val, ts, c.hv, c.hv_ts)
    e.upload_bindings(c.b_node, c.b_ts)
    return e


def _times(n):
    return [T0 + (k % 4) * STEP_NS for k in range(n)]


def changed_bindings(spec, b_ts, nows):
    """Per batch time, the bindings whose window rank differs from the anchor refresh's (the first
    batch time): the merged ranges between the windows' suffix starts (bench.delta_changed)."""
    trs = sorted(tr // 10**9 for tr, _ in spec["hotValue"])

    def starts(now_ns):
        cut = np.sort(np.array([now_ns // 10**9 - t for t in trs], np.int64))
        return np.searchsorted(b_ts, cut, side="right")

    a = starts(nows[0])
    out = []
    for n in nows:
        p = starts(n)
        rg = sorted((min(x, y), max(x, y)) for x, y in zip(a, p) if x != y)
        tot, end = 0, -1
        for lo, hi in rg:
            lo = max(lo, end)
            if hi > lo:
                tot += hi - lo
            end = max(end, hi)
        out.append(int(tot))
    return out


class World:
    """A cluster with its binding log, 2,500 pods (tests take prefixes) and the reference keys per
    (batch time, pod count), each stepped once by one stream engine and never changed."""

    def __init__(self, n_nodes, n_bind):
        import torch
        self.spec = cd.default_policy_spec()
        self.c = synth.make_cluster(self.spec, n_nodes, MAX_PODS, n_bindings=n_bind, seed=20261020 + n_nodes + n_bind)
        self.c.now, self.c.ds = synth.make_pods(MAX_PODS, seed=20261021)
        self.dev = torch.device("cuda", 0)
        self.eng = _engine(self.spec, self.c)
        self.st = torch.cuda.Stream(self.dev)
        self.d_flags = torch.from_numpy(self.c.ds).to(self.dev)
        self.cache = {}

    def now_dev(self, t, P):
        import torch
        return torch.from_numpy(self.c.now[:P] + (t - T0)).to(self.dev)

    def ref(self, t, P):
        import torch
        if (t, P) not in self.cache:
            d_now = self.now_dev(t, P)
            k = torch.empty(P, dtype=torch.int64, device=self.dev)
            torch.cuda.synchronize()
            self.eng.step_keys_async(t, t, d_now, self.d_flags[:P], k, self.st.cuda_stream)
            self.st.synchronize()
            self.cache[(t, P)] = k
        return self.cache[(t, P)]


@pytest.fixture(scope="module")
def worlds():
    made = {}

    def get(n_nodes, n_bind):
        if (n_nodes, n_bind) not in made:
            made[(n_nodes, n_bind)] = World(n_nodes, n_bind)
        return made[(n_nodes, n_bind)]

    yield get
    for w in made.values():
        w.eng.close()


def _steps(w, eng, q, times, sizes, bufs):
    """Batch b of sizes[b] pods at times[b] into bufs[b] on the queue; packets written per step."""
    import torch
    d_now = [w.now_dev(t, P) for t, P in zip(times, sizes)]
    torch.cuda.synchronize()
    packets = []
    for b, (t, P) in enumerate(zip(times, sizes)):
        before = q.packets()
        eng.step_keys_queue(t, t, d_now[b], w.d_flags[:P], bufs[b], q)
        packets.append(q.packets() - before)
    return packets


@pytest.mark.parametrize("n_nodes", NODES)
def test_changed_bindings_cross_the_chunk(worlds, n_nodes):
    """The two binding logs put the delta form's work per step on both sides of its chunk: the small
    log's steps all stay below one 512-binding chunk (one partial workgroup, or none), the large
    log has steps past two chunks (three workgroups and more).  Without both, the cases below
    would pass without crossing a chunk boundary."""
    small = changed_bindings(cd.default_policy_spec(), worlds(n_nodes, BINDINGS[0]).c.b_ts, _times(6))
    large = changed_bindings(cd.default_policy_spec(), worlds(n_nodes, BINDINGS[1]).c.b_ts, _times(6))
    assert 0 < max(small) < CHUNK, small
    assert max(large) > 2 * CHUNK, large


@pytest.mark.parametrize("n_bind", BINDINGS)
@pytest.mark.parametrize("n_nodes", NODES)
@pytest.mark.parametrize("P", PODS)
def test_two_buffers_six_batches(worlds, P, n_nodes, n_bind):
    """Six batches of P pods into two alternating key buffers (the keys' reset rides beside K1):
    the last two batches' buffers equal the stream engine's.  Then the same six batches with a
    buffer each (K3p resets the keys): every batch equals it.  In both, each step from the third
    batch on wrote exactly one packet."""
    import torch
    w = worlds(n_nodes, n_bind)
    times = _times(6)
    sizes = [P] * 6
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    two = [torch.empty(P, dtype=torch.int64, device=w.dev) for _ in range(2)]
    bufs = [two[b % 2] for b in range(6)]
    packets = _steps(w, eng, q, times, sizes, bufs)
    eng.step_flush()
    q.wait()
    assert packets[2:] == [1] * 4, packets
    assert torch.equal(bufs[4], w.ref(times[4], P)), "batch 4"
    assert torch.equal(bufs[5], w.ref(times[5], P)), "batch 5"
    eng.close()
    q.close()
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    bufs = [torch.empty(P, dtype=torch.int64, device=w.dev) for _ in range(6)]
    packets = _steps(w, eng, q, times, sizes, bufs)
    eng.step_flush()
    q.wait()
    assert packets[2:] == [1] * 4, packets
    for b, t in enumerate(times):
        assert torch.equal(bufs[b], w.ref(t, P)), f"batch {b}"
    eng.close()
    q.close()


@pytest.mark.parametrize("n_bind", BINDINGS)
@pytest.mark.parametrize("sizes", [(1024, 1025, 700), (2500, 1024, 257)], ids=["up_down", "down"])
def test_pod_count_changes_across_a_tile(worlds, sizes, n_bind):
    """Three groups of four batches, the pod count changing across a tile boundary between groups
    (1,024 -> 1,025: one tile to two; -> 700: back to one; 2,500 -> 1,024 -> 257: three, one, one),
    each group on its own two alternating key buffers, no flush by the caller in between: the
    stages pending for the old size drain as launches without pod tiles or delta chunks that
    still carry a K1 and its batch's key reset.  The last two batches of every group equal the
    stream engine's."""
    import torch
    w = worlds(1000, n_bind)
    eng = _engine(w.spec, w.c, (("step_defer", 2),))
    q = cd.Queue(0)
    per = [P for P in sizes for _ in range(4)]
    times = _times(len(per))
    two = {P: [torch.empty(P, dtype=torch.int64, device=w.dev) for _ in range(2)] for P in sizes}
    bufs = [two[P][b % 2] for b, P in enumerate(per)]
    _steps(w, eng, q, times, per, bufs)
    eng.step_flush()
    q.wait()
    for g in range(len(sizes)):
        for b in (4 * g + 2, 4 * g + 3):
            assert torch.equal(bufs[b], w.ref(times[b], per[b])), f"batch {b} (P={per[b]})"
    eng.close()
    q.close()


def test_time_jump_past_the_resident_launch(worlds):
    """A step whose changed bindings pass what one resident launch holds (7 workgroups per compute
    unit, 512 changed bindings per delta workgroup) keeps its launches apart: what is pending runs
    first and the delta form goes out alone.  300 nodes, 257 pods; a time-ordered log uniform over
    the 300 s of the widest window before the first batch, dense enough that batch 4's jump of 55 s
    changes more than 7 * CUs * 512 bindings against the anchor (asserted, counted on the host)
    while staying at most half the widest window's suffix (asserted: the step does not re-anchor);
    the other batches are 1 s apart and back near the anchor.  Batch 4 writes more than one
    packet, batches 2, 3 and 5 to 7 exactly one, and every batch equals the stream engine's."""
    import torch
    P, jump = 257, 55
    base = worlds(300, BINDINGS[0])
    limit = 7 * torch.cuda.get_device_properties(0).multi_processor_count * CHUNK
    rate = -(-103 * limit // (100 * 2 * jump))  # bindings per second: 2 * jump * rate = 1.03 * limit
    rng = np.random.default_rng(20261022)
    t0s = T0 // 10**9
    b_ts = np.sort(rng.integers(t0s - 300, t0s + 1, 300 * rate)).astype(np.int64)
    b_node = rng.integers(0, 300, b_ts.size).astype(np.int32)
    times = [T0 + s * 10**9 for s in (0, 1, 2, 3, jump, 1, 2, 3)]
    changed = changed_bindings(base.spec, b_ts, times)
    widest = max(tr for tr, _ in base.spec["hotValue"]) // 10**9
    suffix = b_ts.size - int(np.searchsorted(b_ts, times[4] // 10**9 - widest, side="right"))
    assert changed[4] > limit, (changed, limit)
    assert 2 * changed[4] <= suffix, (changed, suffix)
    assert max(changed[:4] + changed[5:]) < limit // 8, changed

    def engine(opts=()):
        e = cd.Engine(cd.Policy(base.spec), 0)
        for k, v in opts:
            e.set_option(k, v)
        val, ts, _ = base.c.rows(e.metric_names)
        e.upload_nodes(val, ts, base.c.hv, base.c.hv_ts)
        e.upload_bindings(b_node, b_ts)
        return e

    ref_eng, eng = engine(), engine((("step_defer", 2),))
    q = cd.Queue(0)
    d_now = [base.now_dev(t, P) for t in times]
    bufs = [torch.empty(P, dtype=torch.int64, device=base.dev) for _ in times]
    refs = [torch.empty(P, dtype=torch.int64, device=base.dev) for _ in times]
    torch.cuda.synchronize()
    for b, t in enumerate(times):
        ref_eng.step_keys_async(t, t, d_now[b], base.d_flags[:P], refs[b], base.st.cuda_stream)
    base.st.synchronize()
    packets = []
    for b, t in enumerate(times):
        before = q.packets()
        eng.step_keys_queue(t, t, d_now[b], base.d_flags[:P], bufs[b], q)
        packets.append(q.packets() - before)
    eng.step_flush()
    q.wait()
    print(f"changed {changed} limit {limit} suffix {suffix} packets {packets}")
    assert packets[4] > 1 and packets[2:4] == [1, 1] and packets[5:] == [1, 1, 1], packets
    for b in range(len(times)):
        assert torch.equal(bufs[b], refs[b]), f"batch {b}"
    for e in (ref_eng, eng):
        e.close()
    q.close()
