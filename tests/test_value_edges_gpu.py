"""Out-of-domain usages and hot values through every consumer of a node's score, bit for bit
against the CPU oracle (plugins.go:39-98, stats.go:51-138, binding.go:81-97, node.go:113-121).

The inputs are helpers.edge_cluster's: NaN, +-Inf, 1e300, 1e17, |q| around 2^31, signed zero,
denormal, limit +- 1 ulp usages and NaN, +-Inf, >= 2^63 / 10, ~2^31 / 10, fractional, negative hot
values on a seeded share of nodes, many of them expiring inside the batch range.  The device states
the reference's conversion-and-wrap rule (int(float64) as CVTTSD2SQ, the wrapping int64
subtraction, the clamp) once per consumer — see go_int in csrc/node_rec.hpp for the list — and each
test here drives one of them: the per-pair kernel (matrices, int8 matrices, keys), the step path
on a stream and on a dispatch queue (streamed and fused node pass, K3s), top-k, the filter
diagnosis, selection, the answer tables, the scatter update, and greedy in both forms.
tests/test_value_edges.py asserts, from the oracle alone, that these worlds are live: edge nodes
win pods, every class decides some result, edge nodes step inside the batch."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import (EDGE_TIMES, GREEDY_NOW, SELECT_CASES, SH, edge_annotations, edge_world, engine_for,  # noqa: E402
                     greedy_oracle, greedy_world, keys_node_score, oracle_soa, select_ext)
from oracle import oracle as O  # noqa: E402
from oracle import select as S  # noqa: E402
from test_dropin_gpu import same_tables  # noqa: E402
from test_filter_counts_gpu import oracle_counts  # noqa: E402
from test_topk_gpu import want_rows  # noqa: E402

POLICIES = ["default", "wsum21", "negw"]
I64 = np.iinfo(np.int64)


def _dev():
    import torch
    return torch.device("cuda", 0)


def _pods(w):
    import torch
    return torch.from_numpy(w.c.now).to(_dev()), torch.from_numpy(w.c.ds).to(_dev())


# ------------------------------------------------------------------ matrices and keys
@pytest.mark.parametrize("policy", POLICIES)
def test_matrices(policy):
    """eval(matrix=True): the full first-fail and int64 score matrices, the chosen node and its
    score; the same as int8 from eval(matrix=True, compact=True)."""
    w = edge_world("mat-" + policy)
    ff, sc, ch = w.oracle()
    eng = engine_for(w.spec, w.c)
    gff, gsc, gch, gcs = eng.eval(w.c.now, w.c.ds, matrix=True)
    assert np.array_equal(gff, ff), np.argwhere(gff != ff)[:5]
    assert np.array_equal(gsc, sc), np.argwhere(gsc != sc)[:5]
    assert np.array_equal(gch, ch) and np.array_equal(gcs, w.best()[1])
    cff, csc, cch, ccs = eng.eval(w.c.now, w.c.ds, matrix=True, compact=True)
    assert csc.dtype == np.int8
    assert np.array_equal(cff, ff) and np.array_equal(csc, sc.astype(np.int8)), np.argwhere(csc != sc)[:5]
    assert np.array_equal(cch, ch) and np.array_equal(ccs, w.best()[1])
    eng.close()


@pytest.mark.parametrize("keys_path", [0, 1])
@pytest.mark.parametrize("policy", POLICIES)
def test_keys(policy, keys_path):
    """Keys only, 600 nodes x 1,025 pods, through the step path with annotation hot values (0) and
    the per-pair kernel (1): eval, and eval_keys_async on device buffers.  NaN / 9.3e17 / 1.26 hot
    values expire inside the batch range, some beside a NaN or 1e17 usage."""
    import torch
    w = edge_world("keys-" + policy)
    ch, best = w.best()
    eng = engine_for(w.spec, w.c, opts={"keys_path": keys_path})
    _, _, gch, gcs = eng.eval(w.c.now, w.c.ds)
    assert np.array_equal(gch, ch), np.flatnonzero(gch != ch)[:5]
    assert np.array_equal(gcs, best), np.flatnonzero(gcs != best)[:5]
    d_now, d_ds = _pods(w)
    d_keys = torch.empty(len(w.c.now), dtype=torch.int64, device=_dev())
    eng.eval_keys_async(d_now, d_ds, d_keys)
    torch.cuda.synchronize()
    node, score = keys_node_score(d_keys.cpu().numpy())
    assert np.array_equal(node, ch) and np.array_equal(score, best)
    eng.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_strings_in(policy):
    """The annotations in Go's spellings (NaN, +Inf, 1e300, 0x1p-2, 1_0.5, stamps to the ns) parsed
    by crane_parse_annotations, uploaded and evaluated equal the oracle reading the same strings."""
    w = edge_world("mat-" + policy)
    annos = edge_annotations(w.c)
    assert any("NaN," in v or "+Inf," in v for a in annos for v in a.values())
    ff, sc, ch = O.eval_strings(w.spec, annos, w.c.now, w.c.ds)
    eng = engine_for(w.spec)
    val, ts, hv, hv_ts = cd.parse_nodes(eng.metric_names, annos, SH)
    eng.upload_nodes(val, ts, hv, hv_ts)
    gff, gsc, gch, _ = eng.eval(w.c.now, w.c.ds, matrix=True)
    assert np.array_equal(gff, ff) and np.array_equal(gsc, sc) and np.array_equal(gch, ch)
    assert np.array_equal(ff, w.oracle()[0]) and np.array_equal(sc, w.oracle()[1])
    eng.close()


# ------------------------------------------------------------------ the step path
def _step_engine(w, opts):
    eng = engine_for(w.spec, w.c, opts=opts)
    eng.upload_bindings(w.c.b_node, w.c.b_ts)
    return eng


def _check_keys(w, t, keys, what):
    node, score = keys_node_score(keys.cpu().numpy())
    ch, best = w.best(t)
    assert np.array_equal(node, ch), (what, t, np.flatnonzero(node != ch)[:5])
    assert np.array_equal(score, best), (what, t, np.flatnonzero(score != best)[:5])


@pytest.mark.parametrize("step_rows", [1, 0])
@pytest.mark.parametrize("k1_stream", [1, 0])
@pytest.mark.parametrize("policy", POLICIES)
def test_step_stream(policy, k1_stream, step_rows):
    """step_keys_async at four batch times (hot values from the binding log: a penalty on half of
    the edge nodes), streamed and fused node pass, K3s with and without K1's tile rows."""
    import torch
    w = edge_world("step-" + policy)
    eng = _step_engine(w, {"k1_stream": k1_stream, "step_rows": step_rows})
    st = torch.cuda.Stream(_dev())
    d_now, d_ds = _pods(w)
    torch.cuda.synchronize()
    for t in EDGE_TIMES:
        keys = torch.empty(len(w.c.now), dtype=torch.int64, device=_dev())
        eng.step_keys_async(t, t, d_now, d_ds, keys, st.cuda_stream)
        st.synchronize()
        _check_keys(w, t, keys, f"stream k1_stream {k1_stream} step_rows {step_rows}")
    eng.close()


@pytest.mark.parametrize("policy", POLICIES)
def test_step_queue(policy):
    """The same world on a dispatch queue with step_defer 2: six batches into two alternating key
    buffers, the last two batches' keys."""
    import torch
    w = edge_world("step-" + policy)
    eng = _step_engine(w, {"step_defer": 2})
    q = cd.Queue(0)
    d_now, d_ds = _pods(w)
    two = [torch.empty(len(w.c.now), dtype=torch.int64, device=_dev()) for _ in range(2)]
    times = [EDGE_TIMES[b % 4] for b in range(6)]
    torch.cuda.synchronize()
    for b, t in enumerate(times):
        eng.step_keys_queue(t, t, d_now, d_ds, two[b % 2], q)
    eng.step_flush()
    q.wait()
    for b in (4, 5):
        _check_keys(w, times[b], two[b % 2], f"queue batch {b}")
    eng.close()
    q.close()


# ------------------------------------------------------------------ top-k, diagnosis, selection
@pytest.mark.parametrize("policy", POLICIES)
def test_topk_and_filter_counts(policy):
    """257 x 65 with the pods' times on the edge nodes' expiries: the 3 and the 16 best feasible
    nodes per pod, and the nodes counted by first failing predicate."""
    w = edge_world("mat-" + policy)
    eng = engine_for(w.spec, w.c)
    for k in (3, 16):
        got, want = eng.topk(w.c.now, w.c.ds, k=k), want_rows(w.spec, w.c, w.c.now, w.c.ds, k)
        assert np.array_equal(got, want), (k, np.argwhere(got != want)[:5])
    want = oracle_counts(w.spec, w.c, w.c.now, w.c.ds)
    assert np.array_equal(eng.filter_counts(w.c.now, w.c.ds), want)
    assert (want[:, :-1].sum(axis=1) > 0).any() and (want[w.c.ds == 0, -1] > 0).any()
    eng.close()


@pytest.mark.parametrize("pct,weight", SELECT_CASES)
def test_select(pct, weight):
    """Framework-level selection over the edge world's oracle matrices: adaptive windows with other
    plugins' filters and scores, and every node scored; at the shipped profile's weight 3 and at 30,
    where the Dynamic score outweighs the other plugins' sum."""
    import torch
    w = edge_world("mat-default")
    N, P = w.c.n_nodes, len(w.c.now)
    ext_ok, ext_score = select_ext(N, pct)
    ff, sc, _ = w.oracle()
    want = S.framework_select(ff, sc, w.c.ds, ext_ok, ext_score, weight, pct, 11, 0)
    eng = engine_for(w.spec, w.c)
    d_now, d_ds = _pods(w)
    out = [torch.empty(P, dtype=torch.int64, device=_dev()) for _ in range(4)]
    nxt = eng.select(d_now, d_ds, out[0], out[1], torch.from_numpy(ext_ok.astype(np.uint8)).to(_dev()),
                     torch.from_numpy(ext_score.astype(np.int64)).to(_dev()), dyn_weight=weight, percentage=pct, start=11,
                     tie_seed=0, d_wstart=out[2], d_wlen=out[3])
    torch.cuda.synchronize()
    for name, g, x in zip(("chosen", "total", "wstart", "wlen"), out, want[:4]):
        assert np.array_equal(g.cpu().numpy(), x), (name, np.flatnonzero(g.cpu().numpy() != x)[:5])
    assert nxt == want[4]
    if pct == 0:
        assert (want[3] < N).any(), "adaptive windows"
    eng.close()


# ------------------------------------------------------------------ answer tables
def _lookup_all(tab, times):
    """first_fail [T][N], score [T][N] of node_steps tables at each time."""
    return [np.stack(x) for x in zip(*(cd.Engine.table_lookup(tab, int(t)) for t in times))]


def _breakpoint_times(tab, t0, t1):
    ns, bp = tab[0], tab[1]
    live = np.arange(bp.shape[1])[None, :] < ns[:, None]
    bps = np.unique(np.concatenate([bp[live], [t0]]))
    times = np.unique(np.concatenate([bps, bps - 1, bps + 1, [t0, t1 - 1]]))
    return times[(times >= t0) & (times < t1)].astype(np.int64)


@pytest.mark.parametrize("policy", POLICIES)
def test_node_steps(policy):
    """node_steps over the stepping world's range, looked up at every breakpoint and 1 ns either
    side for every node (int8 table scores)."""
    w = edge_world("keys-" + policy)
    eng = engine_for(w.spec, w.c)
    t0, t1 = int(w.c.now.min()) - 7 * 10**9, int(w.c.now.max()) + 7 * 10**9
    tab = eng.node_steps(t0, t1)
    times = _breakpoint_times(tab, t0, t1)
    stepping = [n for n, lab in enumerate(w.labels) if lab and (lab["u_exp"] or lab["h_exp"])]
    assert (tab[0][stepping] > 0).mean() > 0.5 and len(times) > 100
    ff, sc, _ = oracle_soa(w.spec, w.c, now=times, ds=np.zeros(len(times), np.uint8))
    gff, gsc = _lookup_all(tab, times)
    assert np.array_equal(gff, ff), np.argwhere(gff != ff)[:5]
    assert np.array_equal(gsc, sc), np.argwhere(gsc != sc)[:5]
    eng.close()


# ------------------------------------------------------------------ scatter update
@pytest.mark.parametrize("fused", [0, 1])
def test_scatter_update(fused):
    """An engine uploaded with the plain synth cluster and moved to the edge cluster by
    update_nodes on the changed nodes (fused: update_node_steps) holds the records a full upload
    builds: keys, top-k rows and node_steps over the whole int64 range equal a fresh engine's and
    the oracle; the rows update_node_steps returns equal node_steps_subset's."""
    w = edge_world("keys-default")
    c = w.c
    plain = synth.make_cluster(w.spec, c.n_nodes, len(c.now), seed=c.seed, ds_frac=0.1)
    same = lambda a, b: (a == b) | ((a != a) & (b != b))  # noqa: E731
    changed = ~(same(plain.val, c.val).all(0) & (plain.ts == c.ts).all(0) & same(plain.hv, c.hv) & (plain.hv_ts == c.hv_ts))
    idx = np.flatnonzero(changed).astype(np.int64)
    assert set(idx) == set(np.flatnonzero(w.edge)) and 150 < len(idx) < 600
    eng = engine_for(w.spec, plain)
    fresh = engine_for(w.spec, c)
    val, ts, _ = c.rows(eng.metric_names)
    lo, hi = int(I64.min), int(I64.max)
    if fused:
        rows = eng.update_node_steps(idx, val[:, idx], ts[:, idx], c.hv[idx], c.hv_ts[idx], lo, hi)
        assert same_tables(rows, eng.node_steps_subset(lo, hi, idx))
        assert same_tables(rows, fresh.node_steps_subset(lo, hi, idx))
    else:
        eng.update_nodes(idx, val[:, idx], ts[:, idx], c.hv[idx], c.hv_ts[idx])
    ch, best = w.best()
    _, _, gch, gcs = eng.eval(c.now, c.ds)
    assert np.array_equal(gch, ch) and np.array_equal(gcs, best)
    sub = slice(0, len(c.now), 16)
    assert np.array_equal(eng.topk(c.now[sub], c.ds[sub], k=16), want_rows(w.spec, c, c.now[sub], c.ds[sub], 16))
    tab = eng.node_steps(lo, hi)
    assert same_tables(tab, fresh.node_steps(lo, hi))
    times = np.concatenate([c.now[:: 64], [lo, hi - 1, 0]]).astype(np.int64)
    ff, sc, _ = oracle_soa(w.spec, c, now=times, ds=np.zeros(len(times), np.uint8))
    gff, gsc = _lookup_all(tab, times)
    assert np.array_equal(gff, ff) and np.array_equal(gsc, sc)
    eng.close()
    fresh.close()


# ------------------------------------------------------------------ greedy
MERGE_STAGES = ("m2_bsum", "m3_scan", "m4_place", "m5z_direct", "m5a_compact", "m5b_thresholds", "m5c_takers", "m5d_assign")


def _greedy(eng, c, profile=True):
    eng.upload_bindings(c.b_node, c.b_ts)
    eng.set_profiling(profile)
    ch = eng.greedy(400, GREEDY_NOW, c.ds[:400])
    names = [n for n, _ in eng.stage_times()] if profile else []
    eng.set_profiling(False)
    return ch, names


@pytest.mark.parametrize("form", [0, 1])
def test_greedy_nan_falls_back_and_flag_resets(form):
    """(i) NaN usages on every seventh node: a base of int(NaN) rises to 100 with the node's first
    counted binding, so M1 raises its flag and greedy_form 0 runs the sequential kernel — seen in
    the kernel stages: greedy_run ran, no merge stream or assign stage did.  (ii) The same engine,
    re-uploaded without the NaN cells, takes the merge form again: the flag is per call."""
    spec, c, _ = greedy_world("nan")
    eng = engine_for(spec, c, opts={"greedy_form": form})
    ch, names = _greedy(eng, c)
    assert np.array_equal(ch, greedy_oracle(spec, c)), np.flatnonzero(ch != greedy_oracle(spec, c))[:5]
    assert "greedy_run" in names and not set(names) & set(MERGE_STAGES), names
    if form == 0:
        assert "m1_hist" in names, names
    spec, c, _ = greedy_world("plain")
    val, ts, _ = c.rows(eng.metric_names)
    eng.upload_nodes(val, ts, c.hv, c.hv_ts)
    ch, names = _greedy(eng, c)
    assert np.array_equal(ch, greedy_oracle(spec, c))
    if form == 0:
        assert "greedy_run" not in names and {"m1_hist", "m2_bsum", "m4_place"} <= set(names), names
    else:
        assert "greedy_run" in names and "m1_hist" not in names, names
    eng.close()


@pytest.mark.parametrize("form", [0, 1])
@pytest.mark.parametrize("case", ["overflow", "1e17", "negw"])
def test_greedy_huge_bases(case, form):
    """(iii) 1e300 / +Inf: the base is INT64_MIN through overflow, flagged like NaN.  (iv) 1e17:
    about -1e18, not flagged, and the merge's base - 10 v must not wrap.  (v) 1e17 on a negative
    weight: about +1e18, clamped to 100 down the whole staircase."""
    spec, c, _ = greedy_world(case)
    eng = engine_for(spec, c, opts={"greedy_form": form})
    ch, names = _greedy(eng, c)
    want = greedy_oracle(spec, c)
    assert np.array_equal(ch, want), np.flatnonzero(ch != want)[:5]
    if form == 0 and case == "overflow":
        assert "greedy_run" in names and not set(names) & set(MERGE_STAGES), names
    elif form == 0:
        assert "greedy_run" not in names and {"m1_hist", "m2_bsum", "m4_place"} <= set(names), names
    eng.close()
