"""The identity behind the filter diagnosis (csrc/diagnose.hip), in numpy, where no GPU is present.

Predicate k fails iff now < e_pred[k]; with the prefix maxima m_k = max_{j<=k} e_pred[j] a node's
first failing predicate at `now` is k iff m_{k-1} <= now < m_k.  So per pod only the ranks
C_k(now) = #{nodes : m_k <= now} are needed: the count of k is C_{k-1} - C_k (C_{-1} = N), the
feasible count C_{last}.  counts_by_rank below is the kernel's algorithm — sort the pod times, add 1
at lower_bound(times, m_k) per node and predicate, prefix-sum, write each pod through its original
position — and must equal the histogram of the first-fail matrix: the golden cluster's
(expect_filter, produced by the reference's Filter) and a brute-force one on edge cases.
Reference: pkg/plugins/dynamic/plugins.go:39-69, stats.go:42-48,94-112,140-150."""
import numpy as np

from conftest import policy_from_json
from oracle import oracle as O

I64_MIN = -(2**63)
EXTRA_NS = 5 * 60 * 10**9  # stats.go:26


def device_predicates(spec):
    """(policy index, metric, limit, active duration) of the predicates the Filter does not skip
    (plugins.go:56-61: no or zero active duration)."""
    period = {}
    for name, p in spec["syncPolicy"]:
        period.setdefault(name, p)
    out = []
    for j, (name, limit) in enumerate(spec["predicate"]):
        p = period.get(name, 0)
        if p != 0 and p + EXTRA_NS != 0:
            out.append((j, name, limit, p + EXTRA_NS))
    return out


def counts_by_rank(e_pred, pred_orig, n_pred, now, ds):
    """e_pred [npd][N] int64, pred_orig [npd] policy indices -> int32 [P][n_pred + 1]."""
    npd, N = e_pred.shape
    P = len(now)
    out = np.zeros((P, n_pred + 1), np.int64)
    order = np.argsort(now, kind="stable")
    times = now[order]
    prev = np.full(P, N, np.int64)
    m = np.full(N, I64_MIN, np.int64)
    for k in range(npd):
        m = np.maximum(m, e_pred[k])
        pos = np.searchsorted(times, m, side="left")  # the first sorted pod with now >= m_k (P: none)
        diff = np.bincount(pos, minlength=P + 1)[:P]
        c = np.cumsum(diff)                            # C_k per sorted position
        out[order, pred_orig[k]] = prev - c
        prev = c
    out[order, n_pred] = prev
    bypass = np.asarray(ds, bool)
    out[bypass] = 0
    out[bypass, n_pred] = N
    return out.astype(np.int32)


def histogram(ff, n_pred):
    ff = np.asarray(ff)
    return np.stack([(ff == j).sum(axis=1) for j in range(n_pred)] + [(ff < 0).sum(axis=1)], axis=1).astype(np.int32)


def test_rank_identity_on_the_golden_cluster(cluster_small):
    g = cluster_small
    spec = policy_from_json(g["policy"])
    tz = 8 * 3600
    dev = device_predicates(spec)
    N = len(g["nodes"])
    e_pred = np.full((len(dev), N), I64_MIN, np.int64)
    for k, (_, name, limit, dur) in enumerate(dev):
        for n, ann in enumerate(g["nodes"]):
            if name not in ann:
                continue
            ok, v, ts = O.parse_annotation(ann[name], tz)
            if ok and not v < 0 and limit != 0 and v > limit:  # isOverLoad, stats.go:94-112
                e_pred[k, n] = ts + dur
    now = np.array([p["now_ns"] for p in g["pods"]], np.int64)
    ds = np.array([p["daemonset"] for p in g["pods"]], np.uint8)
    n_pred = len(spec["predicate"])
    want = histogram(g["expect_filter"], n_pred)
    assert want[:, :n_pred].any(), "the golden cluster rejects some node"
    got = counts_by_rank(e_pred, [j for j, *_ in dev], n_pred, now, ds)
    assert np.array_equal(got, want)
    # the order of the pods does not matter
    perm = np.random.default_rng(1).permutation(len(now))
    assert np.array_equal(counts_by_rank(e_pred, [j for j, *_ in dev], n_pred, now[perm], ds[perm]), want[perm])


def test_rank_identity_against_brute_force():
    """Random expiries with ties, never-failing predicates (INT64_MIN), the extremes of int64,
    duplicate pod times on and beside expiries, skipped policy columns, DaemonSet pods."""
    rng = np.random.default_rng(2)
    npd, N, n_pred = 5, 300, 8
    pred_orig = [0, 2, 3, 6, 7]
    e = rng.integers(0, 40, (npd, N)).astype(np.int64) * 10
    e[rng.random((npd, N)) < 0.5] = I64_MIN
    e[0, :3] = 2**63 - 1
    e[2, 3:6] = I64_MIN + 1
    now = np.concatenate([rng.integers(-5, 405, 200), [I64_MIN, I64_MIN + 1, 2**63 - 1, 2**63 - 2, 100, 100, 99, 101]])
    now = now.astype(np.int64)
    ds = (rng.random(len(now)) < 0.1).astype(np.uint8)
    fails = now[:, None, None] < e[None, :, :]                     # [P][npd][N]
    first = np.where(fails.any(axis=1), fails.argmax(axis=1), -1)  # device index or -1
    ff = np.where(first >= 0, np.array(pred_orig)[np.maximum(first, 0)], -1)
    ff[ds == 1] = -1
    got = counts_by_rank(e, pred_orig, n_pred, now, ds)
    assert np.array_equal(got, histogram(ff, n_pred))
    assert (got.sum(axis=1) == N).all()
    assert (got[:, [1, 4, 5]] == 0).all()
