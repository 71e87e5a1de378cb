"""The reference pinned on usages and hot values outside what the controller writes, and the
liveness of the worlds tests/test_value_edges_gpu.py runs the engine on — all on the CPU.

synth.make_cluster generates usages in about [-1.2, 1.2] with five decimals and whole hot values
0..12; helpers.edge_cluster overwrites a seeded share of cells with NaN, +-Inf, huge, denormal,
signed-zero and boundary values (helpers.USAGE_CLASSES / HOT_CLASSES).  What the reference does
with them (stats.go:51-76, 114-138, plugins.go:73-98) is pinned three ways here: the C oracle from
parsed columns, the C oracle from annotation strings in Go's spellings, and the pure-Python
restatement tests/golden/pyref.py; the hand-derived rows are the VE-* entries of
tests/golden/kats.json (make_golden.py carries each derivation).

Liveness, from the oracle alone, of every world of helpers.EDGE_WORLDS:
 (a) at least a third of the pods' chosen nodes are edge nodes (per batch time in a step world);
 (b) every class of the generator's tables sits on a node where it decides something: at some pod
     time the node's score or first failing predicate differs from the same node with that one
     value replaced by 0.5 (a usage) or 0 (a hot value) — for the hot-value classes that score as
     0 themselves (-0.0, 0.05: int(h * 10) = 0; -1.0, -Inf: rejected) no result can differ from
     0's, so they are replaced by 1 instead (helpers.HOT_CLASSES holds the replacement);
 (c) in the worlds whose keys step (keys-*, step-*), at least 8 edge nodes per pod kind have an
     edge cell's expiry inside that kind's batch range (tmin, tmax];
 (d) in the same worlds, whose consumers output only the winner per pod, at least 16 pods are won
     by a node whose base is INT64_MIN (NaN, +Inf, 1e300 usage) and, with annotation hot values,
     16 by a node whose penalty is (NaN, +Inf, 1e300, 9.3e17), among at least 5 distinct winners.
For the greedy worlds: the oracle's greedy loop equals its per-call answers replayed pod by pod,
and with NaN / overflowing bases a pod lands on an edge node after that node's score rose."""
import numpy as np
import pytest

cd = pytest.importorskip("crane_dyn")
import pyref  # noqa: E402
from helpers import (EDGE_COMBOS, EDGE_WORLDS, GREEDY_CASES, HOT_CLASSES, USAGE_CLASSES, edge_annotations,  # noqa: E402
                     edge_cluster, edge_policy, edge_world, go_float, greedy_oracle, greedy_replay, greedy_world,
                     oracle_soa, select_ext, SELECT_CASES)
from oracle import oracle as O  # noqa: E402
from oracle import select as S  # noqa: E402


def test_go_float_spellings_parse_back_exactly():
    """Every class value, as the formatter spells it, is read back bit for bit by both parsers."""
    spec = edge_policy("negw")
    vals = [v(spec, "cpu_usage_avg_5m") if callable(v) else v for _, v, _ in USAGE_CLASSES] + [v for _, v, _ in HOT_CLASSES]
    assert {go_float(v) for v in vals} >= {"NaN", "+Inf", "-Inf", "1e300", "0x1p-2", "1_0.5", "-0.0", "5e-324"}
    for v in vals:
        s = go_float(v)
        for got, err in (O.go_parse_float(s), pyref.go_parse_float(s)):
            assert err is None, s
            assert np.float64(got).tobytes() == np.float64(v).tobytes(), (s, got, v)


@pytest.mark.parametrize("kind", ["default", "wsum21", "negw"])
def test_three_references_agree(kind):
    """600 nodes x 8 pods: the oracle from columns, the oracle from strings and pyref, every pair."""
    spec = edge_policy(kind)
    c, labels = edge_cluster(spec, 600, 8, seed=8001)
    c.ds[:] = [0, 0, 1, 0, 0, 1, 0, 0]
    present_u = {lab["u"] for lab in labels if lab and lab["u"]}
    present_h = {lab["h"] for lab in labels if lab and lab["h"]}
    assert present_u == {k for k, _, _ in USAGE_CLASSES} and present_h == {k for k, _, _ in HOT_CLASSES}
    assert {(lab["u"], lab["h"]) for lab in labels if lab} >= set(EDGE_COMBOS)
    ff, sc, ch = oracle_soa(spec, c)
    annos = edge_annotations(c)
    ff2, sc2, ch2 = O.eval_strings(spec, annos, c.now, c.ds)
    assert np.array_equal(ff, ff2) and np.array_equal(sc, sc2) and np.array_equal(ch, ch2)
    for p in range(8):
        f3 = [pyref.filter_node(spec, a, int(c.now[p]), bool(c.ds[p])) for a in annos]
        s3 = [pyref.score_node(spec, a, int(c.now[p])) for a in annos]
        assert np.array_equal(ff[p], f3), p
        assert np.array_equal(sc[p], s3), p
    edge = np.array([lab is not None for lab in labels])
    assert set(np.unique(sc[:, edge])) >= {0, 100}


def test_issue_table_through_the_soa_oracle():
    """The rows of the VE-* KATs that a one-node cluster of parsed columns can state: the same
    answers from columns as make_golden.py derives from strings."""
    spec = cd.default_policy_spec()
    names = [n for n, _ in spec["syncPolicy"]]
    t = int(pyref.go_parse_time(pyref.format_local(1792065600)))
    rows = [(float("nan"), 1.0, -1, 100), (float("nan"), 0.0, -1, 0), (1e300, 0.7, 0, 100), (1e17, float("nan"), 0, 100),
            (0.1, float("nan"), -1, 0), (0.1, 1.26, -1, 78), (0.1, 9.3e17, -1, 0), (1e17, 9.2e17, 0, 100),
            (0.1, -0.0, -1, 90), (0.1, float("-inf"), -1, 90), (float("-inf"), 0.0, -1, 81), (5e-324, 0.0, -1, 91)]
    for u, h, want_ff, want_sc in rows:
        val = np.full((6, 1), 0.1)
        val[0, 0] = u
        ff, sc, _ = O.eval_soa(spec, names, np.ones((6, 1), np.uint8), val, np.full((6, 1), t, np.int64),
                               np.ones(1, np.uint8), np.array([h]), np.array([t], np.int64), np.array([t], np.int64))
        assert (ff[0, 0], sc[0, 0]) == (want_ff, want_sc), (u, h)


@pytest.mark.parametrize("name", sorted(EDGE_WORLDS))
def test_world_is_live(name):
    w = edge_world(name)
    c = w.c
    # (a)
    for t in w.times:
        ch, _ = w.best(t)
        on_edge = np.where(ch >= 0, w.edge[np.maximum(ch, 0)], False)
        assert on_edge.mean() >= 1 / 3, (t, on_edge.mean())
    # (b)
    t = w.times[0]
    ff, sc, _ = w.oracle(t)
    for what, table in (("u", USAGE_CLASSES), ("h", HOT_CLASSES if w.hot else [])):
        if not table:
            assert all(lab is None or lab[what] is None for lab in w.labels)
            continue
        ff2, sc2, _ = w.eval(w.replaced(what), t)
        differs = ((ff != ff2) | (sc != sc2)).any(axis=0)
        live = {lab[what] for n, lab in enumerate(w.labels) if lab and lab[what] and differs[n]}
        assert live == {k for k, *_ in table}, (what, sorted({k for k, *_ in table} - live))
    # (c)
    if name.startswith(("keys-", "step-")):
        for kind in (0, 1):
            now = c.now[c.ds == kind]
            lo, hi = int(now.min()), int(now.max())
            exp = [[e for e in (lab["u_exp"], lab["h_exp"]) if e is not None and lo < e <= hi] for lab in w.labels if lab]
            assert sum(1 for e in exp if e) >= 8, (kind, sum(1 for e in exp if e))
    # (d) keys show the winners only: nodes whose base is INT64_MIN (and, with annotation hot values,
    # nodes whose penalty is) win pods, so a wrong conversion there changes keys
    if name.startswith(("keys-", "step-")):
        won = np.concatenate([w.best(t)[0] for t in w.times])
        labs = [w.labels[n] for n in won if n >= 0 and w.labels[n]]
        assert sum(lab["u"] in ("NaN", "+Inf", "1e300") for lab in labs) >= 16
        assert not w.hot or sum(lab["h"] in ("NaN", "+Inf", "1e300", "9.3e17") for lab in labs) >= 16
        assert len(np.unique(won)) >= 5
    assert -(-c.n_nodes // 256) == {257: 2, 600: 3}[c.n_nodes] and -(-len(c.now) // 1024) == {65: 1, 1025: 2}[len(c.now)]


@pytest.mark.parametrize("pct,weight", SELECT_CASES)
def test_selection_depends_on_the_edge_values(pct, weight):
    """The selection test's world: with the edge usages at 0.5 the framework picks another node or
    total for at least 5 of the 65 pods, and at weight 30 the edge hot values decide picks too."""
    w = edge_world("mat-default")
    ext_ok, ext_score = select_ext(w.c.n_nodes, pct)
    ff, sc, _ = w.oracle()
    want = S.framework_select(ff, sc, w.c.ds, ext_ok, ext_score, weight, pct, 11, 0)
    for what in ("u", "h"):
        ff2, sc2, _ = w.eval(w.replaced(what))
        other = S.framework_select(ff2, sc2, w.c.ds, ext_ok, ext_score, weight, pct, 11, 0)
        moved = ((want[0] != other[0]) | (want[1] != other[1])).sum()
        assert moved >= (5 if what == "u" or weight == 30 else 0), (what, moved)
    assert len(np.unique(want[0])) >= 2


def test_step_worlds_bind_half_of_the_edge_nodes():
    """The penalty is positive on some edge nodes and 0 on others at every batch time."""
    for name in sorted(EDGE_WORLDS):
        w = edge_world(name)
        if w.step:
            for t in w.times:
                hv = w.hv_at(t)[0][w.edge]
                assert (hv > 0).sum() >= len(hv) // 4 and (hv == 0).sum() >= len(hv) // 4, (name, t)


def test_hot_annotation_expiries_beside_wrapped_bases():
    """keys-*: NaN / 9.3e17 / 1.26 hot values expire inside the batch range, and nodes that carry a
    NaN or 1e17 usage as well are among those with such hot values."""
    for name in ("keys-default", "keys-wsum21", "keys-negw"):
        w = edge_world(name)
        for h in ("NaN", "9.3e17", "1.26"):
            assert any(lab and lab["h"] == h and lab["h_exp"] for lab in w.labels), (name, h)
            assert any(lab and lab["h"] == h and lab["u"] in ("NaN", "1e17") for lab in w.labels), (name, h)
        both = [lab for lab in w.labels if lab and lab["u"] in ("NaN", "1e17") and lab["h"] in ("NaN", "9.3e17", "1.26")]
        assert any(lab["h_exp"] for lab in both) and any(lab["u_exp"] for lab in both), name


@pytest.mark.parametrize("case", GREEDY_CASES)
def test_greedy_world(case):
    """The oracle's greedy loop is its per-call Filter / Score / first maximum replayed with the
    placements as bindings.  nan, overflow: some pod lands on an edge node after that node's score
    rose (what the merge form's premise — staircases only fall — excludes).  1e17, negw: edge nodes
    take pods, and none of their scores ever rises."""
    spec, c, edge = greedy_world(case)
    chosen = greedy_oracle(spec, c)
    replay, seen = greedy_replay(spec, c)
    assert np.array_equal(chosen, replay)
    rose = [p for p in range(len(chosen)) if chosen[p] in edge and p and seen[:p, chosen[p]].min() < seen[p, chosen[p]]]
    any_rise = (np.diff(seen, axis=0) > 0).any()
    if case in ("nan", "overflow"):
        assert rose, "no pod landed on an edge node whose score had risen"
        assert any(chosen[p] in edge and seen[p, chosen[p]] == 0 for p in range(len(chosen))), "the first binding at score 0"
    else:
        assert not any_rise
    if case != "plain":
        assert np.isin(chosen, edge).sum() >= 40
    if case == "negw":
        assert (seen[:, edge] == 100).all()
    assert 0 < c.ds[:400].sum() < 400
