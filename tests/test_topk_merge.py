"""crane_topk_merge (csrc/topk_merge.cpp, cd.topk_merge): the host combine of node shards' top-k
rows.  Every input is [P, k], rows descending with -1 pads last; the output is the k largest keys
per pod of the inputs' rows, in the same format.  Expected: the keys of all lists side by side,
sorted descending, cut to k.  No device is involved."""
import numpy as np
import pytest

cd = pytest.importorskip("crane_dyn")

CRANE_E_INVALID = -1


def rows(rng, n_pods, k, n_lists, shapes):
    """n_lists arrays [n_pods, k] of distinct keys packed like the engine's, (score << 32) |
    (0xFFFFFFFF - node) with every list drawing from its own node range (a shard).  Row p has
    shapes[p % len(shapes)] entries per list: an int (that many in every list, capped at k), or a
    tuple with one count per list."""
    out = [np.full((n_pods, k), -1, np.int64) for _ in range(n_lists)]
    for p in range(n_pods):
        want = shapes[p % len(shapes)]
        for l in range(n_lists):
            n = min(k, want if isinstance(want, int) else want[l % len(want)])
            node = 1000 * l + rng.choice(1000, n, replace=False)
            key = (rng.integers(0, 4, n).astype(np.int64) << 32) | (0xFFFFFFFF - node)  # heavy score ties
            out[l][p, :n] = -np.sort(-key)
    return out


def expected(lists, k):
    return -np.sort(-np.concatenate(lists, axis=1), axis=1)[:, :k]


@pytest.mark.parametrize("n_lists", [1, 2, 5])
@pytest.mark.parametrize("k", [1, 16])
def test_merge_equals_sorted_union(n_lists, k):
    rng = np.random.default_rng(100 * n_lists + k)
    # all -1; full rows; only the first list has entries; fewer than k entries in total; a mix
    shapes = [0, k, (k, 0, 0, 0, 0), (min(k, 2), 0, 1, 0, 0), (3, 16, 0, 1, 7)]
    lists = rows(rng, 23, k, n_lists, shapes)
    got = cd.topk_merge(lists)
    want = expected(lists, k)
    assert got.dtype == np.int64 and got.shape == (23, k)
    assert np.array_equal(got, want)
    assert (got[0] == -1).all()                          # a row of pads only
    assert np.array_equal(got[2], lists[0][2])           # a row that one list fills alone
    if k == 16:
        assert ((got[3] >= 0).sum() < k) and (got[3, 0] >= 0)  # fewer than k entries in total
        nz = got >= 0
        assert (nz[:, :-1] >= nz[:, 1:]).all()           # pads last
        assert ((got[:, :-1] > got[:, 1:]) | ~nz[:, 1:]).all()  # strictly descending before them


def test_inputs_unchanged_and_not_aliased():
    rng = np.random.default_rng(7)
    lists = rows(rng, 9, 4, 3, [4, 1, (0, 4, 2)])
    before = [a.copy() for a in lists]
    got = cd.topk_merge(lists)
    assert all(np.array_equal(a, b) for a, b in zip(lists, before))
    assert np.array_equal(got, expected(lists, 4))


def test_no_pods():
    got = cd.topk_merge([np.empty((0, 16), np.int64), np.empty((0, 16), np.int64)])
    assert got.shape == (0, 16) and got.dtype == np.int64


@pytest.mark.parametrize("k", [0, 17])
def test_k_out_of_range(k):
    with pytest.raises(cd.CraneError) as ei:
        cd.topk_merge([np.full((3, k), -1, np.int64)] * 2)
    assert ei.value.code == CRANE_E_INVALID


def test_shape_mismatch():
    with pytest.raises(ValueError):
        cd.topk_merge([np.full((3, 4), -1, np.int64), np.full((3, 5), -1, np.int64)])
    with pytest.raises(ValueError):
        cd.topk_merge([])
