"""The per-pair kernels' lane cache (csrc/pair_eval.hpp) at the sizes where it decides something:
k3m_matrix (matrix.hip), k_sel_pairs (select.hip) and k_topk (topk.hip) evaluate a node at the
minimum time of a 64-pod sub-chunk, keep the result with the interval between the node's expiries on
which it holds, and reuse it, step it once or re-evaluate it per pod in the sub-chunks that follow.
A workgroup of the first two takes P * N / 4096 / 64 pods, so below about 17 M pairs it sees one
sub-chunk and the cache never decides anything; the 4- and 8-nodes-per-lane instances of k3m_matrix
with matrix outputs need 67 M and 134 M pairs in one launch.
Reference: pkg/plugins/dynamic/plugins.go:39-98 (Filter, DaemonSet bypass :41-43, Score)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
from helpers import engine_for, oracle_soa  # noqa: E402
import test_topk_gpu  # noqa: E402


def backwards_blocks(n_pods, seed):
    """A pod order: permuted inside every block of 64, and in every other block of 128 the two
    64-blocks swapped, so that the second sub-chunk of such a workgroup chunk is the earlier one."""
    rng = np.random.default_rng(seed)
    order = np.arange(n_pods)
    for b in range(0, n_pods, 64):
        order[b:b + 64] = rng.permutation(order[b:b + 64])
    for b in range(0, n_pods - 127, 256):
        order[b:b + 128] = np.concatenate([order[b + 64:b + 128], order[b:b + 64]])
    return order


def block_changes(ff, sc, now, ds):
    """[blocks of 64 pods][N]: how often a node's (first_fail, score) changes over the block's
    non-DaemonSet pods in time order."""
    out = []
    for b in range(0, len(now), 64):
        rows = b + np.nonzero(ds[b:b + 64] == 0)[0]
        rows = rows[np.argsort(now[rows], kind="stable")]
        v = ff[rows].astype(np.int32) * 256 + sc[rows].astype(np.int32)
        out.append((v[1:] != v[:-1]).sum(axis=0))
    return np.stack(out)


def test_subchunk_cache_three_consumers(monkeypatch):
    """17,500 nodes x 1,024 pods = 17.92 M pairs: 17.92 M / 4096 waves / 64 lanes = 68 pods per
    workgroup, rounded to 128 = two sub-chunks for k3m_matrix and k_sel_pairs (the smallest shape
    that gives them two); k_topk at k = 4 takes 8192 / (4 * 4) = 512 pods per workgroup = eight
    sub-chunks.  With the pods a second apart, shuffled inside the 64-blocks and every other pair
    of blocks swapped, a lane's cached answer is reused, stepped once, re-evaluated per pod and
    run backwards in time; the preconditions say how often, from the oracle's matrices alone."""
    import torch
    spec = cd.default_policy_spec()
    N, P = 17_500, 1_024
    c = synth.make_cluster(spec, N, P, seed=41, pod_step_ns=10**9, ds_frac=0.1)
    order = backwards_blocks(P, 41)
    now, ds = np.ascontiguousarray(c.now[order]), np.ascontiguousarray(c.ds[order])
    off, osc, och = oracle_soa(spec, c, now, ds)

    ch = block_changes(off, osc, now, ds)
    one, more = int((ch == 1).sum()), int((ch >= 2).sum())
    flat = int(((ch[0::2] == 0) & (ch[1::2] == 0)).sum())
    print("one step", one, "several", more, "flat in both blocks", flat)  # (the oracle: 41833 3992 98045)
    assert one >= 10_000 and more >= 1_000 and flat >= 10_000

    dev = torch.device("cuda", 0)
    eng = engine_for(spec, c)
    d_now, d_flags = torch.from_numpy(now).to(dev), torch.from_numpy(ds).to(dev)
    d_ff = torch.empty((P, N), dtype=torch.int8, device=dev)
    d_sc = torch.empty((P, N), dtype=torch.int8, device=dev)
    d_keys = torch.empty(P, dtype=torch.int64, device=dev)
    eng.eval_matrix_async(d_now, d_flags, d_ff, d_sc, d_keys)
    torch.cuda.synchronize()
    assert np.array_equal(d_ff.cpu().numpy(), off)
    assert np.array_equal(d_sc.cpu().numpy(), osc)
    del d_ff, d_sc
    monkeypatch.setattr(test_topk_gpu, "oracle_soa", lambda *a, **kw: (off, osc, och))  # (the one oracle call)
    want = test_topk_gpu.want_rows(spec, c, now, ds, 4)
    assert np.array_equal(d_keys.cpu().numpy(), want[:, 0])  # a pod's key: its best candidate
    assert np.array_equal(eng.topk(now, ds, k=4), want)

    d_ch = torch.empty(P, dtype=torch.int64, device=dev)
    eng.select(d_now, d_flags, d_ch, dyn_weight=1, percentage=100, start=0, tie_seed=0)
    torch.cuda.synchronize()
    assert np.array_equal(d_ch.cpu().numpy(), och)
    eng.close()


def test_matrix_wide_lanes_equal_narrow():
    """131,072 nodes x 1,024 pods = 134,217,728 pairs, the smallest shape at which k3m_matrix takes
    8 nodes per lane (64 lanes x 8 nodes x 64 pods = the 32,768 pairs a wave gets of 4096 waves).
    The row stride picks the instance: ld = N 8 per lane (dwordx2 stores, 256-pod workgroups),
    ld = N + 4 4 per lane (dword stores, 128 pods), ld = N + 1 one (byte stores, 512 pods).  All
    three write the same matrices and keys, leave the padding alone, and 64 sampled pod rows are
    the oracle's."""
    import torch
    spec = cd.default_policy_spec()
    N, P = 131_072, 1_024
    c = synth.make_cluster(spec, N, P, seed=43, pod_step_ns=10**9, ds_frac=0.1)
    order = backwards_blocks(P, 43)
    now, ds = np.ascontiguousarray(c.now[order]), np.ascontiguousarray(c.ds[order])
    rows = np.sort(np.random.default_rng(43).choice(P, 64, replace=False))
    off, osc, _ = oracle_soa(spec, c, now[rows], ds[rows])
    dev = torch.device("cuda", 0)
    eng = engine_for(spec, c)
    d_now, d_flags = torch.from_numpy(now).to(dev), torch.from_numpy(ds).to(dev)
    d_rows = torch.from_numpy(rows).to(dev)
    out = []
    for pad in (0, 4, 1):
        d_ff = torch.full((P, N + pad), 77, dtype=torch.int8, device=dev)
        d_sc = torch.full((P, N + pad), 77, dtype=torch.int8, device=dev)
        d_keys = torch.empty(P, dtype=torch.int64, device=dev)
        eng.eval_matrix_async(d_now, d_flags, d_ff, d_sc, d_keys, ld=N + pad)
        torch.cuda.synchronize()
        assert bool((d_ff[:, N:] == 77).all()) and bool((d_sc[:, N:] == 77).all()), pad  # padding untouched
        out.append((d_ff, d_sc, d_keys))
    eng.close()
    wide = out[0]
    for pad, (d_ff, d_sc, d_keys) in zip((4, 1), out[1:]):
        assert torch.equal(d_ff[:, :N], wide[0]), pad
        assert torch.equal(d_sc[:, :N], wide[1]), pad
        assert torch.equal(d_keys, wide[2]), pad
    assert np.array_equal(wide[0][d_rows].cpu().numpy(), off)
    assert np.array_equal(wide[1][d_rows].cpu().numpy(), osc)
    del out, wide, d_ff, d_sc, d_keys
    torch.cuda.empty_cache()
