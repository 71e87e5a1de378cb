"""CPU checks of the sequential greedy at per-pod times (crane_dyn_greedy_times).

1. The reference composes from the committed oracle: with all times equal, one-pod greedy calls
   over the growing log reproduce the oracle's own greedy loop.
2. A numpy model of the kernels' event scheme (csrc/greedy_times.hip: the events as a CSR by the
   first pod that sees them, per-window heads over chosen[], recompute of touched nodes only)
   equals the reference at every targeted shape of test_greedy_times_gpu.py.  It checks the
   algorithm, not the kernels, as test_merge_model.py does for the merge form.
"""
import numpy as np
import pytest

cd = pytest.importorskip("crane_dyn")
from crane_dyn import synth  # noqa: E402
import greedy_times_ref as R  # noqa: E402


def test_reference_composition_equals_oracle_greedy():
    spec = cd.default_policy_spec()
    N, P = 300, 256
    c = synth.make_cluster(spec, N, P, n_bindings=3000, seed=5, ds_frac=0.1)
    now = np.full(P, R.T0, np.int64)
    want = R.frozen(spec, c, now, c.ds)
    assert np.array_equal(R.ref(spec, c, now, c.ds), want)
    assert len(np.unique(want)) > 20  # the placements feed back: not one node for all


@pytest.mark.parametrize("name", list(R.CASES))
def test_event_model_equals_reference(name):
    spec, c, now, ds, want, frozen = R.case(name)
    got, recomputed, n_events = R.model(spec, c, now, ds)
    diff = np.flatnonzero(got != want)
    assert diff.size == 0, (diff[:5], got[diff[:5]], want[diff[:5]])
    # the case isolates its event class only if time matters in it
    assert (want != frozen).any()
    # the model recomputes touched nodes only: at most one per event and per placement that
    # leaves a window
    assert recomputed <= n_events + len(spec["hotValue"]) * len(now)


@pytest.mark.parametrize("seed", range(6))
def test_event_model_equal_times_is_frozen_greedy(seed):
    spec = cd.default_policy_spec()
    c = synth.make_cluster(spec, 50, 120, n_bindings=400, seed=seed, ds_frac=0.2)
    now = np.full(120, R.T0, np.int64)
    got, recomputed, n_events = R.model(spec, c, now, c.ds)
    assert np.array_equal(got, R.frozen(spec, c, now, c.ds))
    assert recomputed == 0 and n_events == 0
