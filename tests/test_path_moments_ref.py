"""The restatement of the path moments (tests/path_moments_ref.py) on its own, before any device is involved: synthetic per-step
states and random parent arrays, the walk of the event log against a particle-by-particle walk, the restated mean / variance per time
step within the bounds the GPU tests hold the device to (tests/test_gpu_path_moments.py uses the same `check_bounds`), and the
distinct-ancestor count against np.unique."""
import numpy as np
import pytest

from tests import moments_ref as R
from tests import path_moments_ref as P

SIZES = [1, 2, 255, 2049, (1 << 16) + 63]
STEPS = [1, 7]


@pytest.fixture(scope="module")
def oracle():
    from tests import oracle_lib as O

    O.build()
    return O.load()


def _weights(kind, n, rng):
    if kind == "flat":
        return np.zeros(n)
    if kind == "peaked":
        lw = rng.normal(0, 1, size=n) - 60.0
        lw[n // 2] = 5.0
        return lw
    if kind == "survivor":
        lw = np.full(n, -np.inf)
        lw[n // 3] = -3.25
        return lw
    lw = rng.normal(0, 2, size=n)          # "dead": a third of the cloud has weight zero
    lw[rng.random(n) < 1 / 3] = -np.inf
    lw[0] = 0.5
    return lw


def _history(n, T, rng, last_is_resample):
    """an event log as the filter records it: a step, then per further step none, one or two resamples and a step"""
    events = [None]
    for t in range(1, T):
        for _ in range((t + 1) % 3):
            events.append(rng.integers(0, n, size=n).astype(np.uint32))
        events.append(None)
    if last_is_resample:
        events.append(rng.integers(0, n, size=n).astype(np.uint32))
    return events


def _walk_one(i, events):
    """slot i's ancestors, one particle at a time (k_trajectories' loop)"""
    a, out = i, []
    for e in reversed(events):
        if e is None:
            out.append(a)
        else:
            a = int(e[a])
    return out[::-1]


@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
def test_ancestors_and_distinct(n, T):
    rng = np.random.default_rng(7 * n + T)
    for last in (False, True):
        events = _history(n, T, rng, last)
        anc = P.ancestors(n, events)
        assert anc.shape == (n, T)
        for i in {0, n // 2, n - 1}:
            assert anc[i].tolist() == _walk_one(i, events)
        k = P.distinct(anc)
        assert k.dtype == np.uint64 and k.tolist() == [len(np.unique(anc[:, t])) for t in range(T)]
        assert np.all(np.diff(k.astype(np.int64)) >= 0)      # lineages only coalesce going back
        assert k[-1] == (len(np.unique(events[-1])) if last else n)


@pytest.mark.parametrize("T", STEPS)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["flat", "peaked", "survivor", "dead"])
def test_restated_path_moments_within_the_bounds(oracle, n, T, kind):
    rng = np.random.default_rng(1000 + n + T)
    for dim in (1, 3):
        xs = [rng.normal(2.0, 1.5, size=(n, dim)) * np.array([1.0, 30.0, 1e-3][:dim]) + t for t in range(T)]
        events = _history(n, T, rng, kind == "flat")
        anc = P.ancestors(n, events)
        paths = P.gather(xs, anc)
        assert paths.shape == (n, T, dim)
        lw = _weights(kind, n, rng)
        mean, var = P.path_moments(paths, lw)
        P.check_bounds(paths, lw, mean, var)
        assert R.same_numbers(P.path_moments(paths, lw, var=False)[0], mean)
        # every time step is the cloud moments of that step's gathered states: the last row is what pf_moments gives
        for t in range(T):
            m, c = R.pf_moments(paths[:, t], lw)
            assert R.same_numbers(mean[t], m) and R.same_numbers(var[t], np.diag(c))
        if kind == "flat":
            assert R.same_numbers(mean[0], [R.tree_sum(paths[:, 0, j]) / n for j in range(dim)])
        if kind == "survivor":
            assert np.array_equal(mean, paths[n // 3]) and not var.any()


def test_all_minus_inf_is_degenerate(oracle):
    assert R.pf_weights(np.full(5, -np.inf)) is None
