"""The restatement of the canonical moments (tests/moments_ref.py) on its own, before any device is involved: the tree sum against
math.fsum within the textbook pairwise bound, and the restated mean / covariance within the error bounds the GPU tests hold the device to
(tests/test_gpu_moments.py uses the same `check_bounds`), on synthetic clouds with flat, peaked and one-survivor weights and -inf entries."""
import math

import numpy as np
import pytest

from tests import moments_ref as R

SIZES = [1, 2, 3, 2047, 2048, 2049, (1 << 16) + 63]


@pytest.mark.parametrize("n", SIZES)
def test_tree_sum_within_the_pairwise_bound(n):
    """|TREE(v) - sum v| <= ceil(log2 n) u sum |v|  (Higham, Accuracy and Stability, section 4.2, to first order; n = 1 is exact)"""
    rng = np.random.default_rng(n)
    cases = [rng.normal(size=n), rng.normal(size=n) * np.exp(rng.normal(0, 8, size=n))]
    c = rng.normal(size=n) * 1e8
    c[1::2] = -c[: n // 2] * (1 + 1e-9 * rng.normal(size=n // 2))   # cancelling pairs
    cases.append(c)
    for v in cases:
        exact = math.fsum(v.tolist())
        bound = R.ceil_log2(n) * R.U * math.fsum(np.abs(v).tolist())
        assert abs(R.tree_sum(v) - exact) <= bound, (n, R.tree_sum(v), exact, bound)


def test_tree_sum_is_the_definition():
    assert R.tree_sum([1.0]) == 1.0
    assert R.tree_sum([1.0, 2.0, 4.0]) == (1.0 + 2.0) + (4.0 + 0.0)
    v = np.array([1e16, 1.0, -1e16, 1.0, 3.0])
    assert R.tree_sum(v) == (((1e16 + 1.0) + (-1e16 + 1.0)) + ((3.0 + 0.0) + (0.0 + 0.0)))


def _weights(kind, n, rng):
    if kind == "flat":
        return np.zeros(n)
    if kind == "spread":
        return rng.normal(0, 3, size=n) - 700.0
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


@pytest.fixture(scope="module")
def oracle():
    from tests import oracle_lib as O

    O.build()
    return O.load()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("kind", ["flat", "spread", "peaked", "survivor", "dead"])
def test_restated_moments_within_the_bounds(oracle, n, kind):
    rng = np.random.default_rng(1000 + n)
    for dim in (1, 3):
        x = rng.normal(2.0, 1.5, size=(n, dim)) * np.array([1.0, 30.0, 1e-3][:dim])
        lw = _weights(kind, n, rng)
        mean, cov = R.pf_moments(x, lw)
        R.check_bounds(x, lw, mean, cov)
        assert R.same_numbers(R.pf_moments(x, lw, cov=False)[0], mean)
        if kind == "flat":
            assert R.same_numbers(mean, [R.tree_sum(x[:, j]) / n for j in range(dim)])
        if kind == "survivor":
            assert np.array_equal(mean, x[n // 3]) and not cov.any()


def test_all_minus_inf_is_degenerate(oracle):
    assert R.pf_weights(np.full(5, -np.inf)) is None


def test_site_moments_select_instead_of_multiplying():
    vals = np.array([[1.0, np.nan, 7.0], [3.0, np.inf, 7.0], [6.0, 2.0, 7.0]])
    present = np.array([0b001, 0b001, 0b011])
    count, mean, var = R.site_moments(vals, present)
    assert count.tolist() == [3, 1, 0]
    assert mean[0] == ((1.0 + 3.0) + (6.0 + 0.0)) / 3.0 and mean[1] == 2.0 and var[1] == 0.0
    assert np.isnan(mean[2]) and np.isnan(var[2])
