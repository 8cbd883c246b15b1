"""The restatement of the forecast moments (tests/forecast_ref.py) on its own, before any device is involved: hand-made arrays with n
not a power of two, a -inf weight, and H = 1 against pf_moments' mean and diag(cov) of states[:, 0]."""
import numpy as np
import pytest

from tests import forecast_ref as F
from tests import moments_ref as R


@pytest.fixture(scope="module")
def oracle():
    from tests import oracle_lib as O

    O.build()
    return O.load()


def test_equal_weights_by_hand(oracle):
    """n = 3 (padded to 4 by the tree), equal weights: sums small enough to do by hand, exact in fp64"""
    states = np.array([[[1.0, 10.0], [2.0, 20.0]], [[2.0, 10.0], [4.0, 20.0]], [[3.0, 40.0], [6.0, 80.0]]])   # [3, 2, 2]
    obs = states[:, :, :1] * 0.5
    sm, sv, om, ov = F.forecast_moments(states, obs, np.zeros(3))
    assert np.array_equal(sm, [[2.0, 20.0], [4.0, 40.0]])
    assert np.array_equal(sv, [[2.0 / 3.0, 200.0], [8.0 / 3.0, 800.0]])
    assert np.array_equal(om, [[1.0], [2.0]])
    assert np.array_equal(ov, [[(0.25 + 0.25) / 3.0], [2.0 / 3.0]])
    sm1, sv1, om1, ov1 = F.forecast_moments(states, obs, np.zeros(3), var=False)
    assert sv1 is None and ov1 is None and np.array_equal(sm1, sm) and np.array_equal(om1, om)


def test_a_minus_inf_weight_contributes_nothing(oracle):
    """the dead slot holds NaN-free garbage of another scale: selected to weight 0, it must not show; the live two have weights 1 and
    exp(-ln 2) up to mp_exp's rounding, so the truth is checked through the weights the restatement itself uses"""
    states = np.array([[[1.0]], [[1e100]], [[4.0]], [[-2.0]], [[7.0]]])
    obs = -states
    lw = np.array([0.0, -np.inf, 0.0, 0.0, 0.0])
    sm, sv, om, ov = F.forecast_moments(states, obs, lw)
    assert np.array_equal(sm, [[2.5]]) and np.array_equal(om, [[-2.5]])
    want_var = ((1.5 ** 2 + 1.5 ** 2) + (4.5 ** 2 + 4.5 ** 2)) / 4.0
    assert np.array_equal(sv, [[want_var]]) and np.array_equal(ov, [[want_var]])
    assert R.pf_weights(np.full(5, -np.inf)) is None      # the library's MP_ERR_DEGENERATE


@pytest.mark.parametrize("n", [1, 2, 255, 2049])
def test_one_step_is_the_cloud_moments_of_that_step(oracle, n):
    rng = np.random.default_rng(50 + n)
    states = rng.normal(1.0, 2.0, size=(n, 1, 3)) * np.array([1.0, 30.0, 1e-3])
    obs = rng.normal(size=(n, 1, 2))
    lw = rng.normal(0, 2, size=n)
    if n > 2:
        lw[n // 3] = -np.inf
    sm, sv, om, ov = F.forecast_moments(states, obs, lw)
    for got_m, got_v, cols in ((sm, sv, states[:, 0]), (om, ov, obs[:, 0])):
        m, c = R.pf_moments(cols, lw)
        assert R.same_numbers(got_m[0], m) and R.same_numbers(got_v[0], np.diag(c))


def test_every_horizon_is_reduced_on_its_own(oracle):
    rng = np.random.default_rng(9)
    n, H = 300, 4
    states, obs, lw = rng.normal(size=(n, H, 2)), rng.normal(size=(n, H, 1)), rng.normal(size=n)
    sm, sv, om, ov = F.forecast_moments(states, obs, lw)
    assert sm.shape == sv.shape == (H, 2) and om.shape == ov.shape == (H, 1)
    for k in range(H):
        a = F.forecast_moments(states[:, k:k + 1], obs[:, k:k + 1], lw)
        assert R.same_numbers(a[0][0], sm[k]) and R.same_numbers(a[1][0], sv[k]) and R.same_numbers(a[2][0], om[k]) and R.same_numbers(a[3][0], ov[k])
