"""CPU: the restatement of the quantile definition (tests/quantiles_ref.py; DESIGN.md section 4, "Quantiles") against itself and against
the outside truth, and the three entry points' first check through the C ABI.

  * the sort-and-cumulate statement and the digit-by-digit one return the same bits;
  * with equal weights Q(k / n) for a dyadic k / n is the k-th smallest value, and Q(0.1) at n = 1000 is the 101st (the double 0.1
    exceeds 1 / 10);
  * the returned value v has F(v) >= q - eps and F(v^-) <= q + eps against the real-valued CDF (long-double exponentials, math.fsum),
    eps = 2 n / S + 2^-50;
  * mp_pf_quantiles, mp_pf_path_quantiles and mp_mh_site_quantiles answer a null handle with MP_ERR_INVALID_ARG (no GPU needed;
    without the feature the symbols are missing)."""
import ctypes as C

import numpy as np
import pytest

from tests import quantiles_ref as Q

QS = [0.0, 0.1, 0.25, 0.5, 1.0]


def cloud(n, seed):
    """values with ties, both zeros and a few huge / tiny magnitudes; log-weights with -inf among them (never all)"""
    rng = np.random.default_rng(seed)
    v = rng.normal(0.0, 2.0, size=n)
    tie = rng.random(n) < 0.3
    v[tie] = np.round(v[tie])                                                                    # ties
    pick = rng.random(n)
    v[pick < 0.05] = 0.0
    v[(pick >= 0.05) & (pick < 0.10)] = -0.0
    v[(pick >= 0.10) & (pick < 0.12)] = 1e300
    v[(pick >= 0.12) & (pick < 0.14)] = -4e-310                                                  # a subnormal
    lw = rng.normal(-3.0, 2.5, size=n)
    lw[rng.random(n) < 0.2] = -np.inf
    if not np.isfinite(lw).any():
        lw[0] = -1.25
    return v, lw


@pytest.mark.parametrize("n", [1, 2, 7, 300, 1025])
@pytest.mark.parametrize("seed", [0, 1])
def test_the_two_statements_agree_bit_for_bit(n, seed):
    v, lw = cloud(n, 10 * n + seed)
    W = Q.pf_int_weights(lw)
    assert W is not None and W.max() == int(Q.scale(n))          # the heaviest particle weighs exactly S
    assert (W[lw == -np.inf] == 0).all()
    a = Q.select_sorted(v, W, QS)
    b = Q.select_digits(v, W, QS)
    assert Q.same_bits(a, b), (a, b)
    for bits in (4, 16):                                         # the result does not depend on the digit width
        assert Q.same_bits(a, Q.select_digits(v, W, QS, bits=bits))
    live = W > 0
    assert set(a.view(np.uint64).tolist()) <= set(v[live].view(np.uint64).tolist())      # a stored value of positive weight, its own bits
    k = Q.keys(v[live])
    assert Q.keys(a[:1])[0] == k.min() and Q.keys(a[-1:])[0] == k.max()                   # q = 0 the smallest, q = 1 the largest


def test_zeros_order_and_dead_slots():
    v = np.array([0.0, -0.0, -0.0, 0.0, 5.0, -7.0])
    lw = np.array([0.0, 0.0, 0.0, 0.0, -np.inf, -np.inf])
    W = Q.pf_int_weights(lw)
    got = Q.select_sorted(v, W, [0.0, 0.5, 0.51, 1.0])
    assert Q.same_bits(got, Q.select_digits(v, W, [0.0, 0.5, 0.51, 1.0]))
    assert np.signbit(got).tolist() == [True, True, False, False] and not got.any()       # -0.0 sorts just below +0.0; 5 and -7 are dead
    assert Q.pf_int_weights(np.full(4, -np.inf)) is None
    nan_w = Q.pf_int_weights(np.array([0.0, np.nan]))
    assert not nan_w.any() and np.isnan(Q.select_sorted(v[:2], nan_w, [0.5])).all()
    assert np.isnan(Q.select_digits(v[:2], nan_w, [0.5])).all()


def test_equal_weights_give_order_statistics():
    rng = np.random.default_rng(5)
    n = 64
    v = rng.normal(size=n)
    s = np.sort(v)
    W = Q.pf_int_weights(np.full(n, -2.5))
    assert (W == int(Q.scale(n))).all()
    ks = list(range(1, n + 1))
    got = Q.select_sorted(v, W, [k / n for k in ks])             # k / 64 is exact
    assert Q.same_bits(got, s[[k - 1 for k in ks]])
    assert Q.same_bits(Q.select_digits(v, W, [0.25, 0.5]), s[[15, 31]])
    n = 1000
    v = rng.normal(size=n)
    s = np.sort(v)
    W = Q.pf_int_weights(np.zeros(n))
    for sel in (Q.select_sorted, Q.select_digits):
        got = sel(v, W, [0.1, 0.5, 0.0, 1.0])
        assert Q.same_bits(got, s[[100, 499, 0, 999]]), got       # the 101st: the double 0.1 exceeds 1 / 10; 0.5 is exact: the 500th


@pytest.mark.parametrize("n", [1, 7, 300, 5000])
def test_mass_bound_against_the_real_valued_cdf(n):
    v, lw = cloud(n, 77 + n)
    W = Q.pf_int_weights(lw)
    got = Q.select_sorted(v, W, QS)
    worst = Q.check_mass(v, lw, QS, got)
    print(f"n = {n}: eps = {Q.mass_epsilon(n):.3e}, worst slack / eps = {worst:.3f}")


def test_site_statement_counts_and_absent_sites():
    vals = np.array([[1.0, 9.0, 3.0], [2.0, 9.0, 1.0], [3.0, 9.0, 2.0], [4.0, 9.0, 0.0]])
    present = np.array([0b101, 0b001, 0b101, 0b001], dtype=np.uint64)
    count, out = Q.site_quantiles(vals, present, [0.0, 0.5, 1.0])
    assert count.tolist() == [4, 0, 2]
    assert out[:, 0].tolist() == [1.0, 2.0, 4.0] and np.isnan(out[:, 1]).all() and out[:, 2].tolist() == [2.0, 2.0, 3.0]


def test_entry_points_reject_a_null_handle():
    import __graft_entry__ as g

    g.build()
    from modppl_amd import capi

    L = capi.load()
    qs, out, t, cnt = (C.c_double * 1)(0.5), (C.c_double * 64)(), C.c_int32(-1), (C.c_uint64 * 64)()
    assert L.mp_pf_quantiles(None, qs, 1, out) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(None, qs, 1, out, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(None, qs, 1, cnt, out) == capi.MP_ERR_INVALID_ARG
    assert t.value == -1
