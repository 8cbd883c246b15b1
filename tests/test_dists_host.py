"""The count and positive-real distributions of modppl_amd/csrc/mp_dists.h (poisson, gamma, beta, geometric, uniform_discrete) and
the special functions under them (mp_math.h mp_lgamma, mp_log1p), on the host through tests/host/dists_shim.cpp: the reference's
known answers (modppl/tests/dists.rs:186-211), accuracy against mpmath, each sampler's law on 10^6 draws per parameter point
(chi-square for the counts, Kolmogorov-Smirnov for the reals; fixed seeds), and the support rules."""
import math

import mpmath
import numpy as np
import pytest
from scipy import stats

from tests import dists_shim as S

LOGPDF_EPSILON = 1.19e-7   # modppl/tests/dists.rs
mf = mpmath.mpf


@pytest.fixture(scope="module", autouse=True)
def _mp_precision():
    old = mpmath.mp.prec
    mpmath.mp.prec = 160
    yield
    mpmath.mp.prec = old


def rel_err(y, ref):
    return np.abs(y - ref) / np.maximum(1., np.abs(ref))


def test_shim_compiles_warning_clean_with_the_checker_flags():
    _, diag = S.build()
    assert "warning" not in diag, diag[-3000:]


def test_reference_known_answers():
    """dists.rs:186-211"""
    cases = [
        (S.GEOMETRIC, 1, 0.5, None, -1.3862943611198906), (S.GEOMETRIC, 5, 0.98, None, -19.580317734458244),
        (S.GEOMETRIC, 101, 0.01, None, -5.6202541071917365),
        (S.POISSON, 3, 4.0, None, -1.6328763858683835), (S.POISSON, 5, 1.5, None, -4.2601662022412240),
        (S.POISSON, 52, 36.11, None, -5.969204868031767),
        (S.BETA, 0.3, 0.5, 0.5, -0.364406011717066), (S.BETA, 0.7, 1.5, 2.0, -0.06055443631298263),
        (S.BETA, 0.3, 0.5, 0.5, -0.36440601171706609),
        (S.GAMMA, 1.7, 1.23, 1.46, -1.414334369005868), (S.GAMMA, 8.4, 4.5, 1.0, -3.4049256003700052),
        (S.GAMMA, 0.03, 50.0, 70.0, -528.8122715889206),
    ]
    for dist, x, a, b, want in cases:
        got = S.logpdf(dist, [x], a, b)[0]
        assert abs(got - want) <= LOGPDF_EPSILON, (dist, x, a, b, got, want)


def test_lgamma_against_mpmath():
    xs = np.logspace(-12, 12, 100_000)
    y = S.lgamma(xs)
    ref = np.array([float(mpmath.loggamma(mf(float(v)))) for v in xs])
    assert rel_err(y, ref).max() <= 1e-15
    ints = np.arange(1, 10_001, dtype=np.float64)
    y = S.lgamma(ints)
    ref = np.array([float(mpmath.loggamma(int(v))) for v in ints])
    assert rel_err(y, ref).max() <= 1e-15


def test_lgamma_is_zero_at_one_and_two():
    y = S.lgamma([1.0, 2.0])
    assert y[0] == 0.0 and y[1] == 0.0
    assert np.isnan(S.lgamma([0.0, -1.0, np.nan])).all()
    assert S.lgamma([np.inf])[0] == np.inf


def test_log1p_against_mpmath():
    xs = np.concatenate([-np.logspace(-300, -1e-9, 20_000), np.logspace(-300, 300, 20_000), np.linspace(-0.999, 3., 20_000)])
    y = S.log1p(xs)
    ref = np.array([float(mpmath.log1p(mf(float(v)))) for v in xs])
    assert (np.abs(y - ref) / np.abs(ref)).max() <= 4.5e-16   # < 2 ulp
    assert S.log1p([-1.0])[0] == -np.inf and np.isnan(S.log1p([-1.5])[0]) and S.log1p([0.0])[0] == 0.0


def test_poisson_logpdf_against_mpmath():
    ks = np.array([0, 1, 2, 3, 5, 10, 30, 100, 300, 1e3, 1e4, 1e5, 1e6])
    for r in [1e-3, 0.1, 3., 9.99, 10., 40., 250., 1e4, 1e6]:
        y = S.logpdf(S.POISSON, ks, r)
        ref = [float(k * mpmath.log(mf(r)) - mf(r) - mpmath.loggamma(k + 1)) for k in ks]
        e = rel_err(y, np.array(ref))
        if r == 1e6:
            # k ln r - r - ln k! at k = r = 10^6: terms of 1.4e7 cancel to -7.8; the error is that of the terms (< 1e-15 of them)
            big = ks == 1e6
            assert e[~big].max() <= 1e-13
            assert abs(y[big][0] - ref[-1]) <= 1e-15 * (1e6 * math.log(1e6))
        else:
            assert e.max() <= 1e-13, (r, e.max())


def test_gamma_logpdf_against_mpmath():
    xs = np.logspace(-6, 3, 200)
    for a in [0.05, 0.5, 1., 4.5, 20., 200.]:
        for b in [0.1, 1., 7.]:
            y = S.logpdf(S.GAMMA, xs, a, b)
            ref = [float((mf(a) - 1) * mpmath.log(mf(x)) - mf(x) / mf(b) - mpmath.loggamma(mf(a)) - mf(a) * mpmath.log(mf(b))) for x in xs]
            assert rel_err(y, np.array(ref)).max() <= 1e-13, (a, b)


def test_beta_logpdf_against_mpmath():
    xs = np.concatenate([np.logspace(-8, -1e-9, 100), 1. - np.logspace(-8, -0.5, 100)])
    for a in [0.1, 0.5, 2., 5., 20.]:
        for b in [0.1, 0.5, 2., 5., 20.]:
            y = S.logpdf(S.BETA, xs, a, b)
            ref = [float(mpmath.loggamma(mf(a) + mf(b)) - mpmath.loggamma(mf(a)) - mpmath.loggamma(mf(b)) + (mf(a) - 1) * mpmath.log(mf(x))
                         + (mf(b) - 1) * mpmath.log1p(-mf(x))) for x in xs]
            assert rel_err(y, np.array(ref)).max() <= 1e-13, (a, b)


def test_geometric_logpdf_against_mpmath():
    ps = np.concatenate([np.logspace(-8, -0.31, 60), 1. - np.logspace(-8, -0.31, 60)])
    for k in [0, 1, 5, 100, 1e4, 1e6]:
        y = S.logpdf(S.GEOMETRIC, np.full(ps.size, float(k)), ps)
        ref = [float(k * mpmath.log1p(-mf(p)) + mpmath.log(mf(p))) for p in ps]
        assert rel_err(y, np.array(ref)).max() <= 1e-13, k


def test_uniform_discrete_logpdf():
    for a, b in [(-5., 7.), (0., 0.), (-1000., -3.), (3., 1e6)]:
        xs = np.array([a, b, math.floor((a + b) / 2)])
        y = S.logpdf(S.UNIFORM_DISCRETE, xs, a, b)
        assert (y == -math.log(b - a + 1)).all() or np.abs(y + math.log(b - a + 1)).max() <= 1e-15 * math.log(b - a + 1)


def test_support_rules():
    ninf = -np.inf
    # poisson: negative and non-integer counts; k = 0 at rate 0 (no 0 * ln 0 term)
    assert list(S.logpdf(S.POISSON, [-1., 2.5, np.inf, np.nan], 3.)) == [ninf] * 4
    assert S.logpdf(S.POISSON, [0.], 0.)[0] == 0. and S.logpdf(S.POISSON, [3.], 0.)[0] == ninf
    assert S.logpdf(S.POISSON, [0.], 2.5)[0] == -2.5
    assert (S.sample(S.POISSON, 1000, 0.) == 0.).all()
    assert np.isnan(S.logpdf(S.POISSON, [1.], -1.)[0])
    # gamma: x > 0
    assert list(S.logpdf(S.GAMMA, [0., -1., np.inf], 2., 3.)) == [ninf] * 3
    # beta: 0 < x < 1
    assert list(S.logpdf(S.BETA, [0., 1., -0.5, 1.5], 2., 3.)) == [ninf] * 4
    # geometric: counts
    assert list(S.logpdf(S.GEOMETRIC, [-1., 0.5, np.inf], 0.3)) == [ninf] * 3
    assert S.logpdf(S.GEOMETRIC, [0.], 0.3)[0] == math.log(0.3) or abs(S.logpdf(S.GEOMETRIC, [0.], 0.3)[0] - math.log(0.3)) < 1e-16
    # uniform_discrete: integers in [a, b]
    assert list(S.logpdf(S.UNIFORM_DISCRETE, [-6., 8., 0.5], -5., 7.)) == [ninf] * 3
    # samples strictly inside the support
    g = S.sample(S.GAMMA, 1_000_000, 0.05, 1., seed=5)
    assert (g > 0.).all() and np.isfinite(g).all()
    bt = S.sample(S.BETA, 1_000_000, 0.1, 0.1, seed=6)
    assert (bt > 0.).all() and (bt < 1.).all()
    assert (np.isfinite(S.logpdf(S.BETA, bt, 0.1, 0.1))).all()
    for dist, a, b in [(S.POISSON, 3.7, None), (S.POISSON, 250., None), (S.GEOMETRIC, 0.3, None), (S.UNIFORM_DISCRETE, -4., 9.)]:
        v = S.sample(dist, 100_000, a, b, seed=7)
        assert (v == np.floor(v)).all() and np.isfinite(S.logpdf(dist, v, a, b)).all()


N = 1_000_000


def _chi2(samples, pmf, lo, hi, min_expected=20.):
    """chi-square of integer samples against pmf over [lo, hi], adjacent values merged until each cell expects >= min_expected"""
    ks = np.arange(lo, hi + 1)
    p = pmf(ks)
    obs = np.bincount((np.clip(samples, lo, hi) - lo).astype(np.int64), minlength=ks.size).astype(np.float64)
    p = p.copy()
    p[0] += 1. - p.sum()   # (the tails beyond [lo, hi], in the clipped end cells)
    cells_o, cells_e, acc_o, acc_e = [], [], 0., 0.
    for o, e in zip(obs, p * samples.size):
        acc_o += o
        acc_e += e
        if acc_e >= min_expected:
            cells_o.append(acc_o); cells_e.append(acc_e); acc_o = acc_e = 0.
    cells_o[-1] += acc_o
    cells_e[-1] += acc_e
    return stats.chisquare(cells_o, cells_e).pvalue


@pytest.mark.parametrize("r", [0.1, 3., 9.99, 10., 250., 1e6])
def test_poisson_sampler_law(r):
    x = S.sample(S.POISSON, N, r, seed=101)
    lo, hi = int(max(0, math.floor(r - 8 * math.sqrt(r) - 2))), int(math.ceil(r + 8 * math.sqrt(r) + 12))
    pv = _chi2(x, lambda k: stats.poisson.pmf(k, r), lo, hi)
    assert pv > 1e-4, (r, pv, x.mean(), x.var())
    assert abs(x.mean() - r) <= 5 * math.sqrt(r / N)


@pytest.mark.parametrize("a", [0.05, 0.5, 1., 4.5, 200.])
def test_gamma_sampler_law(a):
    b = 1.7
    x = S.sample(S.GAMMA, N, a, b, seed=202)
    pv = stats.kstest(x, stats.gamma(a, scale=b).cdf).pvalue
    assert pv > 1e-4, (a, pv)


@pytest.mark.parametrize("ab", [(0.1, 0.1), (0.5, 0.5), (2., 5.)])
def test_beta_sampler_law(ab):
    a, b = ab
    x = S.sample(S.BETA, N, a, b, seed=303)
    # Below t = 1 - 2^-40 the law is Kolmogorov-Smirnov's against the conditional cdf; above it the doubles are too coarse to resolve
    # the density (at (0.1, 0.1) 1.3 % of the mass rounds or clamps to 1 - 2^-53, the largest double below 1): there only the mass counts
    t = 1. - 2. ** -40
    d = stats.beta(a, b)
    below = x[x < t]
    pv = stats.kstest(below, lambda v: d.cdf(v) / d.cdf(t)).pvalue
    assert pv > 1e-4, (ab, pv)
    m = (x >= t).mean()
    assert abs(m - d.sf(t)) <= 5 * math.sqrt(d.sf(t) / N) + 1e-12, (ab, m, d.sf(t))


@pytest.mark.parametrize("p", [1e-4, 0.3, 0.98])
def test_geometric_sampler_law(p):
    x = S.sample(S.GEOMETRIC, N, p, seed=404)
    hi = int(math.ceil(math.log(1e-7) / math.log1p(-p)))
    pv = _chi2(x, lambda k: stats.geom.pmf(k + 1, p), 0, hi)   # scipy's geom counts trials: k failures = k + 1 trials
    assert pv > 1e-4, (p, pv)


@pytest.mark.parametrize("ab", [(-7., 5.), (-1000., -990.), (-3., 40.)])
def test_uniform_discrete_sampler_law(ab):
    a, b = ab
    x = S.sample(S.UNIFORM_DISCRETE, N, a, b, seed=505)
    assert x.min() >= a and x.max() <= b
    n = int(b - a + 1)
    pv = _chi2(x - a, lambda k: np.full(k.size, 1. / n), 0, n - 1)
    assert pv > 1e-4, (ab, pv)


def test_draws_are_a_function_of_the_site_stream():
    """the same Philox coordinates give the same variates; another site, step or slot gives others"""
    a = S.sample(S.GAMMA, 1000, 0.7, 2., seed=9, step=3, site=4)
    assert np.array_equal(a, S.sample(S.GAMMA, 1000, 0.7, 2., seed=9, step=3, site=4))
    assert not np.array_equal(a, S.sample(S.GAMMA, 1000, 0.7, 2., seed=9, step=3, site=5))
    assert np.array_equal(a[10:], S.sample(S.GAMMA, 990, 0.7, 2., seed=9, step=3, site=4, slot0=10))


# ---- small shapes: both gammas of a beta can underflow to 0 (Gamma(a) for a < 1 is Gamma(a + 1) U^(1/a)); the beta is then formed
# from their logarithms instead of as 0 / 0 ----

@pytest.mark.parametrize("a", [1e-3, 2e-3, 5e-3, 0.02])
def test_beta_small_symmetric_shapes_are_symmetric(a):
    """Beta(a, a) puts mass 1/2 on each side of 1/2; 10^6 draws, 5 sigma"""
    x = S.sample(S.BETA, N, a, a, seed=606)
    assert np.isfinite(x).all() and x.min() >= 2. ** -1022 and x.max() <= 1. - 2. ** -53
    p = (x > 0.5).mean()
    assert abs(p - 0.5) <= 5 * math.sqrt(0.25 / N), (a, p)


@pytest.mark.parametrize("ab,points", [((1e-3, 5.), [1e-300, 1e-200, 1e-100, 1e-30, 1e-10, 1e-3, 0.1, 0.5]),
                                       ((5., 1e-3), [0.3, 0.6, 0.9, 0.99, 1. - 1e-6, 1. - 1e-12, 1. - 2. ** -50])])
def test_beta_small_shape_cdf(ab, points):
    """the empirical cdf at a handful of points against the regularised incomplete beta (mpmath.betainc)"""
    a, b = ab
    x = S.sample(S.BETA, N, a, b, seed=707)
    for t in points:
        F = float(mpmath.betainc(a, b, 0, t, regularized=True))
        e = (x <= t).mean()
        assert abs(e - F) <= 5 * math.sqrt(F * (1. - F) / N) + 1e-12, (ab, t, e, F)


def test_gamma_tiny_shape_clamped_share():
    """Gamma(10^-3, 1): the variates that underflow are clamped to 2^-1022; their share is P(X <= 2^-1022), the regularised lower
    incomplete gamma there"""
    a = 1e-3
    x = S.sample(S.GAMMA, N, a, 1., seed=808)
    t = 2. ** -1022
    assert x.min() >= t
    F = float(mpmath.gammainc(a, 0, mpmath.mpf(t), regularized=True))
    share = (x == t).mean()
    assert abs(share - F) <= 5 * math.sqrt(F * (1. - F) / N), (share, F)
