"""GPU: the hierarchical fixed-point normalisation against exact arithmetic.  No checker is involved: every case
reads back the log-weights a real model produced on the device (`pf.log_weights`) and computes, from those values, what the
normalisation should return:

  L   = m + ln Z,        Z  = sum_i exp(lw_i - m),  m = max lw   (what `resample()` returns)
  ESS = Z^2 / Z2,        Z2 = sum_i exp(2 (lw_i - m))             (`effective_sample_size(fresh=True)`)
  log-ML = sum over the folds of (m_t + ln Z_t - ln N)            (`log_marginal_likelihood_estimate()`)
  p_i = exp(lw_i - m) / Z                                          (the law of the draws)

The exact side uses x87 long double: exp of lw - m (both doubles; the difference and expl are within 2^-63 relative, an error in
the exponent of |lw - m| 2^-64 becomes at most 2^-64 / e absolutely) and numpy's pairwise sum of positive terms (within
log2(N) 2^-64 relative): together at most 2^-58 relative, negligible against the bounds below.  For N <= 10^4 it is cross-checked
against mpmath at 128 bits.

The tolerances are the error bounds DESIGN.md §4 derives for the fixed-point scheme (u = 2^-53, n_t = ceil(N / 2048),
S = 62 - ceil(log2 N)); nothing is tuned by hand:

  |Q 2^-S - Z|   <= D_Q  = n_t 2^-(S+1) + N u (2 + 2/e) + 6 u Z
  |Q2 2^-S - Z2| <= D_Q2 = n_t 2^-(S+1) + N u (2 + 2/e) + 9 u Z2
  |L - (m + ln Z)| <= d/(1 - d) + 2u (|ln Z| + 2d) + u |L|,         d = D_Q / Z + u
  |ESS / (Z^2/Z2) - 1| <= (1 + d)^2 (1 + u)^2 / (1 - d2) - 1,       d2 = D_Q2 / Z2 + u
  log-ML: the sum of the L bounds, + 2u ln N per fold (mp_log(N)) + 2u (|log-ML| + |L| + ln N) per fold (two additions)
  systematic (stratified) offspring: |c_i - N p_i| <= 1 (2) + N (9u p_i Z + c0 + p_i D_Q) / (Z - D_Q) + 6 N 2^-52,
      c0 = 2^-52 + 2u/e + 2^-(S+1) + 2^(1-S) + 2^-42
"""
import math

import mpmath
import numpy as np
import pytest

from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
U = 2.0 ** -53
E = math.e
MULTI, SYS, STRAT = 0, 1, 2


def S_of(n):
    return 62 - (int(n) - 1).bit_length()


def nt_of(n):
    return (int(n) + 2047) // 2048


class Exact:
    """the exact normalisation of one log-weight vector (long double)"""

    def __init__(self, lw):
        lw = np.ascontiguousarray(lw, dtype=np.float64)
        self.n = lw.size
        self.m = float(lw.max())
        assert np.isfinite(self.m)
        e = np.exp(lw.astype(np.longdouble) - np.longdouble(self.m))
        self.Z = np.sum(e)            # pairwise
        self.Z2 = np.sum(e * e)
        self.lnZ = float(np.log(self.Z))
        self.L = np.longdouble(self.m) + np.log(self.Z)
        self.ess = float(self.Z * self.Z / self.Z2)
        self.p = (e / self.Z).astype(np.float64)
        self.dead = np.isneginf(lw)
        self.lw_min = float(lw[~self.dead].min())
        if self.n <= 10_000:
            with mpmath.workprec(128):
                Zm = mpmath.fsum(mpmath.exp(mpmath.mpf(float(v)) - self.m) for v in lw if v != -np.inf)
                assert abs(mpmath.mpf(float(self.Z)) - Zm) <= 2 ** -52 * Zm   # (the long double sum, seen through a double)
                assert abs(self.lnZ - float(mpmath.log(Zm))) <= 2 ** -52 * max(1.0, abs(self.lnZ))

    def DQ(self):
        n, S, nt = self.n, S_of(self.n), nt_of(self.n)
        return nt * 2.0 ** -(S + 1) + n * U * (2 + 2 / E) + 6 * U * float(self.Z)

    def DQ2(self):
        n, S, nt = self.n, S_of(self.n), nt_of(self.n)
        return nt * 2.0 ** -(S + 1) + n * U * (2 + 2 / E) + 9 * U * float(self.Z2)

    def L_bound(self, L):
        d = self.DQ() / float(self.Z) + U
        return d / (1 - d) + 2 * U * (abs(self.lnZ) + 2 * d) + U * abs(L)

    def ess_bound(self):
        d = self.DQ() / float(self.Z) + U
        d2 = self.DQ2() / float(self.Z2) + U
        return ((1 + d) ** 2 * (1 + U) ** 2 / (1 - d2) - 1) * self.ess

    def count_slack(self, lattice):
        n, S = self.n, S_of(self.n)
        Z, DQ = float(self.Z), self.DQ()
        c0 = 2.0 ** -52 + 2 * U / E + 2.0 ** -(S + 1) + 2.0 ** (1 - S) + 2.0 ** -42
        return lattice + n * (9 * U * self.p * Z + c0 + self.p * DQ) / (Z - DQ) + 6 * n * 2.0 ** -52


class Tracker:
    """runs a filter and holds every normalisation it performs to the exact values; records the largest errors seen"""

    def __init__(self, pf, n):
        self.pf, self.n, self.lnN = pf, n, math.log(n)
        self.lml_exact = 0.0      # (a Python float sum of long double terms: its own error is far below the bound's 2u terms)
        self.lml_bound = 0.0
        self.worst = {"L": 0.0, "ESS": 0.0, "logML": 0.0}

    def _fold_bound(self, ex, L):
        return ex.L_bound(L) + 2 * U * self.lnN + 2 * U * (abs(self.lml_exact) + abs(L) + self.lnN)

    def query(self):
        """fresh ESS and log-ML of the current weights, against the exact ones; -> Exact"""
        ex = Exact(self.pf.log_weights)
        ess = self.pf.effective_sample_size(fresh=True)
        assert abs(ess - ex.ess) <= ex.ess_bound(), (self.n, ess, ex.ess, ex.ess_bound())
        self.worst["ESS"] = max(self.worst["ESS"], abs(ess - ex.ess) / ex.ess_bound())
        lml = self.pf.log_marginal_likelihood_estimate()
        want = self.lml_exact + float(ex.L - np.longdouble(self.lnN))
        bound = self.lml_bound + self._fold_bound(ex, float(ex.L))
        assert abs(lml - want) <= bound, (self.n, lml, want, bound)
        self.worst["logML"] = max(self.worst["logML"], abs(lml - want) / bound)
        return ex

    def resample(self, scheme=MULTI):
        """L of `resample()` against the exact value; -> (Exact of the weights it normalised, parents)"""
        ex = self.query()
        L = self.pf.resample(scheme=scheme)
        err, b = abs(np.longdouble(L) - ex.L), ex.L_bound(L)
        assert err <= b, (self.n, L, float(ex.L), float(err), b)
        self.worst["L"] = max(self.worst["L"], float(err) / b)
        self.lml_bound += self._fold_bound(ex, L)
        self.lml_exact += float(ex.L - np.longdouble(self.lnN))
        return ex, self.pf.parents.astype(np.int64)


def _lgssm(params, n, seed):
    import modppl_amd

    return modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*params), n, seed)


DEFAULT = tuple(O.LGSSM_PARAMS)
# (lgssm parameters mu0, sig0, a, sig_x, sig_y; observations)
REGIMES = {
    "default": (DEFAULT, [0.4, -0.3, 0.9]),
    "flat": ((0.0, 1.0, 0.9, 0.5, 1e6), [0.3, -0.2, 0.1]),              # Z ~ N: Q reaches 2^62 at N = 2^k
    "peaked": ((0.0, 1.0, 0.9, 0.5, 1e-3), [0.5, 0.45, 0.4]),          # most q are 0, log-weights down to about -10^6
    "survivor": ((0.0, 1.0, 0.9, 0.5, 1e-8), [3.3, 3.2, 3.1]),         # one particle carries the population
    "tail": (DEFAULT, [30.0, 30.0, 30.0]),                              # the stress tail: m far below 0
}
SIZES = [1, 2, 2047, 2048, 2049, 3 * 2048 + 1, (1 << 17) + 63, 1 << 20, (1 << 20) + 4096 + 5]


def _run(tr, ys, scheme=MULTI, check=None):
    pf = tr.pf
    pf.init_step(None, np.array(ys[:1]))
    forms = []
    for t in range(1, len(ys)):
        ex, par = tr.resample(scheme)
        if check:
            check(ex, par)
        pf.step(np.array(ys[t:t + 1]))
        forms.append(pf.last_propagate_form())
    tr.query()
    return forms


@pytest.mark.parametrize("n", SIZES)
def test_L_ess_logml_exact_across_sizes(n):
    from modppl_amd import capi

    params, ys = REGIMES["default"]
    tr = Tracker(_lgssm(params, n, 100 + n % 1000), n)
    forms = _run(tr, ys)
    assert set(forms) <= {capi.MP_K1_FORM_TILE, capi.MP_K1_FORM_TWO_TILES}
    print(f"n={n} forms={forms} worst/bound={tr.worst}")


@pytest.mark.parametrize("regime", ["flat", "peaked", "survivor", "tail"])
@pytest.mark.parametrize("n", [2049, (1 << 20) + 4096 + 5])
def test_L_ess_logml_exact_across_weight_regimes(regime, n):
    params, ys = REGIMES[regime]
    tr = Tracker(_lgssm(params, n, 7), n)

    def check(ex, par):
        if regime == "survivor":   # every multinomial parent is the arg-max particle
            assert ex.p.max() == 1.0
            assert np.all(par == int(np.argmax(ex.p)))
        if regime == "peaked":
            assert ex.m - ex.lw_min > 1e5
    _run(tr, ys, check=check)
    print(f"{regime} n={n} worst/bound={tr.worst}")


def test_largest_job_flat_weights():
    """2^24 particles, S = 38 (its smallest), flat weights: Q = Z 2^S close to 2^62; systematic draws within the derived slack"""
    n = 1 << 24
    params, ys = REGIMES["flat"]
    tr = Tracker(_lgssm(params, n, 3), n)

    def check(ex, par):
        c = np.bincount(par, minlength=n)
        assert np.all(np.abs(c - n * ex.p) <= ex.count_slack(1.0))
    _run(tr, ys[:2], scheme=SYS, check=check)
    print(f"2^24 worst/bound={tr.worst}")


def test_two_tile_kernel_normalisation_exact():
    """k_propagate_mt (MP_K1_FORM_TWO_TILES): the multinomial draws deferred into the next step's kernel, whose level 0 then feeds the
    next fold"""
    from modppl_amd import capi

    n = 1 << 20
    params, ys = REGIMES["default"]
    pf = _lgssm(params, n, 12)
    tr = Tracker(pf, n)
    pf.init_step(None, np.array(ys[:1]))
    lnN = math.log(n)
    exact, bound = 0.0, 0.0
    for t in range(1, len(ys)):
        ex = tr.query()
        exact += float(ex.L - np.longdouble(lnN))
        bound += ex.L_bound(float(ex.L)) + 2 * U * lnN + 2 * U * (abs(exact) + abs(float(ex.L)) + lnN)
        tr.lml_exact, tr.lml_bound = exact, bound
        pf.resample(sync=False)
        pf.step(np.array(ys[t:t + 1]))
        assert pf.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES
    tr.query()


@pytest.mark.parametrize("scheme", [SYS, STRAT])
@pytest.mark.parametrize("n", [2049, (1 << 17) + 63, 1 << 20])
def test_lattice_offspring_counts_within_the_derived_slack(n, scheme):
    """offspring within 1 (systematic) or 2 (stratified) of N p_i with p_i exact, plus only the slack the fixed point accounts for"""
    params, ys = REGIMES["default"]
    tr = Tracker(_lgssm(params, n, 40 + scheme), n)
    lattice = 1.0 if scheme == SYS else 2.0

    def check(ex, par):
        c = np.bincount(par, minlength=n)
        slack = ex.count_slack(lattice)
        assert np.all(np.abs(c - n * ex.p) <= slack), float(np.max(np.abs(c - n * ex.p) - slack))
        assert np.all(np.diff(par) >= 0)
    _run(tr, ys, scheme=scheme, check=check)


def _g_test(counts, expected, min_expected):
    """G statistic over bins pooled in index order to an expected count >= min_expected; -> (p-value, bins).  (At 5 expected per bin
    the chi-square law of G is off by several of its standard deviations over 10^5 bins, even with Williams' correction: exact
    multinomial samples gave p ~ 1e-5; from 20 on it is calibrated.)"""
    from scipy import stats

    eb, ob = [], []
    acc_e = acc_o = 0.0
    for e, o in zip(expected.tolist(), counts.tolist()):
        acc_e += e
        acc_o += o
        if acc_e >= min_expected:
            eb.append(acc_e); ob.append(acc_o)
            acc_e = acc_o = 0.0
    eb[-1] += acc_e
    ob[-1] += acc_o
    e, o = np.array(eb), np.array(ob)
    nz = o > 0
    G = 2.0 * np.sum(o[nz] * np.log(o[nz] / e[nz]))
    k, total = e.size, o.sum()
    q = 1.0 + (k * k - 1.0) / (6.0 * total * (k - 1.0))   # Williams' correction: at ~5 expected per bin G alone runs ~3 % high
    return float(stats.chi2.sf(G / q, k - 1)), k


@pytest.mark.parametrize("seed", [5, 6])
def test_multinomial_g_test_at_2_20(seed):
    n = 1 << 20
    params, ys = REGIMES["default"]
    tr = Tracker(_lgssm(params, n, seed), n)
    pvals = []

    def check(ex, par):
        c = np.bincount(par, minlength=n)
        for pool in (20.0, n / 64):   # ~5 * 10^4 bins, and 64 for the large-scale shape
            pv, bins = _g_test(c, n * ex.p, pool)
            pvals.append((pv, bins))
            assert pv > 1e-6, (pv, bins)
        assert c[ex.p == 0.0].sum() == 0
    _run(tr, ys, check=check)
    print(f"G-test seed {seed}: {pvals}")


def test_minus_inf_mixture_never_drawn():
    """the HMM with impossible emissions (state 0 never emits 1): -inf log-weights are left out of Z, Z2 and every draw"""
    import modppl_amd

    prior, emis, trans = [0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]]
    data = [1.0, 0.0, 1.0, 1.0, 0.0]
    for n, scheme in ((6000, MULTI), ((1 << 20) + 4096 + 5, MULTI), ((1 << 17) + 63, SYS)):
        pf = modppl_amd.ParticleSystem(modppl_amd.hmm_model(prior, emis, trans), n, 7)
        tr = Tracker(pf, n)
        seen = []

        def check(ex, par):
            if ex.dead.any():
                seen.append(True)
                assert not np.isin(par, np.flatnonzero(ex.dead)).any()
        _run(tr, data, scheme=scheme, check=check)
        assert seen


@pytest.mark.parametrize("kind", ["band16", "dense16"])
def test_wide_state_kernels_normalisation_exact(kind):
    import modppl_amd
    from modppl_amd import capi

    n, T = 3 * 2048 + 1, 4
    if kind == "band16":
        model, form = modppl_amd.lgssm_band_model(16), capi.MP_K1_FORM_TILE
    else:
        from tests.test_gpu_dense import dense_problem
        model, form = modppl_amd.lgssm_dense_model(*dense_problem(7), 1.0), capi.MP_K1_FORM_DENSE16
    obs = np.random.default_rng(3).normal(0, 1.2, size=(T, 16))
    pf = modppl_amd.ParticleSystem(model, n, 9)
    tr = Tracker(pf, n)
    pf.init_step(None, obs[:1])
    for t in range(1, T):
        tr.resample(SYS if t == 2 else MULTI)
        pf.step(obs[t:t + 1])
        assert pf.last_propagate_form() == form
    tr.query()


def test_sharded_world_one_normalisation_exact():
    import modppl_amd
    from modppl_amd.distributed import ShardedParticleSystem

    n = (1 << 17) + 63
    params, ys = REGIMES["default"]
    pf = ShardedParticleSystem(modppl_amd.lgssm_model(*params), n, 8)
    tr = Tracker(pf, n)
    pf.init_step(None, np.array(ys[:1]))
    for t in range(1, len(ys)):
        tr.resample(MULTI if t == 1 else SYS)
        pf.step(np.array(ys[t:t + 1]))
    tr.query()


@pytest.mark.parametrize("n", [10_000, 1 << 20])
def test_fn_importance_log_ml_exact(n):
    """mp_fn_importance_sampling / _resampling: the log-ML against the exact log-mean-exp of the importance weights.  The call returns
    the NORMALISED log-weights; the weights themselves are the generate weights of the same seed, which a FunctionChains made with it
    reports as `initial_weights`."""
    import modppl_amd
    from tests.test_gpu_fn_importance import HIER, _hier_data

    xs, cons = _hier_data()
    _, lnw, lml_is = modppl_amd.fn_importance_sampling(HIER, xs, cons, n, 21, traces=False)
    _, idx, lml = modppl_amd.fn_importance_resampling(HIER, xs, cons, n, 64, 21, traces=False)
    assert lml == lml_is
    w = modppl_amd.FunctionChains(HIER, xs, cons, n, 21).initial_weights
    ex = Exact(w)
    # the returned log-weights are w - L: within the L bound (+ the subtraction's rounding) of w - (m + ln Z)
    assert np.all(np.abs(lnw - (w - float(ex.L))) <= ex.L_bound(float(ex.L)) + U * np.abs(lnw))
    lnN = math.log(n)
    want = ex.L - np.longdouble(lnN)
    bound = ex.L_bound(lml) + 2 * U * lnN + 2 * U * (abs(float(ex.L)) + lnN)
    assert abs(np.longdouble(lml) - want) <= bound, (lml, float(want), bound)
    print(f"fn importance n={n}: |log-ML error| / bound = {float(abs(np.longdouble(lml) - want)) / bound}")
    assert np.isfinite(w[idx.astype(np.int64)]).all()
