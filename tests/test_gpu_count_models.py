"""GPU: models over the count and positive-real distributions (modppl_amd/csrc/mp_mh_models_counts.h, mp_models_counts.h):
  * kind 130, the Poisson model at the end of the reference's test_update (modppl/tests/dyngenfn.rs:277-301): its exact weight;
  * kind 131, a Poisson change point under regen_mh, against its exact posterior (a sum over tau of gamma-Poisson marginals);
  * kind 132, beta-geometric: importance sampling's log-ML against the exact beta-function ratio, regen_mh's posterior mean;
  * unfold kind 101, a Poisson state-space model through the particle filter at 2^20 particles (the two-tile k_propagate_mt):
    its log-weights bit for bit against the host distributions, the one-tile kernel bit for bit, its log-ML against a grid filter."""
import math

import numpy as np
import pytest

from tests import dists_shim as S

pytestmark = pytest.mark.gpu
UNKNOWN = 1


def test_reference_test_update_poisson_model():
    """dyngenfn.rs:286-300: generate with k = 3, update to k = 1 under ArgDiff::Unknown; the weight is
    poisson.logpdf(1, 5) - poisson.logpdf(3, 5) (the uniform(0, 1) log-densities of the values are 0), bit for bit"""
    import modppl_amd
    from modppl_amd.models import MP_FN_POISSON_UPDATE

    K, V0 = 0, 1
    n = 4096
    fc = modppl_amd.FunctionChains(MP_FN_POISSON_UPDATE, [5.0], {K: 3.0}, n, 11)
    v0, p0 = fc.trace()
    assert (p0 == 0b1111).all() and (v0[:, K] == 3.).all()
    w, (dv, dp) = fc.update({K: 1.0}, argdiff=UNKNOWN)
    want = S.logpdf(S.POISSON, [1.], 5.)[0] - S.logpdf(S.POISSON, [3.], 5.)[0]
    assert abs(want - math.log(6. / 25.)) < 1e-15
    assert np.array_equal(w.view(np.uint64), np.full(n, want).view(np.uint64))
    # the discard: value/1 and value/2 (sites V0 + 1, V0 + 2) with their previous values, and the replaced k = 3
    assert (dp == (1 << K) | (1 << (V0 + 1)) | (1 << (V0 + 2))).all()
    assert (dv[:, K] == 3.).all()
    assert np.array_equal(dv[:, V0 + 1:V0 + 3], v0[:, V0 + 1:V0 + 3])
    v1, p1 = fc.trace()
    assert (p1 == (1 << K) | (1 << V0)).all() and (v1[:, K] == 1.).all() and np.array_equal(v1[:, V0], v0[:, V0])


def test_poisson_update_model_cap_is_the_panic_path():
    import modppl_amd
    from modppl_amd import capi
    from modppl_amd.models import MP_FN_POISSON_UPDATE

    with pytest.raises(capi.ModpplError) as err:
        modppl_amd.FunctionChains(MP_FN_POISSON_UPDATE, [5.0], {0: 40.0}, 256, 1)
    assert err.value.code == capi.MP_ERR_STATE


# ---- kind 131: Poisson change point ---------------------------------------------------------------------------------------------
CP_A, CP_B = 2.0, 2.0   # gamma shape, scale
CP_Y = np.array([2, 1, 3, 2, 0, 4, 1, 2, 3, 1, 7, 9, 6, 8, 5, 7, 10, 6, 8, 7], dtype=np.float64)


def changepoint_posterior(y, a, b):
    """exact: p(tau | y) over tau = 1 .. n - 1, and E[l1 | y], E[l2 | y] (l ~ gamma(shape a, scale b), conjugate per segment)"""
    n = y.size

    def log_marg(seg):
        m, s = seg.size, float(seg.sum())
        return (math.lgamma(a + s) - math.lgamma(a) - a * math.log(b) - (a + s) * math.log(m + 1. / b)
                - sum(math.lgamma(v + 1.) for v in seg))

    taus = np.arange(1, n)
    lp = np.array([log_marg(y[:t]) + log_marg(y[t:]) for t in taus])
    p = np.exp(lp - lp.max())
    p /= p.sum()
    e1 = sum(pi * (a + y[:t].sum()) / (t + 1. / b) for pi, t in zip(p, taus))
    e2 = sum(pi * (a + y[t:].sum()) / (n - t + 1. / b) for pi, t in zip(p, taus))
    return taus, p, e1, e2


def test_changepoint_regen_mh_matches_the_exact_posterior():
    import modppl_amd
    from modppl_amd.models import MP_FN_CHANGEPOINT

    TAU, L1, L2, Y0 = 0, 1, 2, 3
    n = CP_Y.size
    cons = {Y0 + j: float(v) for j, v in enumerate(CP_Y)}
    fc = modppl_amd.FunctionChains(MP_FN_CHANGEPOINT, [n, CP_A, CP_B], cons, 1 << 20, 2024)
    fc.regen_mh([TAU, L1, L2], n_iters=600, cycle=True)
    vals, _ = fc.trace()
    taus, p, e1, e2 = changepoint_posterior(CP_Y, CP_A, CP_B)
    hist = np.bincount(vals[:, TAU].astype(np.int64), minlength=n)[1:n] / vals.shape[0]
    tv = 0.5 * np.abs(hist - p).sum()
    assert tv < 0.01, (tv, hist, p)
    assert abs(vals[:, L1].mean() / e1 - 1.) < 0.01, (vals[:, L1].mean(), e1)
    assert abs(vals[:, L2].mean() / e2 - 1.) < 0.01, (vals[:, L2].mean(), e2)


def test_changepoint_simulate_prior_predictive_is_negative_binomial():
    """y_0 | l1 ~ poisson(l1), l1 ~ gamma(a, scale b): marginally negative binomial, mean a b, variance a b + a b^2"""
    import modppl_amd
    from modppl_amd.models import MP_FN_CHANGEPOINT

    N = 1 << 20
    fc = modppl_amd.FunctionChains(MP_FN_CHANGEPOINT, [CP_Y.size, CP_A, CP_B], {}, N, 77, simulate=True)
    vals, present = fc.trace()
    assert (present == (1 << (3 + CP_Y.size)) - 1).all()
    y0 = vals[:, 3]
    assert (y0 == np.floor(y0)).all() and (y0 >= 0).all()
    mean, var = CP_A * CP_B, CP_A * CP_B + CP_A * CP_B ** 2
    assert abs(y0.mean() - mean) < 5 * math.sqrt(var / N)
    assert abs(y0.var() / var - 1.) < 0.02
    tau = vals[:, 0]
    assert tau.min() == 1 and tau.max() == CP_Y.size - 1 and (vals[:, 1:3] > 0).all()


# ---- kind 132: beta-geometric ---------------------------------------------------------------------------------------------------
BG_A, BG_B = 2.0, 3.0
BG_K = np.array([1, 4, 0, 2, 3, 0, 1, 6, 2, 0, 1, 3, 5, 0, 2, 1, 0, 4, 2, 1, 3, 0, 1, 2, 7, 0, 1, 2, 3, 1], dtype=np.float64)


def _log_beta(a, b):
    return math.lgamma(a) + math.lgamma(b) - math.lgamma(a + b)


def test_beta_geometric_importance_sampling_log_ml():
    import modppl_amd
    from modppl_amd.models import MP_FN_BETA_GEOMETRIC

    n, N = BG_K.size, 1 << 20
    cons = {1 + j: float(v) for j, v in enumerate(BG_K)}
    _, lnw, lml = modppl_amd.fn_importance_sampling(MP_FN_BETA_GEOMETRIC, [n, BG_A, BG_B], cons, N, 5, traces=False)
    exact = _log_beta(BG_A + n, BG_B + BG_K.sum()) - _log_beta(BG_A, BG_B)
    w = np.exp(lnw)   # normalised weights
    se = math.sqrt(max(N * float(np.sum(w * w)) - 1., 0.) / N)   # delta method: Var(log Z_hat) ~ (E w^2 / (E w)^2 - 1) / N
    assert abs(lml - exact) <= 4 * se, (lml, exact, se)
    assert se < 0.05


def test_beta_geometric_regen_mh_posterior_mean():
    import modppl_amd
    from modppl_amd.models import MP_FN_BETA_GEOMETRIC

    n = BG_K.size
    cons = {1 + j: float(v) for j, v in enumerate(BG_K)}
    fc = modppl_amd.FunctionChains(MP_FN_BETA_GEOMETRIC, [n, BG_A, BG_B], cons, 1 << 20, 9)
    fc.regen_mh([0], n_iters=300)
    vals, _ = fc.trace()
    want = (BG_A + n) / (BG_A + BG_B + n + BG_K.sum())
    assert abs(vals[:, 0].mean() / want - 1.) < 0.01, (vals[:, 0].mean(), want)
    assert (vals[:, 0] > 0).all() and (vals[:, 0] < 1).all()


# ---- unfold kind 101: Poisson state-space model -----------------------------------------------------------------------------------
PS = (0.5, 0.9, 0.3, 0.5)   # mu, phi, sigma, sig0
T_PS = 24


def poisson_ssm_observations(T=T_PS, seed=5):
    mu, phi, sigma, sig0 = PS
    rng = np.random.default_rng(seed)
    h = mu + sig0 * rng.standard_normal()
    ys = []
    for t in range(T):
        if t:
            h = mu + phi * (h - mu) + sigma * rng.standard_normal()
        ys.append(float(rng.poisson(math.exp(h))))
    return np.array(ys).reshape(T, 1)


def grid_log_ml(obs, points=3001):
    """the model written down independently: a deterministic filter over h on a grid (trapezoid weights)"""
    mu, phi, sigma, sig0 = PS
    sd = max(sig0, sigma / math.sqrt(1. - phi * phi))
    hs = np.linspace(mu - 9. * sd, mu + 9. * sd, points)
    dh = hs[1] - hs[0]
    wq = np.full(hs.size, dh)
    wq[0] = wq[-1] = dh / 2

    def npdf(x, m, s):
        return np.exp(-0.5 * ((x - m) / s) ** 2) / (s * math.sqrt(2. * math.pi))

    trans = npdf(hs[None, :], mu + phi * (hs[:, None] - mu), sigma)
    pred = npdf(hs, mu, sig0)
    log_ml, post = 0., None
    for t in range(obs.shape[0]):
        if t:
            pred = (post * wq) @ trans
        y = obs[t, 0]
        like = np.exp(y * hs - np.exp(hs) - math.lgamma(y + 1.))
        z = float(np.sum(pred * like * wq))
        log_ml += math.log(z)
        post = pred * like / z
    return log_ml


def _expected_logw(y, states):
    """what a step leaves in the log-weights after a resample: 0 + (0 + poisson.logpdf(y, exp(h)))"""
    rates = S.exp(states[:, 0])
    return 0. + (0. + S.logpdf(S.POISSON, np.full(rates.size, y), rates))


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def test_poisson_ssm_two_tile_kernel_weights_bit_exact():
    import modppl_amd
    from modppl_amd import capi

    obs = poisson_ssm_observations()
    n = 1 << 20
    pf = modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*PS), n, 31)
    pf.init_step(None, obs[:1])
    assert np.array_equal(_bits(pf.log_weights), _bits(0. + S.logpdf(S.POISSON, np.full(n, obs[0, 0]), S.exp(pf.states()[:, 0]))))
    for t in range(1, T_PS):
        pf.resample(sync=False)
        pf.step(obs[t:t + 1])
        assert pf.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES
        assert np.array_equal(_bits(pf.log_weights), _bits(_expected_logw(obs[t, 0], pf.states())))
    assert np.isfinite(pf.log_marginal_likelihood_estimate())


def test_poisson_ssm_one_tile_kernel_is_the_same(diag, monkeypatch):
    """MP_K1_MT=0 (the diagnostics build) keeps k_propagate, one workgroup per tile: the same states and weights, bit for bit"""
    import modppl_amd
    from modppl_amd import capi

    obs = poisson_ssm_observations(12)
    n = 1 << 20
    mt = modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*PS), n, 8)
    monkeypatch.setenv("MP_K1_MT", "0")
    one = modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*PS), n, 8)
    monkeypatch.delenv("MP_K1_MT")
    for pf in (mt, one):
        pf.init_step(None, obs[:1])
    for t in range(1, obs.shape[0]):
        for pf in (mt, one):
            pf.resample(sync=False)
            pf.step(obs[t:t + 1])
        assert mt.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES and one.last_propagate_form() == capi.MP_K1_FORM_TILE
        assert np.array_equal(_bits(mt.states()), _bits(one.states()))
        assert np.array_equal(_bits(mt.log_weights), _bits(one.log_weights))
    assert mt.log_marginal_likelihood_estimate() == one.log_marginal_likelihood_estimate()


# |particle log-ML - grid log-ML| at 2^20 particles.  Eight seeds (20241015, 1 .. 7) on the MI355X gave differences of
# +0.0056 -0.0015 +0.0048 +0.0003 +0.0058 -0.0058 +0.0082 +0.0080 (standard deviation 0.0050): the tolerance is four of those
GRID_TOL = 0.02
GRID_SEED = 20241015


def pf_log_ml(seed, obs, n=1 << 20):
    import modppl_amd

    pf = modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*PS), n, seed)
    pf.init_step(None, obs[:1])
    for t in range(1, obs.shape[0]):
        pf.resample(sync=False)
        pf.step(obs[t:t + 1])
    return pf.log_marginal_likelihood_estimate()


def test_poisson_ssm_against_a_grid_filter():
    obs = poisson_ssm_observations()
    ref = grid_log_ml(obs)
    est = pf_log_ml(GRID_SEED, obs)
    assert abs(est - ref) < GRID_TOL, (est, ref)


def test_poisson_ssm_impossible_count_is_degenerate():
    import modppl_amd
    from modppl_amd import capi

    obs = poisson_ssm_observations(3)
    pf = modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*PS), 70001, 3)
    pf.init_step(None, obs[:1])
    pf.resample(sync=False)
    pf.step(np.array([[-1.0]]))
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.resample()
    assert err.value.code == capi.MP_ERR_DEGENERATE


def test_poisson_ssm_rejects_bad_params():
    import modppl_amd
    from modppl_amd import capi

    for bad in ([0.5, 0.9, 0.0, 0.5], [0.5, 0.9, 0.3, -1.0], [np.nan, 0.9, 0.3, 0.5]):
        with pytest.raises(capi.ModpplError) as err:
            modppl_amd.ParticleSystem(modppl_amd.poisson_state_space_model(*bad), 1024, 1)
        assert err.value.code == capi.MP_ERR_INVALID_ARG
    with pytest.raises(capi.ModpplError):
        modppl_amd.ParticleSystem(modppl_amd.UnfoldModel(101, 1, 1, [0.5, 0.9, 0.3], "short"), 1024, 1)
