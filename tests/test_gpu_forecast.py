"""GPU: ParticleSystem.forecast() / forecast_paths() (mp_pf_forecast_moments / mp_pf_forecast_paths) — every slot runs the model in
Simulate mode from its own state with the Philox counters the next steps would use ("Forecast").

  * the paths against `simulate` after one init_step, and against the states the filter's own next unresampled steps propose: bit for bit;
  * the moments against the numpy restatement (tests/forecast_ref.py) fed with the paths and the log-weights read back in the same state;
  * windows, invisibility to the filter, the law of the forecast of an LGSSM derived from the cloud itself, -inf weights and statuses.
Without mp_pf_forecast_paths / mp_pf_forecast_moments every test here fails at the missing symbol or method.

(The MP_ERR_UNSUPPORTED of mp_pf_forecast_moments for a dim_state other than 1, 2, 4, 16 has no test: no compiled model has one.)"""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import forecast_ref as F
from tests import moments_ref as R
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 2047, 2048, 2049, (1 << 16) + 63]
MODELS = ["lgssm1", "spiral", "bearings", "band16", "dense16", "stochvol", "poisson"]
STAGES = ["init", "step", "resampled"]
HORIZONS = [1, 3]
SEED = 20260411


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> (model, args0, obs [3, dim_obs])"""
    import modppl_amd
    from tests.test_gpu_dense import dense_problem
    from tests.test_gpu_moments import problem as moments_problem

    if name == "dense16":
        A, Q, Rm = dense_problem(1)
        return modppl_amd.lgssm_dense_model(A, Q, Rm, 1.0), None, np.random.default_rng(4).normal(0, 1.2, size=(3, 16))
    if name == "stochvol":
        return modppl_amd.stochastic_volatility_model(), None, np.array([[0.31], [-0.52], [0.12]])
    if name == "poisson":
        return modppl_amd.poisson_state_space_model(), None, np.array([[1.0], [3.0], [0.0]])
    return moments_problem(name)


def new_filter(name, n, seed=SEED):
    import modppl_amd

    model, args0, obs = problem(name)
    return modppl_amd.ParticleSystem(model, n, seed), args0, obs


# ---- 1. against simulate ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_paths_equal_simulate_after_init_step(name, n):
    """after init_step slot i's forecast is trace i of simulate(model, args0, 1 + H, n, seed) at steps 1 .. H: same Philox slot, step and
    kernel time, and the state of step 0 is the same free draw"""
    import modppl_amd

    pf, args0, obs = new_filter(name, n)
    pf.init_step(args0, obs[:1])
    for H in HORIZONS:
        xs, ys = pf.forecast_paths(H)
        sx, sy = modppl_amd.simulate(pf.model, args0, 1 + H, n, SEED)
        assert xs.shape == sx[:, 1:].shape and ys.shape == sy[:, 1:].shape
        assert np.array_equal(pf.states(), sx[:, 0])
        assert np.array_equal(xs, sx[:, 1:]), (name, n, H)
        assert np.array_equal(ys, sy[:, 1:]), (name, n, H)


# ---- 2. against the filter's own next steps --------------------------------------------------------------------------------------------
def _next_steps(name, n, variant, check_form=False):
    from modppl_amd import capi

    a, args0, obs = new_filter(name, n)
    b, _, _ = new_filter(name, n)
    for pf in (a, b):
        pf.init_step(args0, obs[:1])
        for t in range(1, 4):
            if variant == "async":
                pf.resample(sync=False)      # the call below lands on draws nobody has made / a pending lazy launch
            else:
                pf.resample(scheme=capi.MP_RESAMPLE_SYSTEMATIC)
            pf.step(obs[t % 3:t % 3 + 1])
            if check_form:
                assert pf.last_propagate_form() == (capi.MP_K1_FORM_TWO_TILES if variant == "async" else capi.MP_K1_FORM_TILE)
    xs, _ = a.forecast_paths(3)
    assert a.time == b.time == 4
    for k in range(3):
        b.step(obs[(k + 2) % 3:(k + 2) % 3 + 1])          # any finite observation: the proposal does not look at it
        if check_form:
            assert b.last_propagate_form() == capi.MP_K1_FORM_TILE      # (no draws pending: one workgroup per tile)
        assert np.array_equal(b.states(), xs[:, k]), (name, n, variant, k)
    assert np.array_equal(a.forecast_paths(3)[0], xs)


@pytest.mark.parametrize("variant", ["async", "systematic"])
@pytest.mark.parametrize("name", MODELS)
def test_paths_equal_the_next_unresampled_steps(name, variant):
    _next_steps(name, 2049, variant)


@pytest.mark.parametrize("variant", ["async", "systematic"])
def test_paths_equal_the_next_steps_of_the_two_tile_kernel(variant):
    """n = 2^20: the steps behind an asynchronous multinomial resample run as k_propagate_mt (asserted), and the forecast lands on its
    lazy log-weights and parents"""
    _next_steps("lgssm1", 1 << 20, variant, check_form=True)


# ---- 3. moments against the restatement -----------------------------------------------------------------------------------------------
def _same4(got, want):
    return all((g is None and w is None) or R.same_numbers(g, w) for g, w in zip(got, want))


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_moments_equal_the_restatement(name, n, stage):
    pf, args0, obs = new_filter(name, n)
    pf.init_step(args0, obs[:1])
    if stage != "init":
        pf.step(obs[1:2])          # no resample in between: the log-weights of two steps add up
    if stage == "resampled":
        pf.resample()
    lw = pf.log_weights
    if stage == "resampled":
        assert not lw.any()
    elif n > 2:
        assert np.unique(lw).size > 1
    for H in HORIZONS:
        got = pf.forecast(H)
        xs, ys = pf.forecast_paths(H)
        want = F.forecast_moments(xs, ys, lw)
        assert got[0].shape == (H, pf.model.dim_state) and got[2].shape == (H, pf.model.dim_obs)
        assert _same4(got, want), (name, n, stage, H, got, want)
        assert np.all(got[1] >= 0) and np.all(got[3] >= 0)
    again = pf.forecast(3)
    assert all(np.array_equal(g, h) for g, h in zip(got, again))
    sm, sv, om, ov = pf.forecast(3, var=False)
    assert sv is None and ov is None and np.array_equal(sm, got[0]) and np.array_equal(om, got[2])
    sm, sv, om, ov = pf.forecast(3, obs=False)
    assert om is None and ov is None and np.array_equal(sm, got[0]) and np.array_equal(sv, got[1])
    sm, sv, om, ov = pf.forecast(3, var=False, obs=False)
    assert sv is None and om is None and ov is None and np.array_equal(sm, got[0])


# ---- 4. windows -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [2050, (1 << 16) + 63])
@pytest.mark.parametrize("name", ["lgssm1", "bearings", "band16"])
def test_windows_are_slices_of_the_full_call(name, n):
    pf, args0, obs = new_filter(name, n)
    pf.init_step(args0, obs[:1])
    pf.resample(sync=False)
    pf.step(obs[1:2])
    for H in HORIZONS:
        xs, ys = pf.forecast_paths(H)
        for first, count in [(0, 1), (2047, 3), (n - 1, 1)]:
            wx, wy = pf.forecast_paths(H, first, count)
            assert np.array_equal(wx, xs[first:first + count]) and np.array_equal(wy, ys[first:first + count]), (first, count)


# ---- 5. invisible ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 4096 + 5])
def test_invisible_to_the_filter(n):
    """The three-filter scheme of test_gpu_moments.py::test_invisible_to_the_filter: `watched` calls forecast(2) and
    forecast_paths(2, 0, 5) after every step and after every resample, synchronous and asynchronous (so the call lands on deferred draws
    nobody has made; it makes them, and the step behind it runs one workgroup per tile); `after_steps` after every step only (its steps
    make the draws themselves and run as the two-tile kernel, as the plain filter's do, and the call lands on that kernel's pending lazy
    launch).  Final states, parents, log-weights, log-ML, fresh ESS and time are bit-equal to the filter that never calls them."""
    import modppl_amd
    from modppl_amd import capi

    ys = O.lgssm_observations(7).reshape(7, 1)
    mk = lambda: modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 20260302)
    plain, watched, after_steps = mk(), mk(), mk()
    everyone = (plain, watched, after_steps)

    def look(*pfs):
        got = [(pf.forecast(2), pf.forecast_paths(2, 0, 5)) for pf in pfs]
        for g in got[1:]:
            assert _same4(g[0], got[0][0]) and np.array_equal(g[1][0], got[0][1][0]) and np.array_equal(g[1][1], got[0][1][1])

    for pf in everyone:
        pf.init_step(None, ys[:1])
    look(watched, after_steps)
    for t in range(1, 7):
        sync = t % 2 == 1
        Ls = [pf.resample(sync=sync) for pf in everyone]
        assert Ls[0] == Ls[1] == Ls[2]
        look(watched)
        for pf in everyone:
            pf.step(ys[t:t + 1])
        forms = [pf.last_propagate_form() for pf in everyone]
        assert forms == [capi.MP_K1_FORM_TWO_TILES, capi.MP_K1_FORM_TILE, capi.MP_K1_FORM_TWO_TILES], (t, forms)
        look(watched, after_steps)
    for pf in (watched, after_steps):
        assert np.array_equal(plain.states(), pf.states())
        assert np.array_equal(plain.parents, pf.parents)
        assert np.array_equal(plain.log_weights, pf.log_weights)
        assert plain.log_marginal_likelihood_estimate() == pf.log_marginal_likelihood_estimate()
        assert plain.effective_sample_size(fresh=True) == pf.effective_sample_size(fresh=True)
        assert plain.time == pf.time == 7


# ---- 6. the law, from the cloud itself ---------------------------------------------------------------------------------------------------
def test_the_law_of_an_lgssm_forecast():
    """LGSSM d = 1, n = 2^16, unequal weights w_i (normalised), H = 8.  Conditional on the cloud {x_i, w_i}: v_i(k) = a^(k+1) x_i + e_i,
    e_i ~ N(0, S_k) independent over i, S_k = sig_x^2 sum_{j<=k} a^(2j); y_i(k) = v_i(k) + N(0, sig_y^2), i.e. S_k + sig_y^2 for S_k.
      mean:  E = a^(k+1) mean_T,  sd = sqrt(S sum w^2).
      variance V = sum w (c_i + e_i)^2 - ebar^2 with c_i = a^(k+1) (x_i - mean_T), ebar = sum w e ~ N(0, S sum w^2):
             E V = a^(2(k+1)) var_T + S - S sum w^2;   Var((c + e)^2) = 4 c^2 S + 2 S^2 for a normal e (its fourth moment 3 S^2), so
             sd(sum w (c + e)^2) = sqrt(sum w^2 (4 c^2 S + 2 S^2)), sd(ebar^2) = sqrt(2) S sum w^2, and sd V <= their sum.
    Everything is derived from the cloud read back and the model's parameters; every horizon is held to 5 standard deviations."""
    import modppl_amd

    mu0, sig0, a, sig_x, sig_y = O.LGSSM_PARAMS
    n, H = 1 << 16, 8
    ys = O.lgssm_observations(2).reshape(2, 1)
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 20260412)
    pf.init_step(None, ys[:1])
    pf.step(ys[1:2])
    x = pf.states()[:, 0].astype(np.longdouble)
    lw = pf.log_weights.astype(np.longdouble)
    w = np.exp(lw - lw.max())
    w /= w.sum()
    assert np.unique(lw).size > n // 2
    mean_T = float(np.sum(w * x))
    var_T = float(np.sum(w * (x - mean_T) ** 2))
    w2 = float(np.sum(w * w))
    sm, sv, om, ov = pf.forecast(H)
    for k in range(H):
        g = a ** (k + 1)
        S_state = sig_x ** 2 * sum(a ** (2 * j) for j in range(k + 1))
        c2 = (g * (x - mean_T)) ** 2
        for what, S, mean, var in (("state", S_state, sm[k, 0], sv[k, 0]), ("obs", S_state + sig_y ** 2, om[k, 0], ov[k, 0])):
            sd_mean = np.sqrt(S * w2)
            z_mean = (mean - g * mean_T) / sd_mean
            EV = g * g * var_T + S - S * w2
            sd_var = float(np.sqrt(np.sum(w * w * (4 * c2 * S + 2 * S * S)))) + np.sqrt(2.0) * S * w2
            z_var = (var - EV) / sd_var
            print(f"k = {k} {what}: mean {mean:.6f} (z = {z_mean:+.2f}), var {var:.6f} against {EV:.6f} (z = {z_var:+.2f})")
            assert abs(z_mean) <= 5.0, (k, what, mean, g * mean_T, sd_mean)
            assert abs(z_var) <= 5.0, (k, what, var, EV, sd_var)


# ---- 7. -inf weights and statuses ----------------------------------------------------------------------------------------------------------
def test_all_minus_inf_is_degenerate_for_the_moments_only():
    import modppl_amd
    from modppl_amd import capi

    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), 5000, 3)
    pf.init_step(None, [0.3])
    pf.step([np.inf])              # logpdf = -inf for every particle
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.forecast(2)
    assert err.value.code == capi.MP_ERR_DEGENERATE
    xs, ys = pf.forecast_paths(2)
    assert xs.shape == (5000, 2, 1) and np.isfinite(xs).all() and np.isfinite(ys).all()


def test_statuses():
    import modppl_amd
    from modppl_amd import capi

    L = capi.load()
    dp = C.POINTER(C.c_double)
    buf = [np.empty(64) for _ in range(4)]
    b = [x.ctypes.data_as(dp) for x in buf]
    early = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), 8, 1)
    assert L.mp_pf_forecast_paths(early._h, 2, 0, 8, b[0], b[1]) == capi.MP_ERR_STATE
    assert L.mp_pf_forecast_moments(early._h, 2, b[0], b[1], b[2], b[3]) == capi.MP_ERR_STATE
    pf = early
    pf.init_step(None, [0.3])
    assert L.mp_pf_forecast_paths(None, 2, 0, 8, b[0], b[1]) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_moments(None, 2, b[0], b[1], b[2], b[3]) == capi.MP_ERR_INVALID_ARG
    for horizon in (0, -1):
        assert L.mp_pf_forecast_paths(pf._h, horizon, 0, 8, b[0], b[1]) == capi.MP_ERR_INVALID_ARG
        assert L.mp_pf_forecast_moments(pf._h, horizon, b[0], b[1], b[2], b[3]) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_paths(pf._h, 2, 0, 9, b[0], b[1]) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_paths(pf._h, 2, 8, 1, b[0], b[1]) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_paths(pf._h, 2, 2 ** 64 - 1, 2, b[0], b[1]) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_paths(pf._h, 2, 0, 8, None, None) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_forecast_moments(pf._h, 2, None, None, None, None) == capi.MP_ERR_INVALID_ARG
    # one output at a time
    full = pf.forecast(2)
    xs, ys = pf.forecast_paths(2)
    for j in range(4):
        args = [None] * 4
        args[j] = b[0]
        assert L.mp_pf_forecast_moments(pf._h, 2, *args) == capi.MP_OK
        assert np.array_equal(buf[0][:2], full[j][:, 0])
    assert L.mp_pf_forecast_paths(pf._h, 2, 0, 8, b[0], None) == capi.MP_OK and np.array_equal(buf[0][:16], xs.ravel())
    assert L.mp_pf_forecast_paths(pf._h, 2, 0, 8, None, b[1]) == capi.MP_OK and np.array_equal(buf[1][:16], ys.ravel())
    assert L.mp_pf_forecast_paths(pf._h, 2, 8, 0, b[0], b[1]) == capi.MP_OK       # an empty window
    # the HMM: the reason mp_unfold_simulate gives
    hmm_model = modppl_amd.hmm_model([0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]])
    with pytest.raises(capi.ModpplError) as sim_err:
        modppl_amd.simulate(hmm_model, None, 2, 8, 1)
    hmm = modppl_amd.ParticleSystem(hmm_model, 8, 1)
    hmm.init_step(None, [[1.0]])
    for call in (lambda: hmm.forecast(2), lambda: hmm.forecast_paths(2)):
        with pytest.raises(capi.ModpplError) as err:
            call()
        assert err.value.code == capi.MP_ERR_UNSUPPORTED and str(err.value) == str(sim_err.value)


def test_world_of_one_sharded_handle_and_shards_of_a_larger_world():
    import modppl_amd
    from modppl_amd import capi
    from modppl_amd.distributed import HipShardEngine, ShardedParticleSystem

    model, ys, n, seed = modppl_amd.lgssm_model(*O.LGSSM_PARAMS), O.lgssm_observations(3), 50000, 21
    one = modppl_amd.ParticleSystem(model, n, seed)
    sh = ShardedParticleSystem(model, n, seed, exchange="exact")
    for pf in (one, sh):
        pf.init_step(None, ys[:1])
        pf.resample()
        pf.step(ys[1:2])
    assert _same4(one.forecast(3), sh.forecast(3))
    a, b = one.forecast_paths(3, 5, 1000), sh.forecast_paths(3, 5, 1000)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])

    whole = modppl_amd.ParticleSystem(model, 4096, seed)
    whole.init_step(None, ys[:1])
    wx, wy = whole.forecast_paths(2)
    for rank in (0, 1):                                        # the two shards of that job: Philox is keyed by the GLOBAL slot
        eng = HipShardEngine(model, 2048, 4096, 2048 * rank, seed)
        eng.init_step(None, ys[:1].reshape(1, 1))
        with pytest.raises(capi.ModpplError) as err:
            eng.forecast(2)
        assert err.value.code == capi.MP_ERR_UNSUPPORTED
        ex, ey = eng.forecast_paths(2)
        assert np.array_equal(ex, wx[2048 * rank:2048 * (rank + 1)]) and np.array_equal(ey, wy[2048 * rank:2048 * (rank + 1)])
