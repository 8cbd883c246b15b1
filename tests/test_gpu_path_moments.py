"""GPU: ParticleSystem.path_moments() (mp_pf_path_moments) — the smoothed mean and variance of the state at every time step over the
recorded ancestry, and the number of distinct ancestors per step, reduced on the device.

Every check goes through the C ABI and compares with `same_numbers` (bit-equal up to the sign of a zero):
  * the numpy restatement (tests/path_moments_ref.py; DESIGN.md section 4, "Path moments") fed with `pf.trajectories()` and
    `pf.log_weights` read back in the same state; for the LGSSM also the ancestry rebuilt from a lock-step checker's states and parents;
  * `moments()`: the last row is its mean and the diagonal of its covariance;
  * the outside truth (long-double exponentials, math.fsum) within the bounds derived from the definition's operations;
  * invisibility: a filter that calls path_moments() everywhere computes the same bits as one that never does;
  * -inf weights, the degenerate cloud, every status of the entry point, NULL outputs through the raw call.
Without mp_pf_path_moments every test here fails at the missing symbol or method.

MP_ERR_UNSUPPORTED for a dim_state outside {1, 2, 4, 16} has no test: no compiled model has such a width, so no handle reaches it."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import moments_ref as R
from tests import oracle_lib as O
from tests import path_moments_ref as P

pytestmark = pytest.mark.gpu


def _make(model, n, seed):
    import modppl_amd
    from modppl_amd import capi

    return modppl_amd.ParticleSystem(model, n, seed, flags=capi.MP_PF_RECORD_HISTORY)


def check_against_readback(pf, what=""):
    """path_moments() against the restatement on what the handle hands back in the same state, against moments(), and mean-only /
    no-distinct calls against the full one  ->  (mean, var, distinct, paths, lw)"""
    mean, var, k = pf.path_moments(var=True, distinct=True)
    paths, lw = pf.trajectories(), pf.log_weights
    T, d = pf.time, pf.model.dim_state
    assert mean.shape == var.shape == (T, d) and k.shape == (T,) and k.dtype == np.uint64
    rm, rv = P.path_moments(paths, lw)
    assert R.same_numbers(mean, rm), (what, mean, rm)
    assert R.same_numbers(var, rv), (what, var, rv)
    assert np.all(np.diff(k.astype(np.int64)) >= 0) and 1 <= k[0] and k[-1] <= len(lw)
    m, c = pf.moments()
    assert R.same_numbers(mean[-1], m) and R.same_numbers(var[-1], np.diag(c)), (what, mean[-1], m, var[-1], np.diag(c))
    m1, v1, k1 = pf.path_moments(var=False)
    assert v1 is None and k1 is None and np.array_equal(m1, mean, equal_nan=True)
    return mean, var, k, paths, lw


def test_lgssm_against_restatement_and_independent_ancestry():
    """n = 800 is ragged (not a multiple of 256 * 8); some steps come without a resample"""
    import modppl_amd

    T, n, seed = 12, 800, 4
    ys = O.lgssm_observations(T)
    pf = _make(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, seed)
    dyn = O.OraclePF(1, 1, 1, O.LGSSM_PARAMS, n, seed, O.VARIANT_CANONICAL)
    pf.init_step(None, ys[:1])
    dyn.init_step(ys[:1])
    xs, events = [dyn.state().copy()], [None]
    for t in range(1, T):
        if t % 4 != 0:
            pf.resample()
            dyn.resample()
            events.append(dyn.parents().copy())
        pf.step(ys[t:t + 1])
        dyn.step(ys[t:t + 1])
        xs.append(dyn.state().copy())
        events.append(None)

    def against_checker(what):
        mean, var, k, paths, lw = check_against_readback(pf, what)
        anc = P.ancestors(n, events)
        own = P.gather(xs, anc)
        assert np.array_equal(own, paths)
        cm, cv = P.path_moments(own, dyn.log_weights())
        assert R.same_numbers(mean, cm) and R.same_numbers(var, cv), (what, mean, cm)
        assert np.array_equal(k, P.distinct(anc)), (what, k, P.distinct(anc))
        return k, lw

    k, lw = against_checker("lgssm1, a step last")
    assert np.unique(lw).size > 1 and k[-1] == n and k[0] < n
    pf.resample(sync=False)          # the last event is a resample: its draws are deferred and the weights are zero
    dyn.resample()
    events.append(dyn.parents().copy())
    k, lw = against_checker("lgssm1, a resample last")
    assert not lw.any() and k[-1] < n


@functools.lru_cache(maxsize=None)
def wide_case(name):
    """-> (model, args0, obs [T, dim_obs], n)"""
    import modppl_amd
    from tests.test_gpu_pf_models import spiral_obs

    if name == "band4":       # several history slabs
        return modppl_amd.lgssm_band_model(4), None, np.random.default_rng(3).normal(0, 1.2, size=(40, 4)), 3000
    if name == "spiral":
        return modppl_amd.spiral_model(), [0.0, 0.0], spiral_obs(5), 1000
    if name == "band16":      # R = 4 slots per lane
        return modppl_amd.lgssm_band_model(16), None, np.random.default_rng(3).normal(0, 1.2, size=(6, 16)), 2500
    return modppl_amd.lgssm_model(*O.LGSSM_PARAMS), None, O.lgssm_observations(3).reshape(3, 1), 1     # "one"


def _run(pf, args0, obs):
    """init_step; {asynchronous resample; step}*  ->  the event log as tests/path_moments_ref.py walks it, from `pf.parents`"""
    pf.init_step(args0, obs[:1])
    events = [None]
    for t in range(1, len(obs)):
        pf.resample(sync=False)
        events.append(pf.parents.copy())
        pf.step(obs[t:t + 1])
        events.append(None)
    return events


@pytest.mark.parametrize("name", ["band4", "spiral", "band16", "one"])
def test_other_widths_and_bounds(name):
    model, args0, obs, n = wide_case(name)
    pf = _make(model, n, 20260401)
    events = _run(pf, args0, obs)
    mean, var, k, paths, lw = check_against_readback(pf, name)
    assert mean.shape[0] == len(obs)
    worst = P.check_bounds(paths, lw, mean, var)
    print(f"{name}: n = {n}, T = {len(obs)}, error / bound: mean {worst[0]:.3f}, var {worst[1]:.3f}; distinct {k[0]} .. {k[-1]}")
    assert np.array_equal(k, P.distinct(P.ancestors(n, events))), (k, P.distinct(P.ancestors(n, events)))
    pf.resample(sync=False)
    events.append(pf.parents.copy())
    k = check_against_readback(pf, name + ", a resample last")[2]
    assert np.array_equal(k, P.distinct(P.ancestors(n, events)))


def test_lgssm_bounds():
    import modppl_amd

    ys = O.lgssm_observations(12).reshape(12, 1)
    pf = _make(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), 800, 4)
    _run(pf, None, ys)
    mean, var, k, paths, lw = check_against_readback(pf, "lgssm1")
    worst = P.check_bounds(paths, lw, mean, var)
    print(f"lgssm1: n = 800, T = 12, error / bound: mean {worst[0]:.3f}, var {worst[1]:.3f}")


def test_large_n_closes_through_a_second_tree_level():
    """n = 2^21 + 77, d = 1: 1025 workgroups of 2048 slots, so the combine over partials takes two k_mom_tree launches"""
    import modppl_amd

    n, T = (1 << 21) + 77, 3
    ys = O.lgssm_observations(T).reshape(T, 1)
    pf = _make(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 11)
    events = _run(pf, None, ys)
    mean, var, k, paths, lw = check_against_readback(pf, "lgssm1 large")
    assert k[-1] == n and np.array_equal(k, P.distinct(P.ancestors(n, events)))


@pytest.mark.parametrize("n,T", [(800, 12), (1 << 20, 4)])
def test_invisible_to_the_filter(n, T):
    """Same-seed filters; `watched` calls path_moments(var=True, distinct=True) after every asynchronous resample (so it lands on
    draws nobody has looked up) and after every step.  Final states, parents, log-weights, ESS and log-ML are bit-equal, at 800
    particles and at 2^20, the size at which a filter WITHOUT history runs its steps as the two-tile kernel: a filter that records
    history makes every resample's draws at the resample (it copies the parents into the log), so both of these run one workgroup
    per tile — the forms are printed, and asserted equal between the two filters."""
    import modppl_amd

    ys = O.lgssm_observations(T).reshape(T, 1)
    model = modppl_amd.lgssm_model(*O.LGSSM_PARAMS)
    plain, watched = _make(model, n, 20260302), _make(model, n, 20260302)
    for pf in (plain, watched):
        pf.init_step(None, ys[:1])
    watched.path_moments(var=True, distinct=True)
    for t in range(1, T):
        for pf in (plain, watched):
            pf.resample(sync=False)
        watched.path_moments(var=True, distinct=True)
        for pf in (plain, watched):
            pf.step(ys[t:t + 1])
        print("step", t, "forms (plain, watched):", plain.last_propagate_form(), watched.last_propagate_form())
        assert plain.last_propagate_form() == watched.last_propagate_form()
        mean, var, k = watched.path_moments(var=True, distinct=True)
        assert mean.shape == (t + 1, 1) and k[-1] == n
    assert np.array_equal(plain.states(), watched.states())
    assert np.array_equal(plain.parents, watched.parents)
    assert np.array_equal(plain.log_weights, watched.log_weights)
    assert plain.effective_sample_size(fresh=True) == watched.effective_sample_size(fresh=True)
    assert plain.log_marginal_likelihood_estimate() == watched.log_marginal_likelihood_estimate()
    m, c = plain.moments()
    assert R.same_numbers(mean[-1], m) and R.same_numbers(var[-1], np.diag(c))


def test_minus_inf_weights_contribute_nothing_but_count_as_ancestors():
    """the HMM with impossible emissions of test_gpu_moments.py: state 0 never emits 1"""
    import modppl_amd

    n = 2049
    prior, emis, trans = [0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]]
    data = np.array([[1.0], [0.0], [1.0]])
    pf = _make(modppl_amd.hmm_model(prior, emis, trans), n, 7)
    pf.init_step(None, data[:1])
    mean, var, k, paths, lw = check_against_readback(pf, "hmm init")
    dead = lw == -np.inf
    assert dead.any() and not dead.all()
    assert mean[0, 0] == 1.0 and var[0, 0] == 0.0      # every live particle sits in state 1 ...
    assert k[0] == n                                    # ... and the dead ones are ancestors all the same
    pf.step(data[1:2])
    pf.step(data[2:3])                                  # no resample: every slot is its own lineage, a part of them dead again
    mean, var, k, paths, lw = check_against_readback(pf, "hmm steps")
    dead = lw == -np.inf
    assert dead.any() and not dead.all() and k.tolist() == [n, n, n]
    assert mean[0, 0] == 1.0 and var[0, 0] == 0.0 and mean[2, 0] == 1.0 and var[2, 0] == 0.0
    live = paths[~dead]
    assert 0.0 < mean[1, 0] < 1.0 and live[:, 1, 0].min() == 0.0 and live[:, 1, 0].max() == 1.0


def test_all_minus_inf_is_degenerate():
    import modppl_amd
    from modppl_amd import capi

    pf = _make(modppl_amd.hmm_model([0.5, 0.5], [[1.0, 1.0], [0.0, 0.0]], [[0.9, 0.3], [0.1, 0.7]]), 5000, 3)
    pf.init_step(None, [[0.0]])
    pf.path_moments(distinct=True)
    pf.step([[1.0]])               # an observation no state can emit
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.path_moments()
    assert err.value.code == capi.MP_ERR_DEGENERATE


def test_statuses_and_null_outputs():
    import modppl_amd
    from modppl_amd import capi
    from modppl_amd.distributed import HipShardEngine

    model, ys = modppl_amd.lgssm_model(*O.LGSSM_PARAMS), O.lgssm_observations(4).reshape(4, 1)
    L = capi.load()
    dp, up = C.POINTER(C.c_double), C.POINTER(C.c_uint64)
    t = C.c_int32(-1)
    buf = np.empty(8)

    no_flag = modppl_amd.ParticleSystem(model, 64, 1)
    no_flag.init_step(None, ys[:1])
    with pytest.raises(capi.ModpplError) as err:
        no_flag.path_moments()
    assert err.value.code == capi.MP_ERR_STATE

    early = _make(model, 64, 1)
    assert L.mp_pf_path_moments(early._h, buf.ctypes.data_as(dp), None, None, C.byref(t)) == capi.MP_ERR_STATE

    eng = HipShardEngine(model, 2048, 4096, 0, 21)      # the first of two shards
    eng.init_step(None, ys[:1])
    assert L.mp_pf_path_moments(eng._h, buf.ctypes.data_as(dp), None, None, C.byref(t)) == capi.MP_ERR_UNSUPPORTED

    pf = _make(model, 3000, 5)
    _run(pf, None, ys)
    assert L.mp_pf_path_moments(None, buf.ctypes.data_as(dp), None, None, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_moments(pf._h, None, None, None, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_moments(pf._h, buf.ctypes.data_as(dp), None, None, None) == capi.MP_ERR_INVALID_ARG

    # NULL var_out / distinct_out leave the remaining outputs as they are with every output asked for
    mean, var, k = pf.path_moments(var=True, distinct=True)
    for want_var in (False, True):
        for want_k in (False, True):
            m, v, kk = np.full((4, 1), np.nan), np.full((4, 1), np.nan), np.zeros(4, dtype=np.uint64)
            t = C.c_int32(-1)
            assert L.mp_pf_path_moments(pf._h, m.ctypes.data_as(dp), v.ctypes.data_as(dp) if want_var else None,
                                        kk.ctypes.data_as(up) if want_k else None, C.byref(t)) == capi.MP_OK
            assert t.value == 4 and np.array_equal(m, mean)
            assert np.array_equal(v, var) if want_var else np.isnan(v).all()
            assert np.array_equal(kk, k) if want_k else not kk.any()
