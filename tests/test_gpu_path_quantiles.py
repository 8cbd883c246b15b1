"""GPU: ParticleSystem.path_quantiles() (mp_pf_path_quantiles) — the weighted quantiles of the state at every time step over the
recorded ancestry, selected on the device.  The cases and loops are those of tests/test_gpu_path_moments.py.

Every check goes through the C ABI and compares BITS with the restatement (tests/quantiles_ref.py; DESIGN.md section 4, "Quantiles")
applied per time step to `pf.trajectories()` and `pf.log_weights` read back in the same state:
  * every width; a resample as the last event; several history slabs (band4, T = 40); -inf weights (the HMM);
  * the last row equals quantiles();
  * every status of the entry point that a handle of the compiled models reaches (tests/test_gpu_quantiles.py::test_statuses names the
    others), the cap on selectors; invisibility at n = 800.
Without mp_pf_path_quantiles every test here fails at the missing symbol or method."""
import ctypes as C

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import quantiles_ref as Q
from tests.test_gpu_path_moments import _make, _run, wide_case

pytestmark = pytest.mark.gpu

QS = [0.5, 0.05, 0.95, 0.0, 1.0, 0.5]       # unsorted, with a duplicate


def check_against_readback(pf, qs=QS, what=""):
    got = pf.path_quantiles(qs)
    paths, lw = pf.trajectories(), pf.log_weights
    T, d = pf.time, pf.model.dim_state
    assert got.shape == (T, len(qs), d)
    want = Q.path_quantiles(paths, lw, qs)
    assert Q.same_bits(got, want), (what, got, want)
    assert Q.same_bits(got[-1], pf.quantiles(qs)), (what, got[-1])
    return got, paths, lw


def test_lgssm_some_steps_without_a_resample_then_a_resample_last():
    """n = 800 is ragged (not a multiple of 256 * 8)"""
    import modppl_amd

    T, n = 12, 800
    ys = O.lgssm_observations(T)
    pf = _make(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 4)
    pf.init_step(None, ys[:1])
    check_against_readback(pf, what="lgssm1, time 1")
    for t in range(1, T):
        if t % 4 != 0:
            pf.resample()
        pf.step(ys[t:t + 1])
    got, paths, lw = check_against_readback(pf, what="lgssm1, a step last")
    assert np.unique(lw).size > 1
    worst = max(Q.check_mass(paths[:, t, 0], lw, QS, got[t, :, 0]) for t in range(T))
    print(f"lgssm1: n = {n}, T = {T}, eps = {Q.mass_epsilon(n):.3e}, worst slack / eps = {worst:.3f}")
    pf.resample(sync=False)          # the last event is a resample: its draws are deferred and the weights are zero
    got, paths, lw = check_against_readback(pf, what="lgssm1, a resample last")
    assert not lw.any()
    assert Q.same_bits(got[:, 3, 0], paths[:, :, 0].min(axis=0)) and Q.same_bits(got[:, 4, 0], paths[:, :, 0].max(axis=0))


@pytest.mark.parametrize("name", ["band4", "spiral", "band16", "one"])
def test_other_widths(name):
    model, args0, obs, n = wide_case(name)
    pf = _make(model, n, 20260401)
    _run(pf, args0, obs)
    got, paths, lw = check_against_readback(pf, what=name)
    assert got.shape[0] == len(obs)
    pf.resample(sync=False)
    check_against_readback(pf, what=name + ", a resample last")
    if name == "band16":             # sixteen levels of sixteen columns: sixteen chunks of selectors per step
        qs16 = [k / 15 for k in range(16)]
        check_against_readback(pf, qs16, name + ", 16 levels")
        check_against_readback(pf, [0.25], name + ", 1 level")


def test_minus_inf_weights_are_never_returned():
    """the HMM with impossible emissions of test_gpu_path_moments.py: state 0 never emits 1"""
    import modppl_amd

    n = 2049
    prior, emis, trans = [0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]]
    data = np.array([[1.0], [0.0], [1.0]])
    pf = _make(modppl_amd.hmm_model(prior, emis, trans), n, 7)
    pf.init_step(None, data[:1])
    pf.step(data[1:2])
    pf.step(data[2:3])                # no resample: every slot is its own lineage, a part of them dead
    got, paths, lw = check_against_readback(pf, what="hmm steps")
    dead = lw == -np.inf
    assert dead.any() and not dead.all()
    assert (got[0] == 1.0).all() and (got[2] == 1.0).all()        # every live lineage sat in state 1 when it saw a 1
    assert got[1, 3, 0] == 0.0 and got[1, 4, 0] == 1.0


def test_all_minus_inf_is_degenerate():
    import modppl_amd
    from modppl_amd import capi

    pf = _make(modppl_amd.hmm_model([0.5, 0.5], [[1.0, 1.0], [0.0, 0.0]], [[0.9, 0.3], [0.1, 0.7]]), 5000, 3)
    pf.init_step(None, [[0.0]])
    pf.path_quantiles([0.5])
    pf.step([[1.0]])               # an observation no state can emit
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.path_quantiles([0.5])
    assert err.value.code == capi.MP_ERR_DEGENERATE


def test_invisible_to_the_filter():
    """Same-seed filters; `watched` calls path_quantiles() after every asynchronous resample and after every step.  Final states,
    parents, log-weights, ESS, log-ML and the recorded trajectories are bit-equal; the forms are printed and equal."""
    import modppl_amd

    n, T = 800, 12
    ys = O.lgssm_observations(T).reshape(T, 1)
    model = modppl_amd.lgssm_model(*O.LGSSM_PARAMS)
    plain, watched = _make(model, n, 20260302), _make(model, n, 20260302)
    for pf in (plain, watched):
        pf.init_step(None, ys[:1])
    watched.path_quantiles(QS)
    for t in range(1, T):
        for pf in (plain, watched):
            pf.resample(sync=False)
        watched.path_quantiles(QS)
        for pf in (plain, watched):
            pf.step(ys[t:t + 1])
        print("step", t, "forms (plain, watched):", plain.last_propagate_form(), watched.last_propagate_form())
        assert plain.last_propagate_form() == watched.last_propagate_form()
        assert watched.path_quantiles(QS).shape == (t + 1, len(QS), 1)
    assert np.array_equal(plain.states(), watched.states())
    assert np.array_equal(plain.parents, watched.parents)
    assert np.array_equal(plain.log_weights, watched.log_weights)
    assert plain.effective_sample_size(fresh=True) == watched.effective_sample_size(fresh=True)
    assert plain.log_marginal_likelihood_estimate() == watched.log_marginal_likelihood_estimate()
    assert np.array_equal(plain.trajectories(), watched.trajectories())
    assert Q.same_bits(plain.path_quantiles(QS), watched.path_quantiles(QS))


def test_selector_cap():
    """T * n_q * dim_state above 2^18 selectors (0.5 GiB of bins) is MP_ERR_UNSUPPORTED, not a failed allocation: band16 at T = 1025 takes
    8 levels (131 200 selectors) and refuses 16 (262 400).  64 particles keep the 1025 steps short."""
    import modppl_amd
    from modppl_amd import capi

    T, n = 1025, 64
    obs = np.random.default_rng(3).normal(0, 1.2, size=(T, 16))
    pf = _make(modppl_amd.lgssm_band_model(16), n, 8)
    _run(pf, None, obs)
    with pytest.raises(capi.ModpplError) as err:
        pf.path_quantiles([k / 15 for k in range(16)])
    assert err.value.code == capi.MP_ERR_UNSUPPORTED
    qs = [k / 7 for k in range(8)]
    got = pf.path_quantiles(qs)
    assert got.shape == (T, 8, 16)
    paths, lw = pf.trajectories(), pf.log_weights
    for t in (0, 511, T - 1):
        assert Q.same_bits(got[t], Q.path_quantiles(paths[:, t:t + 1], lw, qs)[0]), t
    assert Q.same_bits(got[-1], pf.quantiles(qs))


def test_statuses():
    import modppl_amd
    from modppl_amd import capi
    from modppl_amd.distributed import HipShardEngine

    model, ys = modppl_amd.lgssm_model(*O.LGSSM_PARAMS), O.lgssm_observations(4).reshape(4, 1)
    L = capi.load()
    dp = C.POINTER(C.c_double)
    t = C.c_int32(-1)
    buf = np.full(64, np.nan)
    o = buf.ctypes.data_as(dp)
    q = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(dp)

    no_flag = modppl_amd.ParticleSystem(model, 64, 1)
    no_flag.init_step(None, ys[:1])
    with pytest.raises(capi.ModpplError) as err:
        no_flag.path_quantiles([0.5])
    assert err.value.code == capi.MP_ERR_STATE

    early = _make(model, 64, 1)
    assert L.mp_pf_path_quantiles(early._h, q(0.5), 1, o, C.byref(t)) == capi.MP_ERR_STATE

    eng = HipShardEngine(model, 2048, 4096, 0, 21)      # the first of two shards
    eng.init_step(None, ys[:1])
    assert L.mp_pf_path_quantiles(eng._h, q(0.5), 1, o, C.byref(t)) == capi.MP_ERR_UNSUPPORTED

    pf = _make(model, 3000, 5)
    _run(pf, None, ys)
    assert L.mp_pf_path_quantiles(None, q(0.5), 1, o, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(pf._h, None, 1, o, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(pf._h, q(0.5), 1, None, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(pf._h, q(0.5), 1, o, None) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(pf._h, q(0.5), 0, o, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_path_quantiles(pf._h, q(*([0.5] * 17)), 17, o, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    for bad in (np.nan, -0.5, 1.5):
        assert L.mp_pf_path_quantiles(pf._h, q(bad), 1, o, C.byref(t)) == capi.MP_ERR_INVALID_ARG
    assert t.value == -1 and np.isnan(buf).all()        # nothing was written
    assert L.mp_pf_path_quantiles(pf._h, q(0.5, 0.9), 2, o, C.byref(t)) == capi.MP_OK
    assert t.value == 4 and Q.same_bits(buf[:8].reshape(4, 2, 1), pf.path_quantiles([0.5, 0.9]))
