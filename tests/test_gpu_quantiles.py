"""GPU: ParticleSystem.quantiles() (mp_pf_quantiles) — the weighted quantiles of every state component, selected on the device.

Every check goes through the C ABI and compares BITS (`view(uint64)`) with the restatement of the definition (tests/quantiles_ref.py;
DESIGN.md section 4, "Quantiles") fed with `pf.states()` and `pf.log_weights` read back in the same state:
  * every compiled width, ragged sizes and n = 1, before and after a resample (unequal weights, then all equal);
  * the HMM's 0 / 1 ties with -inf weights among them; the all -inf cloud (MP_ERR_DEGENERATE);
  * n = 2^20 + 77: the size that changes S (2^42 instead of 2^52) and spans many workgroups;
  * levels unsorted and duplicated, one level and sixteen; every status of the entry point;
  * invisibility: a filter that calls quantiles() everywhere computes the same bits as one that never does;
  * the mass bound against the outside truth (long-double exponentials, math.fsum): eps = 2 n / S + 2^-50.
Without mp_pf_quantiles every test here fails at the missing symbol or method."""
import ctypes as C
import functools

import numpy as np
import pytest

from tests import oracle_lib as O
from tests import quantiles_ref as Q

pytestmark = pytest.mark.gpu

QS = [0.5, 0.05, 0.95, 0.0, 1.0, 0.5, 0.1]       # unsorted, with a duplicate
QS16 = [k / 15 for k in range(16)][::-1]


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> (model, args0, obs [3, dim_obs], n)"""
    import modppl_amd
    from tests.test_gpu_pf_models import spiral_obs

    if name == "lgssm1":      # ragged: not a multiple of 256 * 8
        return modppl_amd.lgssm_model(*O.LGSSM_PARAMS), None, O.lgssm_observations(3).reshape(3, 1), 800
    if name == "one":
        return modppl_amd.lgssm_model(*O.LGSSM_PARAMS), None, O.lgssm_observations(3).reshape(3, 1), 1
    if name == "spiral":
        return modppl_amd.spiral_model(), [0.0, 0.0], spiral_obs(3), 1000
    if name == "band4":
        return modppl_amd.lgssm_band_model(4), None, np.random.default_rng(3).normal(0, 1.2, size=(3, 4)), 3000
    return modppl_amd.lgssm_band_model(16), None, np.random.default_rng(3).normal(0, 1.2, size=(3, 16)), 2500


def check_against_readback(pf, qs, what="", mass=True):
    """quantiles(qs) against the restatement (bits) and the outside truth, both on what the handle hands back in the same state"""
    got = pf.quantiles(qs)
    x, lw = pf.states(), pf.log_weights
    want = Q.pf_quantiles(x, lw, qs)
    assert got.shape == (len(qs), pf.model.dim_state)
    assert Q.same_bits(got, want), (what, got, want)
    if mass:
        worst = max(Q.check_mass(x[:, j], lw, qs, got[:, j]) for j in range(x.shape[1]))
        print(f"{what}: n = {len(lw)}, eps = {Q.mass_epsilon(len(lw)):.3e}, worst slack / eps = {worst:.3f}")
    return got, x, lw


@pytest.mark.parametrize("name", ["lgssm1", "one", "spiral", "band4", "band16"])
def test_every_width_before_and_after_a_resample(name):
    import modppl_amd

    model, args0, obs, n = problem(name)
    pf = modppl_amd.ParticleSystem(model, n, 20260501)
    pf.init_step(args0, obs[:1])
    check_against_readback(pf, QS, f"{name} init")
    pf.step(obs[1:2])                # no resample in between: the log-weights of two steps add up
    got, x, lw = check_against_readback(pf, QS, f"{name} step")
    if n > 2:
        assert np.unique(lw).size > 1
    pf.resample()
    got, x, lw = check_against_readback(pf, QS, f"{name} resampled")
    assert not lw.any()              # W_i = S for every i: plain order statistics
    s = np.sort(x, axis=0)
    assert Q.same_bits(got[3], s[0]) and Q.same_bits(got[4], s[-1])
    assert Q.same_bits(got[0], s[max(1, -(-n // 2)) - 1]) and Q.same_bits(got[0], got[5])
    a, b = pf.quantiles(QS), pf.quantiles(QS)
    assert Q.same_bits(a, b) and Q.same_bits(a, got)


@pytest.mark.parametrize("qs", [[0.5], QS16, [1.0, 0.0]])
def test_one_level_and_sixteen(qs):
    import modppl_amd

    for name in ("lgssm1", "band16"):
        model, args0, obs, n = problem(name)
        pf = modppl_amd.ParticleSystem(model, n, 9)
        pf.init_step(args0, obs[:1])
        pf.step(obs[1:2])
        check_against_readback(pf, qs, f"{name} {len(qs)} levels")


def test_hmm_ties_and_minus_inf_weights():
    """the HMM with impossible emissions of test_gpu_moments.py: state 0 never emits 1, so its particles weigh -inf; the values are 0 / 1"""
    import modppl_amd

    n = 2049
    prior, emis, trans = [0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]]
    data = np.array([[1.0], [0.0], [1.0]])
    pf = modppl_amd.ParticleSystem(modppl_amd.hmm_model(prior, emis, trans), n, 7)
    pf.init_step(None, data[:1])
    got, x, lw = check_against_readback(pf, QS, "hmm init")
    dead = lw == -np.inf
    assert dead.any() and not dead.all()
    assert (got == 1.0).all()         # every live particle sits in state 1: a dead slot's 0 is never returned, not even at q = 0
    pf.step(data[1:2])
    got, x, lw = check_against_readback(pf, QS, "hmm step")
    assert got[3, 0] == 0.0 and got[4, 0] == 1.0


def test_all_minus_inf_is_degenerate():
    import modppl_amd
    from modppl_amd import capi

    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), 5000, 3)
    pf.init_step(None, [0.3])
    pf.step([np.inf])              # logpdf = -inf for every particle
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.quantiles([0.5])
    assert err.value.code == capi.MP_ERR_DEGENERATE


def test_large_n_changes_the_scale_and_spans_many_workgroups():
    """n = 2^20 + 77, d = 1: ceil_log2(n) = 21, so S = 2^42 (below 2^20 it is 2^52); 513 workgroups flush into the same bins"""
    import modppl_amd

    n = (1 << 20) + 77
    assert Q.scale(n) == 2.0 ** 42 and Q.scale(1 << 11) == 2.0 ** 52
    ys = O.lgssm_observations(3).reshape(3, 1)
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 11)
    pf.init_step(None, ys[:1])
    pf.step(ys[1:2])
    got, x, lw = check_against_readback(pf, QS, "lgssm1 large")
    assert np.unique(lw).size > 1
    pf.resample(sync=False)
    check_against_readback(pf, QS, "lgssm1 large, resampled", mass=False)


@pytest.mark.parametrize("history", [True, False])
@pytest.mark.parametrize("n,T", [(800, 7), (1 << 20, 5)])
def test_invisible_to_the_filter(n, T, history):
    """Same-seed filters.  `watched` calls quantiles() after every asynchronous resample (so it lands on draws nobody has looked up)
    and after every step; `after_steps` after every step only, so behind an asynchronous resample its call lands on the pending lazy
    launch of the step before.  Final states, parents, log-weights, ESS and log-ML of both are bit-equal to the plain filter's, at 800
    particles and at 2^20, and the kernel form of EVERY step is asserted:
      * `after_steps` takes the plain filter's form at every step, everywhere;
      * `watched` does too at 800 particles and wherever the filters record history (they make every resample's draws at the resample,
        so a call in between finds nothing pending);
      * at 2^20 without history an asynchronous resample leaves its draws to the next step, and ANY read in between (states(),
        moments(), quantiles() alike: they bring the handle to a readable state the same way) makes them first; the step behind it finds
        none pending and runs one workgroup per tile where the other two draw themselves in the two-tile kernel.  That documented
        triple [TWO_TILES, TWO_TILES, TILE] is what tests/test_gpu_moments.py asserts for moments(), and it is asserted here."""
    import modppl_amd
    from modppl_amd import capi

    ys = O.lgssm_observations(T).reshape(T, 1)
    flags = capi.MP_PF_RECORD_HISTORY if history else 0
    mk = lambda: modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 20260302, flags=flags)
    plain, after_steps, watched = mk(), mk(), mk()
    everyone = (plain, after_steps, watched)
    for pf in everyone:
        pf.init_step(None, ys[:1])
    first = watched.quantiles(QS)
    assert Q.same_bits(first, after_steps.quantiles(QS))
    for t in range(1, T):
        for pf in everyone:
            pf.resample(sync=False)
        watched.quantiles(QS)
        for pf in everyone:
            pf.step(ys[t:t + 1])
        forms = [pf.last_propagate_form() for pf in everyone]
        print("step", t, "forms (plain, after_steps, watched):", forms)
        if n == 1 << 20 and not history:
            assert forms == [capi.MP_K1_FORM_TWO_TILES, capi.MP_K1_FORM_TWO_TILES, capi.MP_K1_FORM_TILE]
        else:
            assert forms[0] == forms[1] == forms[2]
        assert Q.same_bits(watched.quantiles(QS), after_steps.quantiles(QS))
    for pf in (after_steps, watched):
        assert np.array_equal(plain.states(), pf.states())
        assert np.array_equal(plain.parents, pf.parents)
        assert np.array_equal(plain.log_weights, pf.log_weights)
        assert plain.effective_sample_size(fresh=True) == pf.effective_sample_size(fresh=True)
        assert plain.log_marginal_likelihood_estimate() == pf.log_marginal_likelihood_estimate()
        assert Q.same_bits(plain.quantiles(QS), pf.quantiles(QS))


def test_statuses():
    """Three outcomes have no test because no handle built from the compiled models reaches them: MP_ERR_UNSUPPORTED for a dim_state
    outside {1, 2, 4, 16} (no model has such a width); MP_ERR_STATE for a log that does not hold one state per step (the path call;
    every step of a history filter records one); every output NaN with MP_OK for a NaN max (no model produces a NaN log-weight; the
    restatement's side of it is in tests/test_quantiles_ref.py)."""
    import modppl_amd
    from modppl_amd import capi
    from modppl_amd.distributed import HipShardEngine

    model, ys = modppl_amd.lgssm_model(*O.LGSSM_PARAMS), O.lgssm_observations(2).reshape(2, 1)
    L = capi.load()
    dp = C.POINTER(C.c_double)
    out = np.full(32, np.nan)
    q = lambda *v: np.array(v, dtype=np.float64).ctypes.data_as(dp)

    early = modppl_amd.ParticleSystem(model, 64, 1)
    assert L.mp_pf_quantiles(early._h, q(0.5), 1, out.ctypes.data_as(dp)) == capi.MP_ERR_STATE

    eng = HipShardEngine(model, 2048, 4096, 0, 21)      # the first of two shards
    eng.init_step(None, ys[:1])
    assert L.mp_pf_quantiles(eng._h, q(0.5), 1, out.ctypes.data_as(dp)) == capi.MP_ERR_UNSUPPORTED

    pf = modppl_amd.ParticleSystem(model, 3000, 5)
    pf.init_step(None, ys[:1])
    o = out.ctypes.data_as(dp)
    assert L.mp_pf_quantiles(None, q(0.5), 1, o) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_quantiles(pf._h, None, 1, o) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_quantiles(pf._h, q(0.5), 1, None) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_quantiles(pf._h, q(0.5), 0, o) == capi.MP_ERR_INVALID_ARG
    assert L.mp_pf_quantiles(pf._h, q(*([0.5] * 17)), 17, o) == capi.MP_ERR_INVALID_ARG
    for bad in (np.nan, -1e-300, 1.0000000000000002, np.inf):
        assert L.mp_pf_quantiles(pf._h, q(0.5, bad), 2, o) == capi.MP_ERR_INVALID_ARG
    assert np.isnan(out).all()                          # nothing was written
    assert L.mp_pf_quantiles(pf._h, q(-0.0, 5e-324, 1.0), 3, o) == capi.MP_OK      # -0.0 is 0; the smallest subnormal is a level
    assert Q.same_bits(out[:3], Q.pf_quantiles(pf.states(), pf.log_weights, [0.0, 5e-324, 1.0]).ravel())
    with pytest.raises(capi.ModpplError) as err:
        pf.quantiles([])
    assert err.value.code == capi.MP_ERR_INVALID_ARG
