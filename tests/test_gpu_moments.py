"""GPU: ParticleSystem.moments() (mp_pf_moments) — the weighted mean and covariance of the cloud reduced on the device.

Every check goes through the C ABI; truth is computed from `pf.states()` and `pf.log_weights` read back in the same state:
  * bit parity with the numpy restatement of the definition (tests/moments_ref.py), equal as numbers;
  * the outside truth (long-double exponentials, math.fsum) within the bounds derived from the definition's operations;
  * invisibility: a filter that calls moments() everywhere computes the same bits as one that never does;
  * repeatability, cov=False, a world-of-one sharded handle, the unsupported and degenerate statuses.
Without mp_pf_moments every test here fails at the missing symbol."""
import functools

import numpy as np
import pytest

from tests import moments_ref as R
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 2047, 2048, 2049, (1 << 16) + 63]
MODELS = ["lgssm1", "spiral", "bearings", "band16"]
STAGES = ["init", "step", "resampled"]
T = 3


@functools.lru_cache(maxsize=None)
def problem(name):
    """-> (model, args0, obs [T, dim_obs])"""
    import modppl_amd
    from tests.test_gpu_pf_models import BEAR, bearings_obs, spiral_obs

    if name == "lgssm1":    # d = 1: after a step the states sit in the row table (x_in_rows)
        return modppl_amd.lgssm_model(*O.LGSSM_PARAMS), None, O.lgssm_observations(T).reshape(T, 1)
    if name == "spiral":
        return modppl_amd.spiral_model(), [0.0, 0.0], spiral_obs(T)
    if name == "bearings":
        return modppl_amd.bearings_model(*BEAR), None, bearings_obs(T).reshape(T, 1)
    return modppl_amd.lgssm_band_model(16), None, np.random.default_rng(3).normal(0, 1.2, size=(T, 16))


def check_against_readback(pf, what=""):
    """moments() against the restatement and the outside truth, both on what the handle hands back in the same state"""
    mean, cov = pf.moments()
    x, lw = pf.states(), pf.log_weights
    rm, rc = R.pf_moments(x, lw)
    assert R.same_numbers(mean, rm), (what, mean, rm)
    assert R.same_numbers(cov, rc), (what, cov, rc)
    worst = R.check_bounds(x, lw, mean, cov)
    print(f"{what}: n = {len(lw)}, error / bound: mean {worst[0]:.3f}, cov {worst[1]:.3f}")
    return mean, cov, x, lw


@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", MODELS)
def test_bit_parity_and_outside_truth(name, n, stage):
    import modppl_amd

    model, args0, obs = problem(name)
    pf = modppl_amd.ParticleSystem(model, n, 20260301)
    pf.init_step(args0, obs[:1])
    if stage != "init":
        pf.step(obs[1:2])          # no resample in between: the log-weights of two steps add up
    if stage == "resampled":
        pf.resample()
    mean, cov, x, lw = check_against_readback(pf, f"{name} {stage}")
    if stage == "resampled":
        assert not lw.any()        # a_i = 1 for every i
        assert R.same_numbers(mean, [R.tree_sum(x[:, j]) / n for j in range(x.shape[1])])
    elif n > 2:
        assert np.unique(lw).size > 1


@pytest.mark.parametrize("n", [2049, (1 << 16) + 63])
def test_minus_inf_weights_contribute_nothing(n):
    """the HMM with impossible emissions of test_gpu_normalisation_exact.py::test_minus_inf_mixture_never_drawn"""
    import modppl_amd

    prior, emis, trans = [0.5, 0.5], [[1.0, 0.2], [0.0, 0.8]], [[0.9, 0.3], [0.1, 0.7]]
    data = np.array([[1.0], [0.0], [1.0]])
    pf = modppl_amd.ParticleSystem(modppl_amd.hmm_model(prior, emis, trans), n, 7)
    pf.init_step(None, data[:1])
    mean, cov, x, lw = check_against_readback(pf, "hmm init")
    dead = lw == -np.inf
    assert dead.any() and not dead.all()
    assert mean[0] == 1.0 and cov[0, 0] == 0.0      # state 0 never emits 1: every live particle sits in state 1
    pf.step(data[1:2])
    check_against_readback(pf, "hmm step")


def test_all_minus_inf_is_degenerate():
    import modppl_amd
    from modppl_amd import capi

    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), 5000, 3)
    pf.init_step(None, [0.3])
    pf.step([np.inf])              # logpdf = -inf for every particle
    assert (pf.log_weights == -np.inf).all()
    with pytest.raises(capi.ModpplError) as err:
        pf.moments()
    assert err.value.code == capi.MP_ERR_DEGENERATE


@pytest.mark.parametrize("n", [1 << 20, (1 << 20) + 4096 + 5])
def test_invisible_to_the_filter(n):
    """Same-seed filters, 6 steps, at the sizes where a step that makes the resample's draws runs as the two-tile kernel
    (tests/test_gpu_model_laws.py).  `watched` calls moments() after every step and after every resample: synchronous resamples and
    asynchronous ones, so the call lands on deferred draws nobody has made; it makes them, and the step behind it finds none pending and
    runs one workgroup per tile with the states left in the row table (x_in_rows) — asserted at every step.  `after_steps` calls it
    after every step only: its steps make the draws themselves and run as the two-tile kernel, as the plain filter's do (asserted at
    every step), and behind an asynchronous resample the call lands on that kernel's pending lazy launch.  So the two watched filters
    take different kernels through the same six steps; final states, parents, log-weights, log-ML and ESS are bit-equal to the plain
    filter's, and every intermediate moments() equals the restatement on a further same-seed filter's read-back."""
    import modppl_amd
    from modppl_amd import capi

    ys = O.lgssm_observations(7).reshape(7, 1)
    mk = lambda: modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, 20260302)
    plain, watched, after_steps, third = mk(), mk(), mk(), mk()
    everyone = (plain, watched, after_steps, third)

    def look(*pfs):
        want = R.pf_moments(third.states(), third.log_weights)
        for pf in pfs:
            got = pf.moments()
            assert R.same_numbers(got[0], want[0]) and R.same_numbers(got[1], want[1]), (got, want)

    for pf in everyone:
        pf.init_step(None, ys[:1])
    look(watched, after_steps)
    for t in range(1, 7):
        sync = t % 2 == 1
        Ls = [pf.resample(sync=sync) for pf in everyone]
        assert Ls[0] == Ls[1] == Ls[2] == Ls[3]
        look(watched)
        for pf in everyone:
            pf.step(ys[t:t + 1])
        forms = [pf.last_propagate_form() for pf in (plain, after_steps, watched)]
        print("step", t, "forms (plain, after_steps, watched):", forms)
        # a step that finds the resample's draws pending makes them itself, two tiles per workgroup; the moments() between the resample
        # and the step has made them already, and that step runs one workgroup per tile — the bits must not care
        assert forms == [capi.MP_K1_FORM_TWO_TILES, capi.MP_K1_FORM_TWO_TILES, capi.MP_K1_FORM_TILE]
        look(watched, after_steps)
    for pf in (watched, after_steps):
        assert np.array_equal(plain.states(), pf.states())
        assert np.array_equal(plain.parents, pf.parents)
        assert np.array_equal(plain.log_weights, pf.log_weights)
        assert plain.log_marginal_likelihood_estimate() == pf.log_marginal_likelihood_estimate()
        assert plain.effective_sample_size(fresh=True) == pf.effective_sample_size(fresh=True)


def test_repeatable_and_mean_only():
    import modppl_amd

    model, args0, obs = problem("bearings")
    pf = modppl_amd.ParticleSystem(model, 3 * 2048 + 17, 5)
    pf.init_step(args0, obs[:1])
    a, b = pf.moments(), pf.moments()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    m, c = pf.moments(cov=False)
    assert c is None and np.array_equal(m, a[0])


def test_world_of_one_sharded_handle_and_a_shard_of_a_larger_world():
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
    a, b = one.moments(), sh.moments()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    want = R.pf_moments(sh.states(), sh.log_weights)
    assert R.same_numbers(b[0], want[0]) and R.same_numbers(b[1], want[1])

    eng = HipShardEngine(model, 2048, 4096, 0, seed)      # the first of two shards
    eng.init_step(None, ys[:1].reshape(1, 1))
    with pytest.raises(capi.ModpplError) as err:
        eng.moments()
    assert err.value.code == capi.MP_ERR_UNSUPPORTED
