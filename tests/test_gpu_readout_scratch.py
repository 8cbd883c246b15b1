"""GPU: one scratch, many callers.  The summary readouts of a filter handle — moments(), path_moments(), forecast(), quantiles(),
path_quantiles() — share ONE grow-only scratch (mp_pf::scratch, csrc/mp_pf_readouts.h; mom_scratch, csrc/mp_moments.h): partials,
results and their pinned host copy.  Nothing of one call may leak into the next, and a buffer that regrows under one caller must
serve the others.

One handle makes all five calls at a short time, steps on, and makes them again in the reverse order at a time and a horizon beyond
the first capacities: in the second round the shared partial buffers and results regrow under whichever caller first needs more
(path_quantiles for the results, forecast for the partials) and the later callers of the round find them grown; the quantile bins
regrow under path_quantiles.  Every answer is compared BIT FOR BIT with the same single call on a fresh same-seed handle that was brought to
the same time and made no other summary call.

The first-capacity rules this relies on (csrc/mp_pf_readouts.h: reserve_steps, quantiles_begin), asserted below so that the test
cannot silently stop covering the regrowth:
  * time steps and horizon steps: max(16, 2 * steps) steps;
  * selectors (levels * dim_state, per time step for the paths): max(256, 2 * selectors)."""
import numpy as np
import pytest

from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

T1, H1 = 3, 2
T2, H2 = 40, 40
QS = [k / 15 for k in range(16)]
SEED = 20261021

CALLS = {
    "moments": lambda pf, H: pf.moments(cov=True),
    "path_moments": lambda pf, H: pf.path_moments(var=True, distinct=True),
    "forecast": lambda pf, H: pf.forecast(H, var=True, obs=True),
    "quantiles": lambda pf, H: (pf.quantiles(QS),),
    "path_quantiles": lambda pf, H: (pf.path_quantiles(QS),),
}


def first_steps(steps):
    return max(16, 2 * steps)


def first_selectors(nsel):
    return max(256, 2 * nsel)


def _case(name):
    """-> (model, obs [T2, dim_obs], n)"""
    import modppl_amd

    if name == "lgssm1":      # two tiles
        return modppl_amd.lgssm_model(*O.LGSSM_PARAMS), O.lgssm_observations(T2).reshape(T2, 1), 4096
    return modppl_amd.lgssm_band_model(16), np.random.default_rng(3).normal(0, 1.2, size=(T2, 16)), 2048     # band16: R = 4 slots per lane


def _advance(pf, obs, t_to):
    """the handle from its time to t_to, resampling before every step"""
    if pf.time == 0:
        pf.init_step(None, obs[:1])
    for t in range(pf.time, t_to):
        pf.resample(sync=False)
        pf.step(obs[t:t + 1])
    assert pf.time == t_to


def _same_bits(got, want):
    assert len(got) == len(want)
    for g, w in zip(got, want):
        assert g.shape == w.shape and g.dtype == w.dtype
        if not np.array_equal(g.view(np.uint64), w.view(np.uint64)):
            return False
    return True


@pytest.mark.parametrize("name", ["lgssm1", "band16"])
def test_one_scratch_many_callers(name):
    import modppl_amd
    from modppl_amd import capi

    model, obs, n = _case(name)
    d = model.dim_state
    assert T2 > first_steps(T1) and H2 > first_steps(H1)
    assert len(QS) * d * T2 > first_selectors(len(QS) * d * T1)

    def fresh():
        return modppl_amd.ParticleSystem(model, n, SEED, flags=capi.MP_PF_RECORD_HISTORY)

    shared = fresh()
    rounds = [(T1, H1, list(CALLS)), (T2, H2, list(CALLS)[::-1])]
    try:
        for T, H, order in rounds:
            _advance(shared, obs, T)
            got = {call: CALLS[call](shared, H) for call in order}
            for call in order:
                alone = fresh()
                try:
                    _advance(alone, obs, T)
                    want = CALLS[call](alone, H)
                finally:
                    alone.close()
                assert _same_bits(got[call], want), (name, T, H, call, got[call], want)
    finally:
        shared.close()
    assert got["path_moments"][0].shape == (T2, d) and got["path_quantiles"][0].shape == (T2, len(QS), d)
    assert got["forecast"][0].shape == (H2, d)
