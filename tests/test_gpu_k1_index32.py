"""GPU: the two-tile kernel (k_propagate_mt, mp_pf_k1mt.h) keeps every row index, tile base, clamp and byte offset in 32 bits off
scalar base pointers.  Nothing it computes may move: forced with MP_K1_MT_GRID=1 it is held, bit for bit, against the tile kernel
(k_propagate, MP_K1_MT=0, which keeps the 64-bit helpers) and against the canonical checker — parents, states, log-weights, fresh ESS
and log-ML — at the sizes where a 32-bit clamp or offset can go wrong: exactly two tiles, a last tile of one row (`last` equals the start
row, no successor exists; the workgroup without a tile B gathers A twice), an odd count of whole tiles, and last tiles one row long or
one row short.  The upper boundary of the form (1024 tiles) is tests/test_gpu_deferred.py::test_timed_path_at_the_timed_size."""
import numpy as np
import pytest

from modppl_amd import capi
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu

TILE = 2048
SIZES = [2 * TILE, 2 * TILE + 1, 5 * TILE, 6 * TILE + 1, 3 * TILE + 2047]
T = 6
SEED = 977
MP_WALK_LINEAR = 12     # mp_pf_kernels.h: a walk still going after this many rows finishes by bisection
LN_2_POW_52 = 36.04365338911715   # a row whose log-weight lies further than this below its tile's maximum quantises to a weight of zero
                                  # (51 fractional bits, rounded to nearest: exp(d) * 2^51 < 1/2)


def _system(monkeypatch, n, **env):
    import modppl_amd

    for k, v in env.items():
        monkeypatch.setenv(k, v)
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, SEED)
    for k in env:
        monkeypatch.delenv(k)
    return pf


def _filters(monkeypatch, n, **mt_env):
    """(two-tile kernel, tile kernel, checker)"""
    mt = _system(monkeypatch, n, MP_K1_MT_GRID="1", **mt_env)
    one = _system(monkeypatch, n, MP_K1_MT="0")
    ref = O.OraclePF(1, 1, 1, O.LGSSM_PARAMS, n, SEED, O.VARIANT_CANONICAL | O.VARIANT_SOA)
    return mt, one, ref


def _same_everywhere(mt, one, ref, what, parents=True):
    for pf in (mt, one):
        if parents:
            assert np.array_equal(pf.parents, ref.parents()), what
        assert np.array_equal(pf.states(), ref.state()), what
        assert np.array_equal(pf.log_weights, ref.log_weights()), what
        assert pf.effective_sample_size(fresh=True) == ref.effective_sample_size(1), what
        assert pf.log_marginal_likelihood_estimate() == ref.log_marginal_likelihood_estimate(), what
    assert np.array_equal(mt.states(), one.states()), what
    assert np.array_equal(mt.log_weights, one.log_weights), what
    if parents:
        assert np.array_equal(mt.parents, one.parents), what


def _run(mt, one, ref, obs, resample_before, look=None):
    """init_step, then for t = 1 ..: (resample when resample_before[t]), step; every value of both kernels against the checker after
    every step.  look(t, ref): the test's own look at the checker's state after step t."""
    for pf in (mt, one):
        pf.init_step(None, obs[:1])
    ref.init_step(obs[:1])
    for t in range(1, len(obs)):
        if resample_before[t]:
            for pf in (mt, one):
                pf.resample(sync=False)
            ref.resample()
        for pf in (mt, one):
            pf.step(obs[t:t + 1])
        ref.step(obs[t:t + 1])
        if resample_before[t]:
            assert mt.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES
            assert one.last_propagate_form() == capi.MP_K1_FORM_TILE
        _same_everywhere(mt, one, ref, f"n={mt.num_particles} t={t}", parents=resample_before[t])
        if look is not None:
            look(t, ref)


def _zero_weight_runs(lw):
    """(the longest run of rows of zero fixed-point weight inside one tile, the longest such run that has a row of non-zero weight on
    either side of it IN ITS TILE — what a walk that starts on the row in front of the run has to cross)"""
    anywhere, between = 0, 0
    for b in range(0, lw.size, TILE):
        d = lw[b:b + TILE] - lw[b:b + TILE].max()
        live = np.flatnonzero(d > -LN_2_POW_52 + 1.0)            # (one unit clear of the rounding boundary on either side)
        dead = d < -LN_2_POW_52 - 1.0
        edges = np.concatenate([[-1], live, [d.size]])
        for i, j in zip(edges[:-1], edges[1:]):
            if j - i - 1 > 0 and np.all(dead[i + 1:j]):
                anywhere = max(anywhere, int(j - i - 1))
                if i >= 0 and j < d.size:
                    between = max(between, int(j - i - 1))
    return anywhere, between


@pytest.mark.parametrize("n", SIZES)
def test_a_resample_before_every_step(monkeypatch, n, diag):
    obs = O.lgssm_observations(T).reshape(T, 1)
    _run(*_filters(monkeypatch, n), obs, [True] * T)


# (sigma_y between the far observation and the cloud, a step without a resample behind it, MP_WALK_BISECT)
WALK_CASES = [pytest.param(1e5, True, None, id="collapsed"), pytest.param(20.0, False, None, id="gapped"), pytest.param(20.0, False, "0", id="gapped_plain_walk")]


@pytest.mark.parametrize("sigmas, second_step, bisect", WALK_CASES)
@pytest.mark.parametrize("n", SIZES)
def test_long_walks_and_bisection_up_to_the_last_row(monkeypatch, n, sigmas, second_step, bisect, diag):
    """`collapsed`: an observation 10^5 sigma_y away, then a second step WITHOUT a resample (the construction of
    tests/test_gpu_lean_ops.py's zero-weight test): every tile is runs of zero-weight rows around the one or two rows that carry it, most
    tiles weigh nothing at level 1, and the next resample's draws all end on the same few rows — clamps at `last`, tiles of one live row.
    `gapped`: the observation 20 sigma_y away, a resample at every step: a few dozen rows of a tile keep a non-zero weight, with runs
    of zero-weight rows BETWEEN them that are longer than the linear walk, so a draw that starts on a light row walks past the rows
    asked for in advance, through the row-at-a-time walk and the bisection over (p, last], to the next live row.  The bisecting
    instantiation of the kernel (the default for this model) and the plain walk (MP_WALK_BISECT=0)."""
    obs = O.lgssm_observations(T).reshape(T, 1).copy()
    far = 2
    obs[far, 0] += sigmas * O.LGSSM_PARAMS[4]
    plan = [True] * T
    drawn_from = far          # the step whose weights the next resample draws from
    if second_step:
        plan[far + 1] = False
        drawn_from = far + 1
    seen = {}

    def look(t, ref):
        if t == drawn_from:
            seen["lw"] = ref.log_weights().copy()

    env = {} if bisect is None else {"MP_WALK_BISECT": bisect}
    _run(*_filters(monkeypatch, n, **env), obs, plan, look)
    anywhere, between = _zero_weight_runs(seen["lw"])
    assert anywhere > MP_WALK_LINEAR, "no tile with a run of zero-weight rows longer than the linear walk"
    if not second_step:
        assert between > MP_WALK_LINEAR, "no run of zero-weight rows longer than the linear walk between two live rows of a tile"


@pytest.mark.parametrize("n", SIZES)
def test_the_replay_launch_stores_what_the_step_left_out(monkeypatch, n, diag):
    """After an asynchronous resample the step's launch stores neither log-weights nor parents; reading them launches the kernel again
    with MP_MT_REPLAY (mt_store_replay).  Against the checker, and against a filter whose every launch stores them (MP_K1_LAZY=0:
    mt_store_tile's own stores of the two arrays)."""
    obs = O.lgssm_observations(T).reshape(T, 1)
    lazy = _system(monkeypatch, n, MP_K1_MT_GRID="1")
    eager = _system(monkeypatch, n, MP_K1_MT_GRID="1", MP_K1_LAZY="0")
    ref = O.OraclePF(1, 1, 1, O.LGSSM_PARAMS, n, SEED, O.VARIANT_CANONICAL | O.VARIANT_SOA)
    for pf in (lazy, eager):
        pf.init_step(None, obs[:1])
    ref.init_step(obs[:1])
    for t in range(1, T):
        for pf in (lazy, eager):
            pf.resample(sync=False)
            pf.step(obs[t:t + 1])
            assert pf.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES
        ref.resample()
        ref.step(obs[t:t + 1])
        if t % 2:   # (the other rounds: nobody reads them, the next resample follows at once)
            for pf in (lazy, eager):
                assert np.array_equal(pf.log_weights, ref.log_weights()), (n, t)
                assert np.array_equal(pf.parents, ref.parents()), (n, t)
    for pf in (lazy, eager):
        assert np.array_equal(pf.parents, ref.parents())
        assert np.array_equal(pf.log_weights, ref.log_weights())
        assert np.array_equal(pf.states(), ref.state())
        assert pf.effective_sample_size(fresh=True) == ref.effective_sample_size(1)
        assert pf.log_marginal_likelihood_estimate() == ref.log_marginal_likelihood_estimate()
