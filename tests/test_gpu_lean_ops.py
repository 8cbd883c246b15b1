"""GPU: the lean forms of the shared helpers leave every bit where it was — polynomial constants as scalar operands of the fma
(mp_fma_c and friends, mp_math.h), the carry-chained DPP scan, the uncanonicalised maxima (mp_max_q) and the 16-lane cross-wave
combines (xwave_max / xwave_prefix, mp_pf_kernels.h).  The two-tile kernel (k_propagate_mt, MP_K1_MT_GRID=1) and the tile kernel
(k_propagate, MP_K1_MT=0) against the canonical checker and against each other at ragged sizes, with log-weights whose spread
inside a tile runs from 0 to far below the exponential's underflow, and with waves and tiles whose whole weight quantises to
zero beside healthy ones; mp_exp / mp_log on the device against the host at every point where the code takes another arm."""
import ctypes as C

import numpy as np
import pytest

from modppl_amd import capi
from tests import oracle_lib as O

pytestmark = pytest.mark.gpu
DP = C.POINTER(C.c_double)

K1_SIZES = [4097, 2048 * 5, 2048 * 6 + 1]   # two-tile kernel: an odd tile count, whole tiles, a last tile of one row
TILE_SIZES = [1, 63, 65, 2047, 2049]        # tile kernel: less than a wave, a wave and one, a tile less one, a tile and one
T = 6
SEED = 4242
EXP_UNDERFLOW = -745.1332191019412          # mp_exp returns 0 below this
EXP_SUBNORMAL = -708.3964185322641          # ln 2^-1022: results below this argument are subnormal (the k < -1022 arm)


def _filters(monkeypatch, n):
    """(two-tile kernel where the job has two tiles, tile kernel, checker), all after init_step on the same data"""
    import modppl_amd

    monkeypatch.setenv("MP_K1_MT_GRID", "1")
    mt = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, SEED)
    monkeypatch.delenv("MP_K1_MT_GRID")
    monkeypatch.setenv("MP_K1_MT", "0")
    one = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(*O.LGSSM_PARAMS), n, SEED)
    monkeypatch.delenv("MP_K1_MT")
    ref = O.OraclePF(1, 1, 1, O.LGSSM_PARAMS, n, SEED, O.VARIANT_CANONICAL | O.VARIANT_SOA)
    return mt, one, ref


def _same_everywhere(mt, one, ref, what, parents=True):
    if parents:
        want = ref.parents()
        assert np.array_equal(mt.parents, want), what
        assert np.array_equal(one.parents, want), what
    for pf in (mt, one):
        assert np.array_equal(pf.states(), ref.state()), what
        assert np.array_equal(pf.log_weights, ref.log_weights()), what
        assert pf.effective_sample_size(fresh=True) == ref.effective_sample_size(1), what
        assert pf.log_marginal_likelihood_estimate() == ref.log_marginal_likelihood_estimate(), what
    assert np.array_equal(mt.states(), one.states()), what
    assert np.array_equal(mt.log_weights, one.log_weights), what
    assert np.array_equal(mt.parents, one.parents), what


def _run(monkeypatch, n, obs, resample_before, look=None):
    """init_step, then for t = 1 ..: (resample when resample_before[t]), step; every value of both kernels against the checker
    after every step.  look(t, ref): the test's own look at the checker's state after step t."""
    mt, one, ref = _filters(monkeypatch, n)
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
        if resample_before[t] and n in K1_SIZES:
            assert mt.last_propagate_form() == capi.MP_K1_FORM_TWO_TILES
        _same_everywhere(mt, one, ref, f"n={n} t={t}", parents=resample_before[t])
        if look is not None:
            look(t, ref)


def _below_tile_max(lw):
    """lw - (maximum of its tile of 2048 rows): the argument of the level-0 exponential"""
    d = np.empty_like(lw)
    for b in range(0, lw.size, 2048):
        d[b:b + 2048] = lw[b:b + 2048] - lw[b:b + 2048].max()
    return d


@pytest.mark.parametrize("n", K1_SIZES + TILE_SIZES)
def test_ragged_sizes(monkeypatch, n, diag):
    obs = O.lgssm_observations(T).reshape(T, 1)
    _run(monkeypatch, n, obs, [True] * T)


@pytest.mark.parametrize("n", K1_SIZES + TILE_SIZES)
def test_wide_exponent_spread_inside_a_tile(monkeypatch, n, diag):
    """One observation 400 sigma_y from the cloud: lw = -(400 - x)^2 / 2 moves by 400 per unit of x, so inside one tile lw - max
    runs from 0 to below -745 — the normal arm of mp_exp_nonpos, its k < -1022 arm (subnormal results) and the exact zero."""
    obs = O.lgssm_observations(T).reshape(T, 1).copy()
    far = 3
    obs[far, 0] += 400.0 * O.LGSSM_PARAMS[4]
    seen = {}

    def look(t, ref):
        if t == far:
            seen["d"] = _below_tile_max(ref.log_weights())

    _run(monkeypatch, n, obs, [True] * T, look)
    d = seen["d"]
    if n >= 2047:   # (a handful of rows cannot be promised to land in a window 37 wide; a tile's worth does)
        assert np.any((d < EXP_SUBNORMAL) & (d > EXP_UNDERFLOW)), "no row in the subnormal arm"
        assert np.any(d < EXP_UNDERFLOW) and np.any((d < 0) & (d > -700)), "no row beyond the underflow / in the normal arm"


@pytest.mark.parametrize("n", K1_SIZES + TILE_SIZES)
def test_waves_and_tiles_of_zero_weight_beside_healthy_ones(monkeypatch, n, diag):
    """An observation 10^5 sigma_y away, then a second step WITHOUT a resample in between: lw moves by 10^5 per unit of x, so in
    every tile only the rows within 0.007 of its best one keep a non-zero fixed-point weight — most waves hand a zero total to the
    cross-wave prefix — and the tiles' maxima lie thousands apart, so that at level 1 (the table the next resample is drawn
    from) most tiles weigh exactly zero beside the few that carry everything.  (A log-weight of this model is -inf only where
    (y - x)^2 overflows, which no particle's x decides: a tile whose maximum is -inf has every other tile dead with it, and that
    resample is refused — tests/test_gpu_deferred.py has it.  Zero WEIGHT beside healthy rows is what the combines can meet with
    this model; a tile maximum of -inf beside finite ones needs a model whose log-weight can be -inf particle by particle, and is
    not covered here.)"""
    obs = O.lgssm_observations(T).reshape(T, 1).copy()
    far = 2
    obs[far, 0] += 1e5 * O.LGSSM_PARAMS[4]
    plan = [True] * T
    plan[far + 1] = False
    seen = {}

    def look(t, ref):
        if t in (far, far + 1):
            seen[t] = ref.log_weights().copy()

    _run(monkeypatch, n, obs, plan, look)
    for t in (far, far + 1):
        lw = seen[t]
        d = _below_tile_max(lw)
        if n >= 2047:
            dead = [np.all(d[w:w + 128] < EXP_UNDERFLOW) for w in range(0, n, 128)]
            assert any(dead) and not all(dead), "no wave of zero weight beside a healthy one"
        if n >= 4097:
            tm = np.array([lw[b:b + 2048].max() for b in range(0, n, 2048)])
            assert np.any(tm - tm.max() < -800.0), "no tile of zero weight at level 1"


def _probe(hiplib, op, a):
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = np.empty_like(a)
    capi.check(hiplib.mp_probe_math(op, a.ctypes.data_as(DP), None, None, a.size, out.ctypes.data_as(DP), 0))
    return out


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def _around(x, ulps=2):
    """x and its neighbours up to `ulps` ulps on either side"""
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    out = [x]
    lo, hi = x, x
    with np.errstate(over="ignore"):   # (the neighbour above the largest double is inf: an argument like any other)
        for _ in range(ulps):
            lo, hi = np.nextafter(lo, -np.inf), np.nextafter(hi, np.inf)
            out += [lo, hi]
    return np.concatenate(out)


def test_exp_log_bitwise_where_the_code_takes_another_arm(hiplib, oracle):
    """device == host, bit for bit, on what tests/test_gpu_math.py does not draw: the arguments where mp_exp's k changes
    ((k + 1/2) ln 2 for every k it can take), the neighbours of its underflow, subnormal and overflow thresholds and of 0,
    a sweep of the subnormal results; for mp_log the neighbours of 1 and of every power of two (k changes), of sqrt 2 times
    those (the reduced argument wraps), and subnormal arguments."""
    rng = np.random.default_rng(5)
    k = np.arange(-1076, 1026, dtype=np.float64)
    ln2 = 0.6931471805599453
    xe = np.concatenate([
        _around((k + 0.5) * ln2, 3), _around(k * ln2, 1),
        _around([EXP_UNDERFLOW, -745.13, EXP_SUBNORMAL, -708.4, 709.782712893384, 0.0, -0.0, 5e-324, -5e-324, 1.0, -1.0]),
        rng.uniform(EXP_UNDERFLOW, EXP_SUBNORMAL, 1 << 16), np.linspace(EXP_UNDERFLOW - 1, EXP_SUBNORMAL + 1, 1 << 14),
        rng.uniform(-1, 1, 1 << 12) * 2.0 ** rng.integers(-1074, -40, 1 << 12)])
    ref = np.empty_like(xe)
    oracle.oracle_mp_exp(O.dptr(xe), xe.size, O.dptr(ref))
    got = _probe(hiplib, 0, xe)
    assert np.array_equal(_bits(got), _bits(ref))
    sub = (xe < EXP_SUBNORMAL) & (xe > EXP_UNDERFLOW)
    assert np.all(ref[sub] < 2.2250738585072014e-308) and np.count_nonzero(ref[sub] > 0) > (1 << 15)   # the subnormal arm was met

    p2 = 2.0 ** np.arange(-1074, 1024, dtype=np.float64)
    xl = np.concatenate([
        _around(p2, 2), _around(p2[52:] * 1.4142135623730951, 3), _around([1.0, 0.0, 2.2250738585072014e-308, 1.7976931348623157e308]),
        p2[:52] * rng.integers(1, 1 << 20, 52), rng.uniform(0, 1, 1 << 14) * 2.2250738585072014e-308,
        1.0 + rng.uniform(-1, 1, 1 << 14) * 2.0 ** rng.integers(-52, -1, 1 << 14)])
    xl = xl[xl >= 0]
    ref = np.empty_like(xl)
    oracle.oracle_mp_log(O.dptr(xl), xl.size, O.dptr(ref))
    got = _probe(hiplib, 1, xl)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan)
    assert np.array_equal(_bits(got[~nan]), _bits(ref[~nan]))
