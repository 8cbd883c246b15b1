"""The device against the independent statement of every filter model's law (tests/model_laws.py): the checks of
tests/test_model_laws.py on `ParticleSystem`, at sizes that select each form of the propagate kernel.

2^18 + 63: one tile per workgroup with a ragged last tile.  2^20 and 2^20 + 4096 + 5: the two-tile kernel for the models
that take it (one state coordinate: lgssm1, hmm), asserted through last_propagate_form(); the dense model runs the
matrix-core kernel at every size.  `resample(sync=False)` before the checked step makes the resample's draws run inside
the propagate kernel (the fused path); the synchronous resample is the other parametrisation.  At 2^20 particles the
Kolmogorov-Smirnov tests see a scale error of about 0.3 %.

Seeds were written down before the first run.
"""
import functools

import pytest

from tests import model_laws as ML

pytestmark = pytest.mark.gpu

N_RAGGED = (1 << 18) + 63
N_TWO = 1 << 20
N_TWO_RAGGED = (1 << 20) + 4096 + 5
SEED, OTHER_SEED, OBS_SEED = 20260201, 20260202, 405
TWO_TILE_LAWS = ("lgssm1", "hmm")     # DIM_STATE == 1: the models the two-tile kernel is built for


@functools.lru_cache(maxsize=None)
def law(name):
    return ML.make_law(name)


def expected_form(name, n, sync):
    from modppl_amd import capi

    if name.startswith("dense"):
        return capi.MP_K1_FORM_DENSE16
    if name in TWO_TILE_LAWS and n >= N_TWO and not sync:   # a drawing launch of at least two tiles per compute unit
        return capi.MP_K1_FORM_TWO_TILES
    return capi.MP_K1_FORM_TILE


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_weights_and_structure_ragged_tile(name):
    ML.check_weights(ML.DeviceEngine(law(name), N_RAGGED, SEED), law(name), OBS_SEED, sync=True)
    r = ML.check_structure(ML.DeviceEngine(law(name), N_RAGGED, SEED + 1), law(name), OBS_SEED)
    assert r.form1 == expected_form(name, N_RAGGED, True)


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_weights_fused_draws(name):
    ML.check_weights(ML.DeviceEngine(law(name), N_TWO, SEED + 2), law(name), OBS_SEED, sync=False)


CASES = [(name, N_TWO, False) for name in ML.LAW_NAMES] + [(name, N_RAGGED, True) for name in ML.LAW_NAMES] \
    + [(name, N_TWO_RAGGED, False) for name in TWO_TILE_LAWS]     # the two-tile kernel's ragged last pair of tiles


@pytest.mark.parametrize("name,n,sync", CASES)
def test_noise_law_and_keying(name, n, sync):
    lw = law(name)
    r = ML.two_steps(ML.DeviceEngine(lw, n, SEED + 3), lw, OBS_SEED, sync=sync)
    assert r.form1 == expected_form(name, n, sync) and r.form2 == r.form1
    ML.check_init_law(lw, r.x0)
    ML.check_noise_law(lw, r.x1, r.x0[r.par1], None if lw.categorical else r.r1)
    ML.check_noise_law(lw, r.x2, r.x1[r.par2], None if lw.categorical else r.r2)
    other = ML.two_steps(ML.DeviceEngine(lw, n, OTHER_SEED), lw, OBS_SEED, sync=sync)
    ML.check_independence(lw, r, other)


@pytest.mark.parametrize("name", ["spiral", "bearings"])
def test_one_step_evidence_against_quadrature(name):
    ML.check_one_step_evidence(ML.DeviceEngine(law(name), N_RAGGED, SEED + 4), law(name))
