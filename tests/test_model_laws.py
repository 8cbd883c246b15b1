"""The CPU checker against an independent statement of every filter model's law (tests/model_laws.py).

Every GPU parity test leans on the checker, and the checker interprets the same functors as the device
(modppl_amd/csrc/mp_models.h): what both would get wrong together only shows against a second statement of the model.
Here the checker's canonical SoA engine (threads=4) is held to it: the weights are the stated density (a), the exact
structure of a step (b), the law of the noise (c), the keying of the draws (d) and, for the two models without an exact
filter, the one-step evidence (e).  spiral, bearings and band D = 2 also run (a) and (b) on the structure-faithful dynamic
engine.  The checker restates lgssm1, spiral, hmm, bearings and the banded model by hand and runs the product's functors of
four of them through its adapter under test-only kinds: those run every check too ("functor" below), so that the model
source the device compiles is held to the law without a GPU.  tests/test_gpu_model_laws.py runs the same checks on the device.

Seeds were written down before the first run.
"""
import functools

import pytest

from tests import model_laws as ML

N_STAT = 1 << 18       # (c), (d), (e)
N_STAT_SLOW = 1 << 14  # dense with a singular Q: the checker derives the eigen transform per call, 180 us per particle and step; the device test runs 2^20
N_SMALL = 6000 + 37    # (a), (b): a few tiles and a ragged one
N_DYN = 3000           # the dynamic engine
SEED, OTHER_SEED, OBS_SEED = 20260101, 20260102, 404


@functools.lru_cache(maxsize=None)
def law(name):
    return ML.make_law(name)


@functools.lru_cache(maxsize=None)
def stat_run(name, seed, functor=False):
    lw = law(name)
    return ML.two_steps(ML.OracleEngine(lw, N_STAT_SLOW if name == "dense16_singular" else N_STAT, seed, functor=functor), lw, OBS_SEED)


FUNCTOR = list(ML.OracleEngine.FUNCTOR_LAWS)


@pytest.mark.parametrize("name", FUNCTOR)
def test_functor_weights_and_structure(name):
    ML.check_weights(ML.OracleEngine(law(name), N_SMALL, SEED + 5, functor=True), law(name), OBS_SEED)
    ML.check_structure(ML.OracleEngine(law(name), N_SMALL, SEED + 6, functor=True), law(name), OBS_SEED)
    ML.check_weights(ML.OracleEngine(law(name), N_DYN, SEED + 7, soa=False, functor=True), law(name), OBS_SEED)


@pytest.mark.parametrize("name", FUNCTOR)
def test_functor_noise_law_and_keying(name):
    r = stat_run(name, SEED + 8, True)
    ML.check_init_law(law(name), r.x0)
    ML.check_noise_law(law(name), r.x1, r.x0[r.par1], r.r1)
    ML.check_noise_law(law(name), r.x2, r.x1[r.par2], r.r2)
    ML.check_independence(law(name), r, stat_run(name, OTHER_SEED, True))


@pytest.mark.parametrize("name", ["spiral", "bearings"])
def test_functor_one_step_evidence_against_quadrature(name):
    ML.check_one_step_evidence(ML.OracleEngine(law(name), N_STAT, SEED + 9, functor=True), law(name))


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_weights_are_the_stated_density(name):
    ML.check_weights(ML.OracleEngine(law(name), N_SMALL, SEED), law(name), OBS_SEED)


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_exact_structure_of_a_step(name):
    ML.check_structure(ML.OracleEngine(law(name), N_SMALL, SEED + 1), law(name), OBS_SEED)


@pytest.mark.parametrize("name", ["spiral", "bearings", "band2"])
def test_dynamic_engine_weights_and_structure(name):
    ML.check_weights(ML.OracleEngine(law(name), N_DYN, SEED + 2, soa=False), law(name), OBS_SEED)
    ML.check_structure(ML.OracleEngine(law(name), N_DYN, SEED + 3, soa=False), law(name), OBS_SEED)


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_initial_draw_has_the_stated_law(name):
    ML.check_init_law(law(name), stat_run(name, SEED).x0)


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_step_noise_has_the_stated_law(name):
    r = stat_run(name, SEED)
    cat = law(name).categorical
    ML.check_noise_law(law(name), r.x1, r.x0[r.par1], None if cat else r.r1)
    ML.check_noise_law(law(name), r.x2, r.x1[r.par2], None if cat else r.r2)


@pytest.mark.parametrize("name", ML.LAW_NAMES)
def test_draws_are_keyed_apart(name):
    ML.check_independence(law(name), stat_run(name, SEED), stat_run(name, OTHER_SEED))


@pytest.mark.parametrize("name", ["spiral", "bearings"])
def test_one_step_evidence_against_quadrature(name):
    ML.check_one_step_evidence(ML.OracleEngine(law(name), N_STAT, SEED + 4), law(name))
