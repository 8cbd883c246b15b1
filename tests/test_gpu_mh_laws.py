"""The device against the independent statement of every MH model, proposal and kernel (tests/mh_laws.py): the checks of
tests/test_mh_laws.py on `FunctionChains` (k_fn_generate, k_fn_logjp, k_fn_propose, k_fn_mh, k_fn_regen) for kinds 101, 105 (200
observations), 102, 103, 113, 114 and 120, and the hand-written kernels (k_mh_iterate, k_pointed_iterate) held to the functor form bit for
bit on the same data, so that what is shown for the functor engine carries over to them.

2^18 + 63 chains for the log-joint and the per-chain accept decisions (a ragged last wavefront); 2^20 for stationarity, where the
Kolmogorov-Smirnov bound sees 0.3 % and a marginal's z-test 0.25 % at even odds.  Nothing here reads the reference or a binary built from it.

(c) runs every move type of mh_laws.moves_of -- each proposal, each single-site mask, the joint structure-changing mask, a cycle -- with
k = 1 and 5 moves.  The statement is evaluated in float64 for the statistics of (c) and in long double for (a) and (b).
(d) also runs the hand-written kernels from the prior for twice the number of sweeps the numpy kernel needs, against the exact posterior.

Assertions at level ALPHA = 1e-7 in this file: about 4 000 (mh_laws.check_stationarity returns its count).  Seeds are fixed.
"""
import numpy as np
import pytest

from tests import mh_laws as ML

pytestmark = pytest.mark.gpu

KINDS = (101, 105, 102, 103, 113, 114, 120)
N_AB = (1 << 18) + 63
N_C = 1 << 20
SEED = 20261101


@pytest.mark.parametrize("kind", KINDS)
def test_logjoint_and_accept_decisions(kind):
    law = ML.make_law(kind)
    eng = ML.Engine("device", law, N_AB, SEED)
    ML.check_logjoint(eng, "after creation")
    v, p = law.sample(np.random.default_rng(SEED + 1), N_AB)
    eng.plant(v, p)
    ML.check_logjoint(eng, "after planting")
    tally = ML.Tally()
    props = ML.proposals(law)
    for pr in props:
        ML.check_accept_decisions(eng, pr, tally)
    tally.require(sorted({pr.changes for pr in props if pr.changes is not None}))
    single, joint, cycle = ML.regen_masks(law)
    for m in single + ([joint] if joint else []):
        eng.regen_mh(m, 1)
        ML.check_logjoint(eng, f"after regen_mh {m}")


@pytest.mark.parametrize("k", [1, 5])
@pytest.mark.parametrize("kind", KINDS)
def test_stationarity_from_planted_exact_draws(kind, k):
    law = ML.make_law(kind)
    for j, mv in enumerate(ML.moves_of(law)):
        eng = ML.Engine("device", law, N_C, SEED + 10 + 2 * j + (k == 5))
        ML.check_stationarity(eng, mv, k, SEED + 50 + 2 * j + (k == 5), dt=np.float64)
        eng.g.close()


def test_handwritten_kernels_equal_the_functor_form():
    """(d) HierarchicalChains(functor=False) and PointedChains(functor=False) cannot take a planted state; on the law data sets, over a
    schedule that visits every arm (add_or_remove, both drifts, regen cycles and a joint mask; the three noise matrices), they hold the
    functor form's states bit for bit from the same seed, with equal accept counts: checks (a)-(c) on the functor engine carry over."""
    import modppl_amd

    law = ML.make_law(101)
    n, seed = N_AB, SEED + 3
    h = modppl_amd.HierarchicalChains(law.xs, law.ys, n, seed)
    f = modppl_amd.HierarchicalChains(law.xs, law.ys, n, seed, functor=True)

    def same():
        assert np.array_equal(h.states(), f.states())
        assert np.array_equal(h.logjp(), f.logjp())
    same()
    for sweep in range(4):
        assert h.mh_add_or_remove(1) == f.mh_add_or_remove(1); same()
        assert h.mh(0.1, 3) == f.mh(0.1, 3); same()
        assert h.mh(0.02, 2) == f.mh(0.02, 2); same()
        assert h.regen_mh([1, 2, 3], 3, cycle=True) == f.regen_mh([1, 2, 3], 3, cycle=True); same()
        assert h.regen_mh([2, 3], 1) == f.regen_mh([2, 3], 1); same()
    st = h.states()
    assert 0.05 < (st[:, 0] == 0.0).mean() < 0.95       # both branches are populated
    law = ML.make_law(120)
    h = modppl_amd.PointedChains(law.box, law.cov, law.obs, n, seed)
    f = modppl_amd.PointedChains(law.box, law.cov, law.obs, n, seed, functor=True)
    for sweep in range(3):
        for nz in ML.POINTED_NOISES:
            assert h.mh(nz, 2) == f.mh(nz, 2)
            assert np.array_equal(h.states(), f.states())
            assert np.array_equal(h.logjp(), f.logjp())


# (d) sweeps from the prior.  K = the first number of sweeps (mh_laws.sweep_schedule) after which the numpy kernel, started from 2^16 prior
# draws with seed 20261201, passes every statistic of (c) (mh_laws.numpy_sweeps_to_converge); the device runs 2 K.
K_HIER = 104       # K = 104: the first passing sweep count (9.5 minutes of numpy); the device runs 208, a margin of a factor 2
K_POINTED = 34     # K = 34: the first passing sweep count; the device runs 68


def _run_sweeps(law, mh, n_sweeps):
    for _ in range(n_sweeps):
        for q, reps in ML.sweep_schedule(law):
            mh(q, reps)


def test_handwritten_kernels_converge_from_the_prior():
    import modppl_amd

    law = ML.make_law(101)
    h = modppl_amd.HierarchicalChains(law.xs, law.ys, N_C, SEED + 5)
    _run_sweeps(law, lambda q, reps: h.mh_add_or_remove(reps) if q.kind == 2 else h.mh(q.args[0], reps), 2 * K_HIER)
    st = h.states()
    v, p = law._template((0,), N_C)
    v[:, :4] = st
    p = np.where(st[:, 0] != 0.0, np.uint64(law.configs()[1].present), np.uint64(law.configs()[0].present))
    assert np.all(st[st[:, 0] != 0.0][:, 3] == 0.0)
    ML.check_exact_sample(law, (v, p), "hand-written hierarchical kernels from the prior")
    law = ML.make_law(120)
    g = modppl_amd.PointedChains(law.box, law.cov, law.obs, N_C, SEED + 6)
    _run_sweeps(law, lambda q, reps: g.mh(np.array(q.args).reshape(2, 2), reps), 2 * K_POINTED)
    v, p = law.sample(np.random.default_rng(0), N_C)      # (for the table's shape and the observation slots)
    v[:, 1:3] = g.states()
    ML.check_exact_sample(law, (v, p), "hand-written pointed kernel from the prior")
