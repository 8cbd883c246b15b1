"""The MH engines that run without a GPU against the independent statement of every MH model, proposal and kernel (tests/mh_laws.py).

Engines: "tries", the checker's dynamic machinery (OracleFunctionChains), and "host", the PRODUCT's static handlers of
modppl_amd/csrc/mp_genfn.h compiled for the host (HostStaticFunctionChains) -- what the k_fn_* kernels run per lane.  Both compile the
model source the device compiles, so a wrong model body fails here without a GPU; a wrong rule in the handlers of mp_genfn.h or in a density
of mp_dists.h fails on "host".  The LIMIT of "host": its mh and regen loops (oracle/src/mh_functor_adapter.hpp mh_with, regen) are hand
copies of k_fn_mh and k_fn_regen, not mp_mh_fn.h itself, so a mistake in a kernel's own loop -- alpha put together wrongly from the three
weights, a wrong Philox step -- shows on the device only (tests/test_gpu_mh_laws.py, checks (b) and (c)).  The hand-written
checker engines (OracleMH, OraclePointedMH) are held to the statement's log-joint and, bit for bit, to the "tries" engine on the same data.
tests/test_gpu_mh_laws.py runs the same checks on the device.

What guards the statement itself: its input conditions, the mpmath spot check of its log-joints, and its own numpy kernels, which must
leave its own exact posterior draws exact.

Mutations tried against this file (each on a scratch copy; check and engine that failed):
  bernoulli<IS_LINEAR>(0.7) -> 0.6 in mp_hier_fn                          (a) after creation, 101 tries (and host)
  scaled line: ln_sd_small = mp_log(0.4) beside the sd 0.5                 (a) 103 host; NOT tries: the checker's normal takes (mu, sd) and
                                                                           computes the logarithm itself, so a hoisted constant is the product's alone
  nested normal<E>(c + b + d, ..) losing d                                 (a) 113 tries and host
  wide toggle's 0.8 -> 0.7 on one side only                                (b) 114 tries and host
  gc: a dropped site (coeffs/c, d, o2) left out of the discard             (b) 101, 113, 114 host (tries has its own gc: passes)
  regenerate's generate(args, sub) arm: sub-call's running weight kept     (c) 103 host, regen mask {big}: accept count and marginal
  mvnormal2: off-diagonals of cov_inv sign-flipped                         (a) 120 host
  backward proposal score dropped from alpha in k_fn_mh (mp_mh_fn.h)       not catchable here (see LIMIT above): device checks (b), (c)

Assertions at level ALPHA = 1e-7 in this file (mh_laws.check_stationarity returns its count; summed over the runs below): about 9 000;
the chance that a correct engine fails any of them is below 1e-3.  Seeds are fixed.
Wall time of this file: about 12 minutes on one CPU core (50 tests); the statistics of (c) evaluate the statement in float64.
"""
import numpy as np
import pytest

from tests import mh_laws as ML
from tests import oracle_lib as O

KINDS = (101, 105, 102, 103, 113, 114, 120)
ENGINES = ("tries", "host")
N_AB = 4096 + 63        # (a), (b): not a multiple of 64
N_C = 1 << 15           # (c): the minority branch of every two-branch model expects more than mh_laws.MIN_CELL chains
N_C_DATA = 1 << 14      # (c) for the 200-observation model: the statement costs 200 terms per chain and walk
N_NUMPY = 1 << 15       # the numpy kernels on their own
SEED = 20261001

def n_c(kind):
    return N_C_DATA if kind == 105 else N_C


@pytest.mark.parametrize("kind", KINDS)
def test_input_conditions(kind):
    """on the numpy statement alone: every configuration with prior mass >= 0.05 keeps posterior mass >= 0.02; every structure-changing
    move carries at least 0.5 % of exact posterior draws across in each direction (a test must not pass because nothing moved)"""
    law = ML.make_law(kind)
    cs = law.configs()
    assert abs(sum(c.prior for c in cs) - 1) < 1e-12 and abs(sum(c.post for c in cs) - 1) < 1e-12
    assert all(c.post >= 0.02 for c in cs if c.prior >= 0.05), [(c.cfg, c.prior, c.post) for c in cs if c.prior >= 0.05]
    if kind == 101:
        assert cs[0].post >= 0.1          # the quadratic branch
    if kind == 120:
        mass = float(ML.stats.multivariate_normal(law.obs, law.cov).cdf(np.array([5.0, 5.0]), lower_limit=np.array([-5.0, -5.0])))
        assert abs(mass - law.box_mass) < 1e-6 and 0.3 < law.box_mass < 0.9      # (scipy's own accuracy; the Simpson value stands to 1e-13)
        return
    rng = np.random.default_rng(SEED + kind)
    old = law.sample(rng, 2 * N_NUMPY)
    single, joint, _ = ML.regen_masks(law)
    for pr in ML.proposals(law):
        if pr.changes is None:
            continue
        new, _ = ML.mh_move(law, pr, rng, old)
        a, b = old[0][:, pr.changes] != 0, new[0][:, pr.changes] != 0
        assert np.mean(a & ~b) >= 0.005 and np.mean(~a & b) >= 0.005, (pr.name, np.mean(a & ~b), np.mean(~a & b))
    new, _ = ML.regen_move(law, rng, old, joint)
    s = [q for q in joint if q in law.discrete][0]
    a, b = old[0][:, s] != 0, new[0][:, s] != 0
    assert np.mean(a & ~b) >= 0.005 and np.mean(~a & b) >= 0.005, (joint, np.mean(a & ~b), np.mean(~a & b))


@pytest.mark.parametrize("kind", KINDS)
def test_the_statement_in_mpmath(kind):
    law = ML.make_law(kind)
    v, p = law.sample(np.random.default_rng(SEED + 1), 24)
    ML.check_logjoint_mp(law, v, p, 24)
    v, p = law.prior_sample(np.random.default_rng(SEED + 2), 24)
    ML.check_logjoint_mp(law, v, p, 24)


@pytest.mark.parametrize("kind", KINDS)
def test_numpy_kernels_leave_the_exact_posterior(kind):
    """guards the statement: its own mh and regen_mh, one and five moves of every type, on its own exact draws"""
    law = ML.make_law(kind)
    rng = np.random.default_rng(SEED + 3)
    n = N_NUMPY // 8 if kind == 105 else N_NUMPY
    for mv in ML.moves_of(law):
        for k in (1, 5):
            cur = law.sample(rng, n)
            for it in range(k):
                if mv[0] == "mh":
                    cur, _ = ML.mh_move(law, mv[1], rng, cur)
                else:
                    cur, _ = ML.regen_move(law, rng, cur, [mv[1][it % len(mv[1])]] if mv[0] == "cycle" else mv[1])
            ML.check_exact_sample(law, cur, ("numpy", kind, mv[0], getattr(mv[1], "name", mv[1]), k))


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("kind", KINDS)
def test_logjoint_and_accept_decisions(kind, which):
    """(a) after creation, after planting, after every move; (b) every proposal, three rounds from planted posterior draws"""
    law = ML.make_law(kind)
    eng = ML.Engine(which, law, N_AB, SEED + 4)
    ML.check_logjoint(eng, "after creation")
    v, p = law.sample(np.random.default_rng(SEED + 5), N_AB)
    eng.plant(v, p)
    ML.check_logjoint(eng, "after planting")
    tally = ML.Tally()
    props = ML.proposals(law)
    for rnd in range(3):
        for pr in props:
            ML.check_accept_decisions(eng, pr, tally)
    tally.require(sorted({pr.changes for pr in props if pr.changes is not None}))
    single, joint, cycle = ML.regen_masks(law)
    for m in single + ([joint] if joint else []):
        eng.regen_mh(m, 1)
        ML.check_logjoint(eng, f"after regen_mh {m}")


@pytest.mark.parametrize("which", ENGINES)
@pytest.mark.parametrize("kind", KINDS)
def test_stationarity_from_planted_exact_draws(kind, which):
    """(c) every move type, k = 1 and 5"""
    law = ML.make_law(kind)
    made = 0
    for j, mv in enumerate(ML.moves_of(law)):
        for k in (1, 5):
            eng = ML.Engine(which, law, n_c(kind), SEED + 100 + 2 * j + (k == 5))
            made += ML.check_stationarity(eng, mv, k, SEED + 200 + 2 * j + (k == 5), dt=np.float64)
    assert made > 0


def test_handwritten_checker_engines():
    """(d) on the CPU: OracleMH and OraclePointedMH restate the two reference models by hand.  On the law data sets, over a schedule that
    visits every arm, they equal the "tries" engine bit for bit from the same seed, and their logjp is the statement's."""
    law = ML.make_law(101)
    n, seed = 3000, SEED + 7
    o = O.OracleMH(law.xs, law.ys, n, seed)
    e = ML.Engine("tries", law, n, seed)
    pr = {q.name: q for q in ML.proposals(law)}

    def same():
        # both keep logjp as the trie's RUNNING sum (update subtracts and adds log-densities): equal bit for bit; a running sum has no
        # term-count bound of its own, so against the statement it is held to the ceiling the suite used before, 1e-12 relative + 1e-10
        v, p = e.trace()
        assert np.array_equal(o.state(), v[:, :4])
        assert np.array_equal(o.logjp(), e.logjp())
        ref, _ = law.logjoint(v, p)
        assert np.all(np.abs(o.logjp().astype(ML.LD) - ref) <= 1e-10 + 1e-12 * np.abs(ref))
    same()
    for sweep in range(4):
        assert o.mh_add_or_remove(1) == e.mh(pr["add_or_remove"], 1); same()
        assert o.mh(0.1, 3) == e.mh(pr["drift 0.1"], 3); same()
        assert o.mh(0.02, 2) == e.mh(pr["drift 0.02"], 2); same()
        assert o.regen_mh([1, 2, 3], 3, cycle=True) == e.regen_mh([1, 2, 3], 3, cycle=True); same()
        assert o.regen_mh([2, 3], 1) == e.regen_mh([2, 3], 1); same()
    law = ML.make_law(120)
    o = O.OraclePointedMH(law.box, law.cov, law.obs, n, seed)
    e = ML.Engine("tries", law, n, seed)
    for sweep in range(3):
        for q in ML.proposals(law):
            assert o.mh(np.array(q.args).reshape(2, 2), 2) == e.mh(q, 2)
            v, p = e.trace()
            assert np.array_equal(o.state(), v[:, 1:3])
            ref, tol = law.logjoint(v, p)
            assert np.array_equal(o.logjp(), e.logjp()) and np.all(np.abs(o.logjp().astype(ML.LD) - ref) <= 1e-10 + 1e-12 * np.abs(ref))
