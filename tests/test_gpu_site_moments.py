"""GPU: FunctionChains.site_moments() (mp_mh_site_moments) — per-site count, mean and variance over the chains of a registered function,
reduced on the device, against the numpy restatement (tests/moments_ref.py) applied to what mp_mh_read_trace hands
back in the same state.  Nothing is planted: the values and presence bits are what the MH kernels produced.
Without mp_mh_site_moments every test here fails at the missing symbol."""
import numpy as np
import pytest

from tests import moments_ref as R

pytestmark = pytest.mark.gpu

SIZES = [1, 2049, (1 << 16) + 63]
XS = np.linspace(-2.0, 2.0, 16)
YS = 0.4 - 1.1 * XS + 0.6 * XS * XS + 0.1 * np.random.default_rng(41).normal(size=16)


def check(fc):
    count, mean, var = fc.site_moments()
    vals, present = fc.trace()
    rc, rm, rv = R.site_moments(vals, present)
    assert count.dtype == np.uint64 and np.array_equal(count, rc), (count, rc)
    assert R.same_numbers(mean, rm), (mean, rm)
    assert R.same_numbers(var, rv), (var, rv)
    none = count == 0
    assert np.isnan(mean[none]).all() and np.isnan(var[none]).all()
    assert np.isfinite(mean[~none]).all() and (var[~none] >= 0).all()
    c2, m2, v2 = fc.site_moments(var=False)
    assert v2 is None and np.array_equal(c2, count) and R.same_numbers(m2, mean)
    return count, mean, var


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("is_linear", [0.0, 1.0])
def test_hierarchical_functor_every_site_present_or_one_absent_everywhere(n, is_linear):
    """kind 101 with 16 observations: constrained to the quadratic branch all 20 sites are in every trace; constrained to the linear
    one `coeffs/c` is in none (count 0, NaN moments)"""
    import modppl_amd
    from modppl_amd import capi

    cons = {capi.MP_SITE_Y0 + k: float(y) for k, y in enumerate(YS)}
    cons[capi.MP_SITE_IS_LINEAR] = is_linear
    fc = modppl_amd.FunctionChains(capi.MP_MH_MODEL_HIERARCHICAL_FN, XS, cons, n, 31)
    assert fc.num_sites == 20
    check(fc)
    fc.mh(capi.MP_MH_PROPOSAL_HIERARCHICAL_DRIFT, [0.2], 3)
    fc.regen_mh([capi.MP_SITE_A, capi.MP_SITE_B], 2, cycle=True)
    count, mean, var = check(fc)
    want = np.full(20, n, dtype=np.uint64)
    if is_linear:
        want[capi.MP_SITE_C] = 0
    assert np.array_equal(count, want)
    assert np.allclose(mean[capi.MP_SITE_Y0:], YS, rtol=1e-14, atol=0)     # every chain holds the same observation


@pytest.mark.parametrize("n", SIZES)
def test_presence_differs_between_chains_above_bit_32(n):
    """kind 114 (41 sites, two presence words per chain): the add-or-remove proposal and a masked regenerate make `o2` (site 34) come
    and go, so the masked path runs on a bit of the high word"""
    import modppl_amd
    from tests.test_oracle_mh_functor import WF_BIG, WF_NS, WF_O1, WF_O2, wide_problem

    xs, cons = wide_problem()
    fc = modppl_amd.FunctionChains(114, xs, cons, n, 5)
    assert fc.num_sites == WF_NS
    check(fc)
    for sweep in range(2):
        fc.mh(1, [0.15], 2)
        fc.mh(2, [], 2)
        fc.regen_mh([WF_O1], 2)
        fc.regen_mh([WF_BIG, WF_O2], 2)
    count, mean, var = check(fc)
    if n > 1:
        assert 0 < count[WF_O2] < n, count
        assert var[WF_O2] > 0


def test_hand_written_chains_are_unsupported():
    import modppl_amd
    from modppl_amd import capi

    h = modppl_amd.HierarchicalChains(XS, YS, 256, 3, functor=False)
    p = modppl_amd.PointedChains([-5.0, 5.0, -5.0, 5.0], [[1.0, -0.6], [-0.6, 2.0]], [0.5, -0.25], 256, 3, functor=False)
    for chains in (h, p):
        with pytest.raises(capi.ModpplError) as err:
            chains.site_moments()
        assert err.value.code == capi.MP_ERR_UNSUPPORTED
    # (the C entry point itself, not only the wrapper's first call)
    import ctypes as C
    cnt, m = (C.c_uint64 * 64)(), (C.c_double * 64)()
    L = capi.load()
    for chains in (h, p):
        assert L.mp_mh_site_moments(chains._h, cnt, m, None) == capi.MP_ERR_UNSUPPORTED
    f = modppl_amd.HierarchicalChains(XS, YS, 256, 3, functor=True)
    assert f.site_moments()[0][capi.MP_SITE_A] == 256
