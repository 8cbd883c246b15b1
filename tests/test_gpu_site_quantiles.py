"""GPU: FunctionChains.site_quantiles() (mp_mh_site_quantiles) — per-site quantiles over the chains of a registered function, selected on
the device, compared BIT FOR BIT with the restatement (tests/quantiles_ref.py; DESIGN.md section 4, "Quantiles") applied to what
mp_mh_read_trace hands back in the same state.  Nothing is planted: the values and presence bits are what the MH kernels produced.
Without mp_mh_site_quantiles every test here fails at the missing symbol or method."""
import ctypes as C

import numpy as np
import pytest

from tests import quantiles_ref as Q
from tests.test_gpu_site_moments import XS, YS

pytestmark = pytest.mark.gpu

SIZES = [1, 3001]
QS = [0.5, 0.05, 0.95, 0.0, 1.0, 0.5]       # unsorted, with a duplicate


def check(fc, qs=QS):
    count, got = fc.site_quantiles(qs)
    vals, present = fc.trace()
    rc, want = Q.site_quantiles(vals, present, qs)
    assert count.dtype == np.uint64 and np.array_equal(count, rc), (count, rc)
    assert got.shape == (len(qs), fc.num_sites)
    assert Q.same_bits(got, want), (got, want)
    assert np.array_equal(count, fc.site_moments()[0])
    none = count == 0
    assert np.isnan(got[:, none]).all() and np.isfinite(got[:, ~none]).all()
    return count, got


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("is_linear", [None, 0.0, 1.0])
def test_hierarchical_functor_c_is_there_iff_quadratic(n, is_linear):
    """kind 101 with 16 observations.  `is_linear` unconstrained: every chain draws its own branch, so `coeffs/c` is in the traces of the
    quadratic chains only; constrained to the linear branch it is in none (count 0, NaN), to the quadratic one in all."""
    import modppl_amd
    from modppl_amd import capi

    cons = {capi.MP_SITE_Y0 + k: float(y) for k, y in enumerate(YS)}
    if is_linear is not None:
        cons[capi.MP_SITE_IS_LINEAR] = is_linear
    fc = modppl_amd.FunctionChains(capi.MP_MH_MODEL_HIERARCHICAL_FN, XS, cons, n, 31)
    assert fc.num_sites == 20
    check(fc)
    fc.mh(capi.MP_MH_PROPOSAL_HIERARCHICAL_DRIFT, [0.2], 3)
    fc.regen_mh([capi.MP_SITE_A, capi.MP_SITE_B], 2, cycle=True)
    count, got = check(fc)
    vals, present = fc.trace()
    quadratic = int((vals[:, capi.MP_SITE_IS_LINEAR] == 0.0).sum())
    assert count[capi.MP_SITE_C] == quadratic and count[capi.MP_SITE_A] == n
    if is_linear is None and n > 1:
        assert 0 < quadratic < n
    if is_linear == 1.0:
        assert count[capi.MP_SITE_C] == 0 and np.isnan(got[:, capi.MP_SITE_C]).all()
    assert Q.same_bits(got[:, capi.MP_SITE_Y0:], np.tile(YS, (len(QS), 1)))      # every chain holds the same observation
    check(fc, [0.5])
    check(fc, [k / 15 for k in range(16)])


@pytest.mark.parametrize("n", SIZES)
def test_presence_differs_between_chains_above_bit_32(n):
    """kind 114 (41 sites, two presence words per chain): `o2` (site 34) comes and goes, so the presence test runs on the high word"""
    import modppl_amd
    from tests.test_oracle_mh_functor import WF_BIG, WF_NS, WF_O1, WF_O2, wide_problem

    xs, cons = wide_problem()
    fc = modppl_amd.FunctionChains(114, xs, cons, n, 5)
    assert fc.num_sites == WF_NS
    for sweep in range(2):
        fc.mh(1, [0.15], 2)
        fc.mh(2, [], 2)
        fc.regen_mh([WF_O1], 2)
        fc.regen_mh([WF_BIG, WF_O2], 2)
    count, got = check(fc)
    if n > 1:
        assert 0 < count[WF_O2] < n, count


def test_hand_written_chains_are_unsupported_and_the_other_statuses():
    import modppl_amd
    from modppl_amd import capi

    h = modppl_amd.HierarchicalChains(XS, YS, 256, 3, functor=False)
    p = modppl_amd.PointedChains([-5.0, 5.0, -5.0, 5.0], [[1.0, -0.6], [-0.6, 2.0]], [0.5, -0.25], 256, 3, functor=False)
    for chains in (h, p):
        with pytest.raises(capi.ModpplError) as err:
            chains.site_quantiles([0.5])
        assert err.value.code == capi.MP_ERR_UNSUPPORTED
    # (the C entry point itself, not only the wrapper's first call)
    cnt, out, qs = (C.c_uint64 * 64)(), (C.c_double * 64)(), (C.c_double * 17)(*([0.5] * 17))
    L = capi.load()
    for chains in (h, p):
        assert L.mp_mh_site_quantiles(chains._h, qs, 1, cnt, out) == capi.MP_ERR_UNSUPPORTED
    f = modppl_amd.HierarchicalChains(XS, YS, 256, 3, functor=True)
    pf = modppl_amd.PointedChains([-5.0, 5.0, -5.0, 5.0], [[1.0, -0.6], [-0.6, 2.0]], [0.5, -0.25], 256, 3, functor=True)
    count, got = f.site_quantiles([0.0, 1.0])
    assert count[capi.MP_SITE_A] == 256 and got[0, capi.MP_SITE_A] <= got[1, capi.MP_SITE_A]
    assert pf.site_quantiles([0.5])[0].max() == 256
    assert L.mp_mh_site_quantiles(None, qs, 1, cnt, out) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(f._h, None, 1, cnt, out) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(f._h, qs, 1, None, out) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(f._h, qs, 1, cnt, None) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(f._h, qs, 0, cnt, out) == capi.MP_ERR_INVALID_ARG
    assert L.mp_mh_site_quantiles(f._h, qs, 17, cnt, out) == capi.MP_ERR_INVALID_ARG
    for bad in (float("nan"), -0.25, 1.25):
        assert L.mp_mh_site_quantiles(f._h, (C.c_double * 1)(bad), 1, cnt, out) == capi.MP_ERR_INVALID_ARG
