"""mp_sin, mp_cos and mp_atan2 (modppl_amd/csrc/mp_math.h) against exact references, on the host through the CPU checker's
bindings.  The device evaluates the same definitions bit for bit (tests/test_gpu_math.py); this file checks that the definitions
compute the right numbers.

The sin / cos reference reduces exactly: x - n pi/2 is formed as an error-free expansion of x and the products n * P_k, where P_k are
the 32-bit pieces of pi/2 to 352 bits (each product is exact: n < 2^21), then summed in long double (64-bit significand) and
passed to sinl / cosl on |r| <= pi/4, where those need no reduction of their own.  Its relative error, stated and asserted against
mpmath at 256 bits on a sample of each set, is below 2^-60, i.e. under 1/128 ulp of a double.

Measured on the argument sets below (maximum error in ulps of the correctly rounded result):
  sin 0.77, cos 0.77 on 2.1 M random arguments: [-10, 10], the whole domain, and log-uniform magnitudes down to 1e-300;
  sin 0.50, cos 0.50 on the 6.3 M doubles next to +-n pi/2, n = 1 .. 2^20 - 1 (asserted: below 1);
  atan2 1.47 on 2 M random pairs over the four quadrants and exponent ratios 2^-120 .. 2^120 (asserted: at most 2).

mp_rem_pio2 is fdlibm's medium case (e_rem_pio2.c): pi/2 in 33-bit pieces, a second iteration when the first cancels more than 16
bits and a third when the second leaves more than 49.  The third matters in this domain.  Each double next to n pi/2 cancels about 53
bits, at most 73 (x = 321307.9594422229).  With two iterations only, x = 413441.44719405076 (n = 263205, 70 bits) gave 1.06 ulp:
above the bound below.  With all three, the near-multiple set is within 0.5 ulp.  The three give 151 bits, enough for 53 + 73.
Without the second iteration the near-multiple set errs by 2e11 ulp, and random arguments by 150 ulp.
"""
import math

import mpmath
import numpy as np
import pytest

from tests import oracle_lib as O

DOMAIN = 1647099.0   # mp_math.h: |x| < 2^20 pi/2 is reduced, anything else is NaN
REF_REL_ERR = 2.0 ** -60


@pytest.fixture(scope="module")
def L(oracle):
    return oracle


def _sin(L, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    L.oracle_mp_sin(O.dptr(x), x.size, O.dptr(out))
    return out


def _cos(L, x):
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    L.oracle_mp_cos(O.dptr(x), x.size, O.dptr(out))
    return out


def _atan2(L, y, x):
    y = np.ascontiguousarray(y, dtype=np.float64)
    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(y)
    L.oracle_mp_atan2(O.dptr(y), O.dptr(x), y.size, O.dptr(out))
    return out


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.uint64)


def ulp_err(got, ref_ld):
    """|got - ref| in ulps of the double nearest ref (ref in long double)"""
    ref_d = ref_ld.astype(np.float64)
    ulp = np.spacing(np.abs(ref_d)).astype(np.longdouble)
    return np.abs(got.astype(np.longdouble) - ref_ld) / ulp


# pi/2 to 352 bits as eleven doubles of at most 32 significant bits each: n * P_k is exact for n < 2^21
def _pio2_pieces():
    with mpmath.workprec(420):
        I = int(mpmath.floor(mpmath.pi / 2 * mpmath.mpf(2) ** (31 + 32 * 10)))
    pieces = []
    for k in range(11):
        c = (I >> (32 * (10 - k))) & 0xFFFFFFFF
        pieces.append(math.ldexp(c, -31 - 32 * k))
    return pieces


PIO2 = _pio2_pieces()


def _two_sum(a, b):
    s = a + b
    bb = s - a
    return s, (a - (s - bb)) + (b - bb)


def _exact_sum_ld(terms):
    """sum of arrays of doubles, exact until the final rounding to long double (~2^-63 relative): Shewchuk's grow-expansion"""
    comps = []
    for t in terms:
        q, new = t, []
        for c in comps:
            q, h = _two_sum(q, c)
            new.append(h)
        comps = new + [q]
    r = np.zeros(terms[0].shape, dtype=np.longdouble)
    for c in comps:   # ascending magnitude, non-overlapping
        r += c.astype(np.longdouble)
    return r


def exact_reduce(x):
    """-> (n mod 4, r in long double, cancelled bits) with x = n pi/2 + r, |r| <= pi/4 (+ rounding of n), r to ~2^-63 relative"""
    x = np.asarray(x, dtype=np.float64)
    n = np.rint(x * (2 / math.pi))
    r = _exact_sum_ld([x] + [-n * p for p in PIO2])   # x - n * (pi/2 to 352 bits)
    with np.errstate(divide="ignore"):
        lost = np.floor(np.log2(np.abs(x))) - np.floor(np.log2(np.abs(r.astype(np.float64))))
    return n.astype(np.int64) & 3, r, lost


def ref_sin_cos(x):
    q, r, lost = exact_reduce(x)
    s, c = np.sin(r), np.cos(r)
    sin = np.choose(q, [s, c, -s, -c])
    cos = np.choose(q, [c, -s, -c, s])
    return sin, cos, q, lost


def _ld_to_mpf(v):
    """a long double exactly: its 64-bit significand is the sum of two doubles"""
    hi = float(v)
    return mpmath.mpf(hi) + mpmath.mpf(float(v - np.longdouble(hi)))


def _check_reference_against_mpmath(x, sin_ref, cos_ref, k=400):
    idx = np.random.default_rng(1).choice(x.size, min(k, x.size), replace=False)
    with mpmath.workprec(256):
        for i in idx:
            xi = mpmath.mpf(float(x[i]))
            for ref, f in ((sin_ref[i], mpmath.sin), (cos_ref[i], mpmath.cos)):
                exact = f(xi)
                err = abs(_ld_to_mpf(ref) - exact)
                assert err <= REF_REL_ERR * abs(exact), (float(x[i]), float(err / abs(exact)))


def test_reference_is_long_double():
    assert np.finfo(np.longdouble).nmant >= 63, "the exact references need x87 long double"


def test_sin_cos_random_arguments(L):
    rng = np.random.default_rng(2024)
    n = 700_000
    x = np.concatenate([rng.uniform(-10, 10, n), rng.uniform(-DOMAIN, DOMAIN, n) * (1 - 2 ** -40),
                        np.exp(rng.uniform(math.log(1e-300), math.log(DOMAIN), n)) * rng.choice([-1., 1.], n)])
    s_ref, c_ref, _, _ = ref_sin_cos(x)
    _check_reference_against_mpmath(x, s_ref, c_ref)
    es, ec = ulp_err(_sin(L, x), s_ref), ulp_err(_cos(L, x), c_ref)
    assert es.max() < 1.0, (float(es.max()), float(x[es.argmax()]))
    assert ec.max() < 1.0, (float(ec.max()), float(x[ec.argmax()]))


def test_sin_cos_tiny_and_subnormal_arguments(L):
    rng = np.random.default_rng(5)
    m = rng.uniform(1, 2, 200_000)
    x = np.ldexp(m, rng.integers(-1074, -20, m.size)) * rng.choice([-1., 1.], m.size)
    x = np.concatenate([x, [5e-324, -5e-324, 2.2250738585072014e-308, -2.2250738585072009e-308, 0.0, -0.0, 2 ** -27, 2 ** -26]])
    s_ref, c_ref = np.sin(x.astype(np.longdouble)), np.cos(x.astype(np.longdouble))
    s, c = _sin(L, x), _cos(L, x)
    nz = x != 0
    assert ulp_err(s[nz], s_ref[nz]).max() < 1.0
    assert ulp_err(c, c_ref).max() < 1.0
    sub = np.abs(x) < 2 ** -27
    assert np.array_equal(_bits(s[sub]), _bits(x[sub]))   # sin x = x, signed zeros and subnormals included
    assert np.all(c[sub] == 1.0)


def near_multiples_of_pio2(nmax=1 << 20, width=1):
    """the double nearest n pi/2 and `width` neighbours on each side, n = 1 .. nmax, both signs of x"""
    k = np.arange(1, nmax + 1, dtype=np.float64)
    near = _exact_sum_ld([k * p for p in PIO2]).astype(np.float64)   # (a double rounding at worst: the neighbours cover it)
    xs = [near]
    up, dn = near.copy(), near.copy()
    for _ in range(width):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, -np.inf)
        xs += [up, dn]
    x = np.concatenate(xs)
    return np.concatenate([x, -x])


def test_the_last_multiple_is_outside_the_domain(L):
    """2^20 pi/2 = 1647099.33 lies beyond the bound: n = 2^20 gives NaN, every smaller n is reduced"""
    x = near_multiples_of_pio2()
    out = np.abs(x) >= DOMAIN
    assert np.all(np.abs(x[out]) > 1647099.3) and out.sum() == 6
    assert np.all(np.isnan(_sin(L, x[out]))) and np.all(np.isnan(_cos(L, x[out])))


def test_sin_cos_next_to_multiples_of_pio2(L):
    x = near_multiples_of_pio2()
    x = x[np.abs(x) < DOMAIN]
    s_ref, c_ref, q, lost = ref_sin_cos(x)
    s, c = _sin(L, x), _cos(L, x)
    es, ec = ulp_err(s, s_ref), ulp_err(c, c_ref)
    # the value that is +-sin r: sin for even n, cos for odd n; the other one is +-cos r, near 1
    small = np.where(q % 2 == 0, es, ec)
    assert small.max() < 1.0, (float(small.max()), float(x[small.argmax()]))
    assert max(es.max(), ec.max()) < 1.0
    # the docstring's claim: the deepest cancellation in the domain, and 53 result bits on top of it, fit in the 151 bits of three
    # iterations
    assert 60 < lost.max() <= 151 - 53, lost.max()
    i = np.random.default_rng(3).choice(x.size, 300, replace=False)
    i = np.concatenate([i, np.argsort(lost)[-100:]])   # the deepest cancellations too
    _check_reference_against_mpmath(x[i], s_ref[i], c_ref[i])


def test_sin_cos_domain_contract(L):
    """mp_math.h: |x| >= 1647099, +-inf and NaN give NaN; just inside the bound is reduced"""
    bad = np.array([DOMAIN, -DOMAIN, np.nextafter(DOMAIN, np.inf), 1e7, -1e300, 1.7976931348623157e308, np.inf, -np.inf, np.nan])
    assert np.all(np.isnan(_sin(L, bad))) and np.all(np.isnan(_cos(L, bad)))
    ok = np.array([np.nextafter(DOMAIN, 0), -np.nextafter(DOMAIN, 0), 1647098.5])
    s_ref, c_ref, _, _ = ref_sin_cos(ok)
    assert ulp_err(_sin(L, ok), s_ref).max() < 1.0 and ulp_err(_cos(L, ok), c_ref).max() < 1.0


def _random_pairs(rng, n):
    my, mx = rng.uniform(1, 2, n), rng.uniform(1, 2, n)
    ey = rng.integers(-500, 500, n)
    ex = ey - rng.integers(-120, 121, n)
    y = np.ldexp(my, ey) * rng.choice([-1., 1.], n)
    x = np.ldexp(mx, ex) * rng.choice([-1., 1.], n)
    return y, x


def test_atan2_random_pairs(L):
    rng = np.random.default_rng(77)
    y, x = _random_pairs(rng, 1_000_000)
    y2 = rng.normal(0, 1, 1_000_000)
    x2 = rng.normal(0, 1, 1_000_000)
    y, x = np.concatenate([y, y2]), np.concatenate([x, x2])
    ref = np.arctan2(y.astype(np.longdouble), x.astype(np.longdouble))
    idx = rng.choice(y.size, 400, replace=False)
    with mpmath.workprec(256):
        for i in idx:
            exact = mpmath.atan2(mpmath.mpf(float(y[i])), mpmath.mpf(float(x[i])))
            assert abs(_ld_to_mpf(ref[i]) - exact) <= REF_REL_ERR * abs(exact)
    err = ulp_err(_atan2(L, y, x), ref)
    assert err.max() <= 2.0, (float(err.max()), float(y[err.argmax()]), float(x[err.argmax()]))


def test_atan2_special_cases_are_numpys_bits(L):
    z, inf, nan = 0.0, np.inf, np.nan
    vals = [z, -z, 1.0, -1.0, 0.5, -3.0, inf, -inf, nan, 5e-324, -5e-324, 1e300, -1e300, 2.0 ** 61, -(2.0 ** 61), 2.0 ** -61]
    y, x = np.meshgrid(vals, vals)
    y, x = y.ravel(), x.ravel()
    special = lambda v: (v == 0) | np.isinf(v) | np.isnan(v)
    keep = special(y) | special(x) | (x == 1.0)
    y, x = y[keep], x[keep]
    # |y/x| beyond 2^60 and 2^-60 (exponents apart by more than 60) in every quadrant, and x = 1 exactly (atan2 is atan there)
    e = np.array([61, 62, 100, 1000, -61, -62, -100, -1000], dtype=np.float64)
    for sy in (1., -1.):
        for sx in (1., -1.):
            for m in (1.0, 1.5, 1.9999999999999998):
                y = np.concatenate([y, sy * m * np.ones(e.size), sy * np.ldexp(m, e.astype(int))])
                x = np.concatenate([x, sx * np.ldexp(1.0, (-e).astype(int)), sx * np.ones(e.size)])
    got, want = _atan2(L, y, x), np.arctan2(y, x)
    nan_w = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan_w)
    bad = ~nan_w & (_bits(got) != _bits(want))
    assert not bad.any(), list(zip(y[bad][:8], x[bad][:8], got[bad][:8], want[bad][:8]))


def test_atan_branch_edges(L):
    """mp_atan's intervals (0.4375, 0.6875, 1.1875, 2.4375) and its cut-offs (2^-28, 2^66), each with neighbours, through
    atan2(y, 1) = atan(y)"""
    edges = np.array([0.4375, 0.6875, 1.1875, 2.4375, 2.0 ** -28, 2.0 ** 66])
    ys = [edges]
    up, dn = edges.copy(), edges.copy()
    for _ in range(3):
        up, dn = np.nextafter(up, np.inf), np.nextafter(dn, 0)
        ys += [up, dn]
    y = np.concatenate(ys + [np.linspace(0.01, 5, 500)])
    y = np.concatenate([y, -y])
    got = _atan2(L, y, np.ones_like(y))
    ref = np.arctan(y.astype(np.longdouble))
    assert ulp_err(got, ref).max() < 1.0
    # atan is odd and monotone across every edge
    assert np.array_equal(got[:y.size // 2], -got[y.size // 2:])
    o = np.argsort(y)
    assert np.all(np.diff(got[o]) >= 0)
