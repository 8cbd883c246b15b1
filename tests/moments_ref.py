"""The canonical moments of DESIGN.md section 4, restated in numpy (modppl_amd/csrc/mp_moments.h is the device's statement).

    TREE(v): pad v with +0.0 up to the next power of two; repeat v <- v[0::2] + v[1::2] until one element is left.

Everything else is elementwise IEEE fp64 around that one line; `mp_exp` is the checker's (tests/oracle_lib.py, oracle_mp_exp), the same
source the device compiles.  Plus the outside truth the bounds are held against: long-double exponentials and math.fsum.
"""
import math

import numpy as np

U = 2.0 ** -53


def tree_sum(v):
    v = np.asarray(v, dtype=np.float64).ravel()
    p = 1 << max(0, int(v.size - 1).bit_length())
    v = np.concatenate([v, np.zeros(p - v.size)])
    while v.size > 1:
        v = v[0::2] + v[1::2]
    return float(v[0])


def mp_exp(x):
    from tests import oracle_lib as O

    x = np.ascontiguousarray(x, dtype=np.float64)
    out = np.empty_like(x)
    if x.size:
        O.load().oracle_mp_exp(O.dptr(x), x.size, O.dptr(out))
    return out


def pf_weights(lw):
    """(m, d_i = lw_i - m as rounded, a_i); None when every log-weight is -inf (the library's MP_ERR_DEGENERATE)"""
    lw = np.asarray(lw, dtype=np.float64)
    m = lw.max()
    if m == -np.inf:
        return None
    dead = lw == -np.inf
    d = np.where(dead, 0.0, lw) - m
    return m, d, np.where(dead, 0.0, mp_exp(d))


def pf_moments(x, lw, cov=True):
    """-> (mean [d], cov [d, d] or None), bit for bit what mp_pf_moments returns (up to the sign of a zero)"""
    x = np.asarray(x, dtype=np.float64).reshape(len(lw), -1)
    _, _, a = pf_weights(lw)
    A = tree_sum(a)
    dim = x.shape[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean = np.array([tree_sum(a * x[:, j]) / A for j in range(dim)])
        if not cov:
            return mean, None
        c = x - mean
        C = np.empty((dim, dim))
        for j in range(dim):
            for k in range(j + 1):
                C[j, k] = C[k, j] = tree_sum(a * (c[:, j] * c[:, k])) / A
    return mean, C


def site_moments(vals, present, var=True):
    """vals [n, ns], present [n] (bit s = site s is in chain i's trace) -> (count uint64 [ns], mean [ns], var [ns] or None)"""
    vals = np.asarray(vals, dtype=np.float64)
    n, ns = vals.shape
    present = np.asarray(present).astype(np.uint64)
    count, mean, v = np.zeros(ns, dtype=np.uint64), np.empty(ns), np.empty(ns)
    with np.errstate(invalid="ignore", divide="ignore"):
        for s in range(ns):
            p = ((present >> np.uint64(s)) & np.uint64(1)).astype(bool)
            count[s] = int(p.sum())
            cnt = np.float64(count[s])
            mean[s] = np.float64(tree_sum(np.where(p, vals[:, s], 0.0))) / cnt
            cs = np.where(p, vals[:, s] - mean[s], 0.0)
            v[s] = np.float64(tree_sum(np.where(p, cs * cs, 0.0))) / cnt
    return count, mean, (v if var else None)


def same_numbers(a, b):
    """equal as numbers: bit-equal up to the sign of a zero; NaN matches NaN"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- outside truth --------------------------------------------------------------------------------------------------------------
def _fsum(v):
    return math.fsum(np.asarray(v, dtype=np.float64).tolist())


def _prod_sum(a, *fs):
    """sum_i a_i prod_f f_i, with a long double and fs float64: the products are exact in 2 x float64 pieces only approximately, so
    they are formed in long double (64-bit mantissa: relative error 2^-64 per operation, 2^-11 u) and summed with fsum in two float64 pieces"""
    p = a.copy()
    for f in fs:
        p = p * f.astype(np.longdouble)
    hi = p.astype(np.float64)
    lo = (p - hi.astype(np.longdouble)).astype(np.float64)
    return _fsum(np.concatenate([hi, lo]))


def pf_truth(x, lw, mean_dev=None):
    """Exact-as-can-be moments for the arguments d_i AS ROUNDED in fp64 (that subtraction is part of the definition): exp in long
    double, sums by math.fsum.  -> (E [d], mean bound scale [d] = sum a |x| / A, C [d, d] centred at mean_dev, cov bound scale [d, d] =
    sum a |c_j| |c_k| / A); the latter two None without mean_dev."""
    x = np.asarray(x, dtype=np.float64).reshape(len(lw), -1)
    _, d, _ = pf_weights(lw)
    dead = np.asarray(lw) == -np.inf
    a = np.where(dead, np.longdouble(0), np.exp(d.astype(np.longdouble)))
    one = np.ones(len(lw))
    A = _prod_sum(a, one)
    dim = x.shape[1]
    E = np.array([_prod_sum(a, x[:, j]) / A for j in range(dim)])
    S = np.array([_prod_sum(a, np.abs(x[:, j])) / A for j in range(dim)])
    if mean_dev is None:
        return E, S, None, None
    c = x.astype(np.longdouble) - np.asarray(mean_dev, dtype=np.float64).astype(np.longdouble)
    C, SC = np.empty((dim, dim)), np.empty((dim, dim))
    for j in range(dim):
        for k in range(j + 1):
            pj = a * c[:, j] * c[:, k]
            hi = pj.astype(np.float64)
            lo = (pj - hi.astype(np.longdouble)).astype(np.float64)
            C[j, k] = C[k, j] = _fsum(np.concatenate([hi, lo])) / A
            SC[j, k] = SC[k, j] = float(np.sum(np.abs(pj))) / A   # (a scale, not a value: long-double pairwise sum)
    return E, S, C, SC


def ceil_log2(n):
    return max(0, int(n - 1).bit_length())


def check_bounds(x, lw, mean, cov):
    """the issue's bounds: |mean_j - E_j| <= (2 l + 8) u sum a |x_j| / A;  |cov_jk - C_jk| <= (2 l + 12) u sum a |c_j||c_k| / A with C
    centred at the mean that was returned; exact symmetry, diagonal >= 0.  Returns the worst ratios error / bound (for printing)."""
    n = len(lw)
    l = ceil_log2(n)
    E, S, C, SC = pf_truth(x, lw, mean if cov is not None else None)
    em = np.abs(mean - E)
    bm = (2 * l + 8) * U * S
    assert np.all(em <= bm), (em, bm)
    rm = float(np.max(np.where(bm > 0, em / np.where(bm > 0, bm, 1), 0.0)))
    rc = 0.0
    if cov is not None:
        ec = np.abs(cov - C)
        bc = (2 * l + 12) * U * SC
        assert np.all(ec <= bc), (ec, bc)
        assert np.array_equal(cov, cov.T) and np.all(np.diag(cov) >= 0)
        rc = float(np.max(np.where(bc > 0, ec / np.where(bc > 0, bc, 1), 0.0)))
    return rm, rc
