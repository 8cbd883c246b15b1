"""The canonical quantiles of DESIGN.md section 4 ("Quantiles"), restated in numpy and Python integers (modppl_amd/csrc/mp_quantiles.h
is the device's statement).  Integers only: no floating-point sum occurs, so no order of summation has to be reproduced.

    key(x)  = the order-preserving 64-bit image of a double: b = bits(x); ~b if the sign bit is set, else b | 2^63
    W_i     = a_i > 0 ? trunc(a_i S) : 0,  a_i = the weights of moments_ref.pf_weights,  S = 2^min(52, 63 - ceil_log2(n))
    A       = sum W_i;   tau(q) = max(1, ceil(q A)) with q the exact rational value of the double (fractions.Fraction)
    Q(q)    = the smallest key k with sum_{key_i <= k} W_i >= tau(q), returned as its double

Two statements: `select_sorted` (sort and cumulate) and `select_digits` (most significant digit first, 8 bits at a time, integer bin
sums — the device's method, written independently of the sort).  Plus the outside truth the mass bound is held against: long-double
exponentials and math.fsum.
"""
import math
from fractions import Fraction

import numpy as np

from tests import moments_ref as R

SIGN = np.uint64(1 << 63)


def keys(x):
    b = np.ascontiguousarray(x, dtype=np.float64).view(np.uint64)
    return np.where((b & SIGN) != 0, ~b, b | SIGN)


def unkey(k):
    k = np.uint64(k)
    b = (k & ~SIGN) if (k & SIGN) else ~k
    return np.array([b], dtype=np.uint64).view(np.float64)[0]


def scale(n):
    """S = 2^min(52, 63 - ceil_log2(n))"""
    return 2.0 ** min(52, 63 - R.ceil_log2(n))


def pf_int_weights(lw):
    """-> W uint64 [n]; None when every log-weight is -inf (the library's MP_ERR_DEGENERATE).  A NaN max gives all zeros."""
    lw = np.asarray(lw, dtype=np.float64)
    m = lw.max()                       # (numpy's max: a NaN wins, as the device's does)
    if m == -np.inf:
        return None
    if np.isnan(m):
        return np.zeros(lw.size, dtype=np.uint64)
    a = R.pf_weights(lw)[2]
    with np.errstate(invalid="ignore"):
        pos = a > 0                    # a NaN compares false
        return np.where(pos, np.trunc(np.where(pos, a, 0.0) * scale(lw.size)), 0.0).astype(np.uint64)


def target(q, A):
    """tau(q) = max(1, ceil(q A)), exactly"""
    q = float(q)
    assert 0.0 <= q <= 1.0
    return max(1, math.ceil(Fraction(q) * int(A)))


def select_sorted(v, W, qs):
    """sort and cumulate -> float64 [len(qs)]; NaN where A = 0"""
    k = keys(v)
    W = np.asarray(W, dtype=np.uint64)
    order = np.argsort(k, kind="stable")
    ks = k[order]
    cum = np.cumsum(W[order], dtype=np.uint64)               # A <= n S <= 2^63: no wrap
    A = int(cum[-1]) if W.size else 0
    out = np.full(len(qs), np.nan)
    if A == 0:
        return out
    for i, q in enumerate(qs):
        pos = int(np.searchsorted(cum, np.uint64(target(q, A)), side="left"))   # the first element whose running sum reaches tau
        out[i] = unkey(ks[pos])
    return out


def select_digits(v, W, qs, bits=8):
    """most significant digit first: per pass the integer bin sums of one key digit over the elements whose higher digits equal the
    prefix; the first digit whose running sum reaches the remaining target joins the prefix.  Nothing reaches it (A = 0): NaN."""
    k = keys(v)
    W = np.asarray(W, dtype=np.uint64)
    A = int(W.astype(object).sum()) if W.size else 0
    out = np.full(len(qs), np.nan)
    if A == 0:
        return out
    nb = 1 << bits
    for i, q in enumerate(qs):
        tau, live, prefix = target(q, A), np.ones(k.size, dtype=bool), 0
        for shift in range(64 - bits, -1, -bits):
            dg = ((k >> np.uint64(shift)) & np.uint64(nb - 1)).astype(np.int64)
            hist = [0] * nb
            for d_, w_ in zip(dg[live].tolist(), W[live].tolist()):
                hist[d_] += w_
            run = 0
            for digit in range(nb):
                if run + hist[digit] >= tau:
                    break
                run += hist[digit]
            tau -= run
            prefix = (prefix << bits) | digit
            live &= dg == digit
        out[i] = unkey(prefix)
    return out


def pf_quantiles(x, lw, qs):
    """-> [len(qs), d], bit for bit what mp_pf_quantiles returns; None for the degenerate cloud"""
    x = np.asarray(x, dtype=np.float64).reshape(len(lw), -1)
    W = pf_int_weights(lw)
    if W is None:
        return None
    return np.stack([select_sorted(x[:, j], W, qs) for j in range(x.shape[1])], axis=1)


def path_quantiles(paths, lw, qs):
    """paths [n, T, d] (trajectories()) -> [T, len(qs), d], bit for bit what mp_pf_path_quantiles returns"""
    paths = np.asarray(paths, dtype=np.float64)
    n, T, d = paths.shape
    W = pf_int_weights(lw)
    if W is None:
        return None
    out = np.empty((T, len(qs), d))
    for t in range(T):
        for j in range(d):
            out[t, :, j] = select_sorted(paths[:, t, j], W, qs)
    return out


def site_quantiles(vals, present, qs):
    """vals [n, ns], present [n] (bit s = site s is in chain i's trace) -> (count uint64 [ns], [len(qs), ns])"""
    vals = np.asarray(vals, dtype=np.float64)
    n, ns = vals.shape
    count, out = np.zeros(ns, dtype=np.uint64), np.empty((len(qs), ns))
    for s in range(ns):
        p = (np.asarray(present).astype(np.uint64) >> np.uint64(s)) & np.uint64(1)
        count[s] = int(p.sum())
        out[:, s] = select_sorted(vals[:, s], p, qs)
    return count, out


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(np.array_equal(a.view(np.uint64), b.view(np.uint64)))


# ---- outside truth --------------------------------------------------------------------------------------------------------------
def mass_epsilon(n):
    """the normalised integer CDF is within 2 n / S of the one built from the a_i themselves; 2^-50 for forming
    the truth's own quotients"""
    return 2.0 * n / scale(n) + 2.0 ** -50


def check_mass(v, lw, qs, got):
    """F(got) >= q - eps and F(got^-) <= q + eps, F the real-valued CDF from long-double exponentials and math.fsum.  Returns the worst
    slack used, as a fraction of eps (for printing)."""
    v, lw = np.asarray(v, dtype=np.float64), np.asarray(lw, dtype=np.float64)
    _, d, _ = R.pf_weights(lw)
    a = np.where(lw == -np.inf, np.longdouble(0), np.exp(d.astype(np.longdouble)))
    hi = a.astype(np.float64)
    lo = (a - hi.astype(np.longdouble)).astype(np.float64)
    total = math.fsum(hi.tolist() + lo.tolist())
    k, eps, worst = keys(v), mass_epsilon(len(lw)), -np.inf
    for q, g in zip(qs, np.asarray(got, dtype=np.float64)):
        kg = keys(np.array([g]))[0]
        le, lt = k <= kg, k < kg
        F_at = math.fsum(hi[le].tolist() + lo[le].tolist()) / total
        F_below = math.fsum(hi[lt].tolist() + lo[lt].tolist()) / total
        assert F_at >= q - eps, (q, g, F_at, eps)
        assert F_below <= q + eps, (q, g, F_below, eps)
        worst = max(worst, (q - F_at) / eps, (F_below - q) / eps)
    return worst
