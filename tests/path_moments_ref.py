"""The path moments of DESIGN.md section 4 ("Path moments"), restated in numpy on tests/moments_ref.py's tree sum and weights
(modppl_amd/csrc/mp_moments.h, k_path_mom1 / k_path_mom2, is the device's statement):

    v_i(t) = x_t[anc_i(t)];   mean[t][j] = TREE(a_i v_ij(t)) / A;   var[t][j] = TREE(a_i (v_ij(t) - mean[t][j])^2) / A;
    distinct[t] = the number of distinct anc_i(t) over all n slots.

Plus the walk of the event log that defines anc_i(t), and the outside truth the bounds are held against, per time step.
"""
import numpy as np

from tests import moments_ref as R


def ancestors(n, events):
    """events, oldest first: None for a step, a [n] array of parents for a resample  ->  anc [n, T] (T = the number of steps):
    the walk of k_trajectories, newest event first — a resample maps a <- parents[a], a step is time t read at the current a"""
    T = sum(e is None for e in events)
    anc = np.empty((n, T), dtype=np.int64)
    a, t = np.arange(n, dtype=np.int64), T
    for e in reversed(events):
        if e is None:
            t -= 1
            anc[:, t] = a
        else:
            a = np.asarray(e, dtype=np.int64)[a]
    return anc


def gather(xs, anc):
    """xs [T][n, d] per-step states, anc [n, T]  ->  paths [n, T, d]"""
    return np.stack([np.asarray(xs[t], dtype=np.float64).reshape(anc.shape[0], -1)[anc[:, t]] for t in range(anc.shape[1])], axis=1)


def path_moments(paths, lw, var=True):
    """paths [n, T, d], lw [n]  ->  (mean [T, d], var [T, d] or None), bit for bit what mp_pf_path_moments returns (up to the sign of a zero)"""
    paths = np.asarray(paths, dtype=np.float64)
    n, T, d = paths.shape
    _, _, a = R.pf_weights(lw)
    A = R.tree_sum(a)
    mean, v = np.empty((T, d)), (np.empty((T, d)) if var else None)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            for j in range(d):
                mean[t, j] = R.tree_sum(a * paths[:, t, j]) / A
                if var:
                    c = paths[:, t, j] - mean[t, j]
                    v[t, j] = R.tree_sum(a * (c * c)) / A
    return mean, v


def distinct(anc):
    """anc [n, T]  ->  uint64 [T]"""
    anc = np.asarray(anc)
    return np.array([len(np.unique(anc[:, t])) for t in range(anc.shape[1])], dtype=np.uint64)


def check_bounds(paths, lw, mean, var):
    """per (t, j): |mean - E| <= (2 l + 8) u sum a |v| / A;  |var - V| <= (2 l + 12) u sum a c^2 / A with c centred at the mean that was
    returned (the bounds of moments_ref.check_bounds: the gather adds no arithmetic); var >= 0.  -> the worst ratios error / bound"""
    paths = np.asarray(paths, dtype=np.float64)
    n, T, d = paths.shape
    l = R.ceil_log2(n)
    _, dd, _ = R.pf_weights(lw)
    dead = np.asarray(lw) == -np.inf
    a = np.where(dead, np.longdouble(0), np.exp(dd.astype(np.longdouble)))
    A = R._prod_sum(a, np.ones(n))
    rm = rv = 0.0
    for t in range(T):
        for j in range(d):
            x = paths[:, t, j]
            E, S = R._prod_sum(a, x) / A, R._prod_sum(a, np.abs(x)) / A
            em, bm = abs(mean[t, j] - E), (2 * l + 8) * R.U * S
            assert em <= bm, (t, j, em, bm)
            rm = max(rm, em / bm if bm > 0 else 0.0)
            if var is not None:
                c = x.astype(np.longdouble) - np.longdouble(mean[t, j])
                p = a * c * c
                hi = p.astype(np.float64)
                lo = (p - hi.astype(np.longdouble)).astype(np.float64)
                V = R._fsum(np.concatenate([hi, lo])) / A
                ev, bv = abs(var[t, j] - V), (2 * l + 12) * R.U * V
                assert ev <= bv and var[t, j] >= 0, (t, j, ev, bv, var[t, j])
                rv = max(rv, ev / bv if bv > 0 else 0.0)
    return rm, rv
