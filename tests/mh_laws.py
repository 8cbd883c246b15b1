"""The Metropolis-Hastings models, their proposals and the two MH kernels written down a second time, in numpy, from their prose:
the comment block above each functor in modppl_amd/csrc/mp_mh_models.h and the reference's own text (modppl/tests/dyngenfns/
hierarchical.rs, simple.rs; modppl/src/inference/mh.rs:9-75 read as mathematics).  Nothing here includes, parses or calls the C++,
and no arithmetic of the library is used: the device and the CPU checker interpret the same functor source, so parity between them
cannot see a wrong constant in a model body, a shared misreading of the accept rule or a handler rule that is self-consistent but
not the law.  These statements can.

A model is a `body(w)` over a walker `_Walk` — a dozen lines that read like the prose.  One walker gives, in np.longdouble (and in
mpmath at 160 bits for a spot check): the log-density of every site of a trace, with the sites each branch must hold; a redraw of
chosen sites from their stated distributions (the numpy form of regen_mh's proposal); and the presence word a set of values demands.
A proposal is a body over the same walker whose trace is the table of its choices, so that it is a DENSITY log q(choices | trace).

Every model here is linear-Gaussian once its discrete choices are fixed (kind 120: a Gaussian truncated to a box), so its exact
posterior is a finite mixture of Gaussians: per configuration the log-joint is a quadratic form in the continuous latents, read off
the statement exactly (second differences of a quadratic are exact), which gives the marginal likelihood, the conditional mean and the
Cholesky factor with no MCMC.  `sample` plants exact posterior draws; `whiten` maps draws back to i.i.d. N(0, 1) coordinates.

The checks at the bottom take an engine adapter (`Engine`: the checker's tries, the product's handlers on the host, the device) and
are called from tests/test_mh_laws.py (CPU) and tests/test_gpu_mh_laws.py (GPU).  No test functions here.

Statistical convention of these checks: chains are independent, so every test is an i.i.d. test with a closed-form critical value
at level ALPHA = 1e-7 per assertion; no tolerance is tuned to an output.  Seeds are fixed.
"""
import itertools
import math

import mpmath
import numpy as np
from scipy import stats

LD = np.longdouble
U = 2.0 ** -52            # one ulp of 1.0: every rounding (2^-53 relative) and every "< 1 ulp" function is counted as one U
MP_BITS = 160
ALPHA = 1e-7
Z_CRIT = float(stats.norm.isf(ALPHA / 2))     # 5.327: two-sided normal critical value at ALPHA
MIN_CELL = 4096           # a configuration's own moment tests need the normal approximation of a product's mean: n >= 4096 keeps the
                          # Edgeworth correction of the 5.3 sigma tail (excess kurtosis 6 / 24 * He4(5.3) / n) under 5 %
MIN_EXPECT = 100          # cells of the configuration chi-square are pooled up to this expectation: at level 1e-7 the chi-square tail needs
                          # near-normal cells (skewness 1/sqrt(E) = 0.1), far above the textbook 5
_PI = LD(4) * np.arctan(LD(1))
LN_2PI = np.log(LD(2) * _PI)

# Roundings in one normal log-density -(z*z + ln 2pi)/2 - ln sd, z = (x - mu)/sd, as tests/model_laws.py counts them: x - mu (1), the
# division (1): z has two, z*z carries them twice (4) and adds its own (1); + ln 2pi (1); ln 2pi an mp_log value, < 1 ulp (tests/test_math.py)
# (1); the halving is exact; - ln sd (1); ln sd an mp_log value (1).  Total 9, relative to the sum of the magnitudes of the terms.
K_NORMAL = 9
# bernoulli: ln p or ln(1 - p): the subtraction's rounding is at most 2^-53 ABSOLUTE in the logarithm's argument <= 1 ... / (1 - p) <= 2 U for
# p <= 1/2 and the proposals' 0.95; the logarithm itself < 1 ulp: 2 U + U |lp|, counted as K_BERN (1 + |lp|)
K_BERN = 2
# uniform_2d: -ln((xmax - xmin)(ymax - ymin)): two differences and a product (3), the logarithm (1): the first three are relative errors of
# the argument, i.e. absolute errors of the logarithm: K_UNIF (1 + |lp|)
K_UNIF = 4


class LawError(AssertionError):
    pass


def bit(p, site):
    return ((np.asarray(p, dtype=np.uint64) >> np.uint64(site)) & np.uint64(1)).astype(bool)


def bits_of(sites):
    b = 0
    for s in sites:
        b |= 1 << int(s)
    return b


class _Walk:
    """One pass through a body, in order.  Modes:
       score  (rng None, strict)   the log-density of every site of the trace (v, p); a site a branch must hold and the trace lacks, or the
                                   reverse, is a LawError
       visit  (rng None, lax)      the same without the presence check: `new` is the presence word the values demand
       redraw (rng given)          sites in `mask`, and sites the new values demand that the trace lacks, are drawn from their stated
                                   distribution given what precedes them; the others keep their value
    lp[:, site]: log-densities (vector sites: at their first slot); tol: the rounding allowance of the engines' float64 evaluation, counted
    term by term; mag: sum of |lp|; nterm: how many terms a sum of the trace's log-densities has."""

    def __init__(self, n_sites, v, p, rng=None, mask=0, strict=True, mp=False, dt=LD):
        self.dt = dt      # long double; float64 where only a statistic is wanted (2^20 chains)
        self.v = np.array(v, dtype=np.float64, copy=True)
        self.n, self.ns = self.v.shape[0], n_sites
        self.old = np.array(p, dtype=np.uint64, copy=True)
        self.new = np.zeros(self.n, dtype=np.uint64)
        self.rng, self.mask, self.strict, self.mp = rng, int(mask), strict, mp
        self.lp = self.zeros((self.n, n_sites))
        self.data_lp = self.zeros(self.n)          # declared data sites (kind 105): observations that are not slots of the trace
        self.tol = np.zeros(self.n, dtype=LD)
        self.mag = np.zeros(self.n, dtype=LD)
        self.nterm = np.zeros(self.n, dtype=np.int64)

    # ---- arithmetic: long double, or mpmath numbers in object arrays ----
    def zeros(self, shape):
        if self.mp:
            z = np.empty(shape, dtype=object)
            z[...] = mpmath.mpf(0)
            return z
        return np.zeros(shape, dtype=self.dt)

    def num(self, a):
        a = np.asarray(a)
        if a.dtype == object:
            return a
        if self.mp:
            return np.array([mpmath.mpf(float(x)) for x in a.ravel()], dtype=object).reshape(a.shape)
        return a.astype(self.dt)

    def const(self, c):
        return mpmath.mpf(float(c)) if self.mp else self.dt(float(c))

    def ln(self, c):
        """the logarithm of a float64 constant or array"""
        if np.ndim(c) == 0:
            return mpmath.log(mpmath.mpf(float(c))) if self.mp else np.log(self.dt(float(c)))
        if self.mp:
            return np.array([mpmath.log(mpmath.mpf(float(x))) for x in c], dtype=object)
        return np.log(np.asarray(c).astype(self.dt))

    def _f(self, a):
        return np.array([float(x) for x in a], dtype=np.float64) if self.mp else np.asarray(a, dtype=np.float64)

    def _absf(self, a):
        return np.abs(np.array([float(x) for x in a], dtype=np.float64)).astype(LD) if self.mp else np.abs(a)

    def val(self, site):
        return self.num(self.v[:, site])

    def has(self, site):
        return bit(self.old, site)

    # ---- bookkeeping ----
    def _site(self, site, when, width=1):
        """which chains draw this site now (redraw mode); the presence check (score mode)"""
        when = np.ones(self.n, dtype=bool) if when is None else np.asarray(when, dtype=bool)
        have = self.has(site)
        for j in range(width):
            self.new[when] |= np.uint64(1 << (site + j))
        if self.rng is None:
            if self.strict and not np.array_equal(have, when):
                raise LawError(f"site {site}: present in {int(have.sum())} chains, the branch holds it in {int(when.sum())}")
            if not self.strict and np.any(when & ~have):
                raise LawError(f"site {site}: demanded by the values and absent")
            return when, np.zeros(self.n, dtype=bool)
        return when, when & (~have | bool((self.mask >> site) & 1))

    def _mean(self, terms):
        """a mean given as a sum of products, [(f, f, ..), ..]: value, and the rounding allowance of its float64 evaluation:
        (multiplications + additions) roundings, each at most U times the sum of the magnitudes of the terms"""
        if not isinstance(terms, list):
            terms = [(terms,)]
        tot, mag, k = self.zeros(self.n), np.zeros(self.n, dtype=LD), len(terms) - 1
        for t in terms:
            prod = self.zeros(self.n) + self.const(1)
            for f in t:
                prod = prod * (self.num(np.broadcast_to(f, (self.n,))) if np.ndim(f) or isinstance(f, np.ndarray) else self.const(f))
            k += len(t) - 1
            tot = tot + prod
            mag = mag + self._absf(prod)
        return tot, k * U * mag

    def _put(self, site, when, lp, tol):
        if site is None:
            self.data_lp = self.data_lp + lp
        else:
            self.lp[when, site] = lp[when]
        a = self._absf(lp)
        a = np.where(np.isfinite(a), a, 0)        # (a point outside its box: -inf exactly, no rounding to allow for)
        self.tol[when] += tol[when]
        self.mag[when] += a[when]
        self.nterm[when] += 1

    def _normal_lp(self, x, mu, mu_err, sd):
        sd_c = self.const(sd)
        z = (x - mu) / sd_c
        ln_sd = self.ln(sd)
        lp = -(z * z + (mpmath.log(2 * mpmath.pi) if self.mp else LN_2PI)) / 2 - ln_sd
        az = self._absf(z)
        M = az * az / 2 + LN_2PI / 2 + abs(LD(float(ln_sd)))
        return lp, K_NORMAL * U * M + az / LD(sd) * mu_err     # (d lp / d mu = z / sd)

    # ---- the distributions a body may name ----
    def normal(self, site, mean, sd, when=None):
        when, draw = self._site(site, when)
        mu, mu_err = self._mean(mean)
        if draw.any():
            self.v[draw, site] = (self._f(mu) + sd * self.rng.standard_normal(self.n))[draw]
        x = self.val(site)
        lp, tol = self._normal_lp(x, mu, mu_err, sd)
        self._put(site, when, lp, tol)
        out = self.zeros(self.n)
        out[when] = x[when]
        return out

    def observe(self, site, y, mean, sd):
        """a normal site whose value is the datum y: a slot of the trace (site) or a declared data site (site None)"""
        mu, mu_err = self._mean(mean)
        when = np.ones(self.n, dtype=bool)
        if site is not None:
            if self.rng is None and self.strict and not (self.has(site).all() and np.all(self.v[:, site] == y)):
                raise LawError(f"observation site {site} does not hold its datum")
            if (self.mask >> site) & 1:
                raise LawError("an observation is never masked here")
            self.v[:, site] = y
            self.new |= np.uint64(1 << site)
        lp, tol = self._normal_lp(self.num(np.full(self.n, y)), mu, mu_err, sd)
        self._put(site, when, lp, tol)

    def bernoulli(self, site, prob, when=None):
        when, draw = self._site(site, when)
        prob = np.broadcast_to(np.asarray(prob, dtype=np.float64), (self.n,))
        if draw.any():
            self.v[draw, site] = (self.rng.random(self.n) < prob)[draw].astype(np.float64)
        b = (self.v[:, site] != 0.0) & when
        one = self.const(1)
        lp = np.where(b, self.ln(prob), self.ln_1m(prob, one))
        self._put(site, when, lp, K_BERN * U * (1 + self._absf(lp)))
        return b

    def ln_1m(self, prob, one):
        if self.mp:
            return np.array([mpmath.log(one - mpmath.mpf(float(q))) for q in prob], dtype=object)
        return np.log(one - prob.astype(self.dt))

    def uniform_2d(self, site, box):
        """both coordinates of a point uniform on [xmin, xmax] x [ymin, ymax]: slots site, site + 1"""
        when, draw = self._site(site, None, width=2)
        xmin, xmax, ymin, ymax = (float(b) for b in box)
        if draw.any():
            self.v[draw, site] = (self.rng.random(self.n) * (xmax - xmin) + xmin)[draw]
            self.v[draw, site + 1] = (self.rng.random(self.n) * (ymax - ymin) + ymin)[draw]
        x, y = self.v[:, site], self.v[:, site + 1]
        inside = (xmin <= x) & (x <= xmax) & (ymin <= y) & (y <= ymax)
        area = (self.const(xmax) - self.const(xmin)) * (self.const(ymax) - self.const(ymin))
        neg_ln_area = -(mpmath.log(area) if self.mp else np.log(area))
        lp = self.zeros(self.n) + neg_ln_area
        if not self.mp:
            lp[~inside] = -np.inf
        elif not inside.all():
            raise LawError("mpmath spot check outside the box")
        self._put(site, when, lp, K_UNIF * U * (1 + abs(LD(float(neg_ln_area)))) + np.zeros(self.n, dtype=LD))   # (outside: -inf, exactly)
        return self.val(site), self.val(site + 1)

    def mvnormal2(self, site, mean, cov, datum=None):
        """a bivariate normal at slots site, site + 1: -(d' inv(cov) d + ln det cov + 2 ln 2pi) / 2; datum: an observed value.
        Roundings, relative to the sum M of the magnitudes of the four products, |ln det| / 2 and ln 2pi: the inverse's entries carry the
        determinant's three roundings amplified by amp = (|c00 c11| + |c01 c10|) / det, a division and a sign (3 amp + 1); each product
        d_i inv_ij d_j adds two for the differences and two for the multiplications; three additions, the sum with ln det and 2 ln 2pi
        (2), ln det (det's 3 amp, the logarithm 1: absolute).  K_MVN = 12 + 8 amp covers them with a factor 2 to spare."""
        when, draw = self._site(site, None, width=2)
        c = [float(q) for q in np.asarray(cov, dtype=np.float64).reshape(4)]
        c00, c01, c10, c11 = (self.const(q) for q in c)
        det = c00 * c11 - c01 * c10
        amp = (abs(c[0] * c[3]) + abs(c[1] * c[2])) / float(det)
        mu0, e0 = self._mean(mean[0])
        mu1, e1 = self._mean(mean[1])
        if datum is not None:
            if self.rng is None and self.strict and not (self.has(site).all() and np.all(self.v[:, site] == datum[0]) and np.all(self.v[:, site + 1] == datum[1])):
                raise LawError("observation site does not hold its datum")
            self.v[:, site], self.v[:, site + 1] = datum[0], datum[1]
        elif draw.any():
            l00 = math.sqrt(c[0])
            l10 = c[2] / l00
            l11 = math.sqrt(c[3] - l10 * l10)
            z0, z1 = self.rng.standard_normal(self.n), self.rng.standard_normal(self.n)
            self.v[draw, site] = (self._f(mu0) + l00 * z0)[draw]
            self.v[draw, site + 1] = (self._f(mu1) + l10 * z0 + l11 * z1)[draw]
        d0, d1 = self.val(site) - mu0, self.val(site + 1) - mu1
        i00, i01, i10, i11 = c11 / det, -c01 / det, -c10 / det, c00 / det
        q = [d0 * i00 * d0, d0 * i01 * d1, d1 * i10 * d0, d1 * i11 * d1]
        ln_det = mpmath.log(det) if self.mp else np.log(det)
        lp = -(q[0] + q[1] + q[2] + q[3] + ln_det + 2 * (mpmath.log(2 * mpmath.pi) if self.mp else LN_2PI)) / 2
        M = sum(self._absf(t) for t in q) / 2 + abs(LD(float(ln_det))) / 2 + LN_2PI
        # (an error e_i of a mean moves the quadratic form by |d lp / d mu_i| e_i = |(inv d)_i| e_i)
        g0, g1 = self._absf(i00 * d0 + i01 * d1), self._absf(i10 * d0 + i11 * d1)
        self._put(site, when, lp, (12 + 8 * amp) * U * M + g0 * e0 + g1 * e1)
        return self.val(site), self.val(site + 1)

    # ---- results ----
    def stale(self):
        return self.old & ~self.new

    def finish(self):
        if self.rng is None and self.strict and np.any(self.stale()):
            raise LawError("the trace holds sites its branch does not")
        absent = ~self.new
        for k in range(self.ns):
            self.v[bit(absent, k), k] = 0.0
        return self

    def total(self):
        """the trace's log-joint: its sites' log-densities, then the declared data sites'"""
        t = self.zeros(self.n)
        for k in range(self.ns):
            t = t + self.lp[:, k]
        return t + self.data_lp

    def total_tol(self):
        """each term's own allowance, plus nterm - 1 additions each rounding a partial sum of magnitude <= mag"""
        return self.tol + np.maximum(self.nterm - 1, 0) * U * self.mag


class _TraceView:
    """what a proposal's body reads of the trace it is applied to"""

    def __init__(self, w, v, p):
        self.w, self.v, self.p = w, np.asarray(v, dtype=np.float64), np.asarray(p, dtype=np.uint64)

    def val(self, site):
        return self.w.num(self.v[:, site])

    def flag(self, site):
        return self.v[:, site] != 0.0

    def has(self, site):
        return bit(self.p, site)

    def get(self, site, dflt):
        return self.w.num(np.where(self.has(site), self.v[:, site], dflt))


# =========================================================================================================================
# Cholesky in long double (d <= 5)
# =========================================================================================================================
def _chol(A):
    d = A.shape[0]
    C = np.zeros((d, d), dtype=LD)
    for i in range(d):
        for j in range(i + 1):
            s = A[i, j] - sum((C[i, k] * C[j, k] for k in range(j)), LD(0))
            if i == j:
                if not s > 0:
                    raise LawError("precision matrix not positive definite")
                C[i, i] = np.sqrt(s)
            else:
                C[i, j] = s / C[j, j]
    return C


def _fwd(C, b):
    """solve C y = b; b [.., d]"""
    d = C.shape[0]
    y = np.zeros(b.shape, dtype=LD)
    for i in range(d):
        y[..., i] = (b[..., i] - sum((C[i, k] * y[..., k] for k in range(i)), LD(0))) / C[i, i]
    return y


def _bwd(C, b):
    """solve C' x = b"""
    d = C.shape[0]
    x = np.zeros(b.shape, dtype=LD)
    for i in reversed(range(d)):
        x[..., i] = (b[..., i] - sum((C[k, i] * x[..., k] for k in range(i + 1, d)), LD(0))) / C[i, i]
    return x


class Config:
    """(a plain record) one setting of a model's discrete choices: prior mass, which continuous latents exist, and the Gaussian the log-joint is in them:
    ln p(z, cfg, y) = c + b'z - z'Az/2, A = C C' (Cholesky);  mean = A^-1 b;  ln p(cfg, y) = c + b'mean/2 + (d/2) ln 2pi - sum ln C_ii;
    a draw is mean + C'^-1 eps;  eps = C'(z - mean) whitens it."""


# =========================================================================================================================
# Laws
# =========================================================================================================================
class Law:
    kind = None
    discrete = ()          # sites holding a bool
    box = None

    def body(self, w):
        raise NotImplementedError

    # ---- the statement ----
    def walk(self, v, p, **kw):
        w = _Walk(self.ns, v, p, **kw)
        self.body(w)
        return w.finish()

    def logjoint(self, values, present, mp=False, dt=LD):
        """-> (log-joint per chain, the rounding allowance of a float64 evaluation of it); a trace whose sites are not its branch's
        is a LawError"""
        w = self.walk(values, present, mp=mp, dt=dt)
        return w.total(), w.total_tol()

    def structure(self, values, present):
        """the presence word the values demand (what the reference's gc leaves), and the values with the dropped sites zeroed"""
        w = self.walk(values, present, strict=False)
        return w.v, w.new

    def redraw(self, rng, values, present, mask):
        """sites of `mask` (a bit set) redrawn from the model given what precedes them, with whatever the new branch needs and
        lacks; an UNMASKED site the new branch drops is the reference's panic (leftover constraints, dyngenfn.rs:526-529): LawError"""
        w = self.walk(values, present, rng=rng, mask=mask)
        if np.any(w.stale() & ~np.uint64(mask)):
            raise LawError("regen_mh: an unmasked site would be dropped")
        return w.v, w.new

    # ---- the exact posterior ----
    def obs_table(self):
        """observations that are slots of the trace: {site: value}"""
        return self.constraints

    def _template(self, cfg, n):
        v = np.zeros((n, self.ns))
        p = bits_of(self.obs_table())
        for s, y in self.obs_table().items():
            v[:, s] = y
        for s, b in zip(self.discrete, cfg):
            v[:, s] = float(b)
            p |= 1 << s
        return v, np.full(n, p, dtype=np.uint64)

    def configs(self):
        if getattr(self, "_configs", None) is not None:
            return self._configs
        out = []
        for cfg in itertools.product((0, 1), repeat=len(self.discrete)):
            c = Config()
            c.cfg = cfg
            v0, p0 = self._template(cfg, 1)
            w = self.walk(v0, p0, rng=np.random.default_rng(0), mask=0)      # (only to learn which sites the branch holds)
            c.present = int(w.new[0])
            c.cont = [k for k in range(self.ns) if (c.present >> k) & 1 and k not in self.discrete and k not in self.obs_table()]
            d = len(c.cont)
            # the quadratic form, from 1 + d + d (d + 1) / 2 evaluations of the statement: 0, e_i, e_i + e_j (i <= j)
            pts = [np.zeros(d)] + [np.eye(d)[i] for i in range(d)] + [np.eye(d)[i] + np.eye(d)[j] for i in range(d) for j in range(i, d)]
            v, p = self._template(cfg, len(pts))
            p[:] = c.present
            v[:, c.cont] = np.array(pts)
            f, _ = self.logjoint(v, p)
            c.prior = float(np.exp(sum((self.walk(v[:1], p[:1]).lp[0, s] for s in self.discrete), LD(0))))
            f0, fe = f[0], f[1:1 + d]
            A = np.zeros((d, d), dtype=LD)
            q = 1 + d
            for i in range(d):
                for j in range(i, d):
                    if i == j:
                        A[i, i] = -(f[q] - 2 * fe[i] + f0)
                    else:
                        A[i, j] = A[j, i] = -(f[q] - fe[i] - fe[j] + f0)
                    q += 1
            c.A = A
            c.b = np.array([fe[i] - f0 + A[i, i] / 2 for i in range(d)], dtype=LD)
            c.C = _chol(A)
            c.mean = _bwd(c.C, _fwd(c.C, c.b))
            c.log_z = f0 + np.dot(c.b, c.mean) / 2 + d * LN_2PI / 2 - np.sum(np.log(np.diag(c.C)))
            out.append(c)
        lz = np.array([c.log_z for c in out], dtype=LD)
        self.log_evidence = lz.max() + np.log(np.sum(np.exp(lz - lz.max())))
        for c in out:
            c.post = float(np.exp(c.log_z - self.log_evidence))
        self._configs = out
        return out

    def config_index(self, values):
        idx = np.zeros(values.shape[0], dtype=np.int64)
        for s in self.discrete:
            idx = idx * 2 + (values[:, s] != 0.0)
        return idx

    def sample(self, rng, n):
        """n exact posterior draws -> (values, present)"""
        cs = self.configs()
        which = rng.choice(len(cs), size=n, p=np.array([c.post for c in cs]) / sum(c.post for c in cs))
        v, p = np.zeros((n, self.ns)), np.zeros(n, dtype=np.uint64)
        for k, c in enumerate(cs):
            sel = np.flatnonzero(which == k)
            if sel.size == 0:
                continue
            tv, tp = self._template(c.cfg, sel.size)
            eps = rng.standard_normal((sel.size, len(c.cont))).astype(LD)
            tv[:, c.cont] = (c.mean + _bwd(c.C, eps)).astype(np.float64)
            v[sel], p[sel] = tv, c.present
        return v, p

    def whiten(self, values, k):
        """the continuous latents of chains in configuration k -> coordinates that are i.i.d. N(0, 1) under the exact posterior"""
        c = self.configs()[k]
        return ((values[:, c.cont].astype(LD) - c.mean) @ c.C).astype(np.float64)

    def prior_sample(self, rng, n):
        v, p = self._template((0,) * len(self.discrete), n)
        w = self.walk(v, p & np.uint64(bits_of(self.obs_table())), rng=rng, mask=0)
        return w.v, w.new


def _obs_dict(y0, ys):
    return {y0 + k: float(y) for k, y in enumerate(ys)}


class Hierarchical(Law):
    """hierarchical.rs:17-47 / mp_mh_models.h kind 101:  is_linear ~ bernoulli(0.7);  coeffs: a, b ~ normal(0, 1), and c ~ normal(0, 1)
    in the quadratic branch only;  y_k ~ normal(a + b x_k [+ c x_k^2], 0.1).  Sites: 0 is_linear, 1 a, 2 b, 3 c, 4 + k y_k.
    A linear trace holds no c."""
    kind, name, ns, discrete = 101, "hier", 20, (0,)
    IS_LINEAR, A, B, C, Y0 = 0, 1, 2, 3, 4
    XS = np.array([-1.0, -0.5, 0.0, 0.5, 1.0])
    CURV = 0.2       # P(quadratic | y) = 0.16 (tests/test_mh_laws.py test_input_conditions asserts >= 0.1)
    NOISE = np.array([0.3, -0.5, 0.2, 0.6, -0.4])

    def __init__(self):
        self.xs = self.XS
        self.ys = 0.3 + 0.4 * self.xs + self.CURV * self.xs ** 2 + 0.1 * self.NOISE
        self.params = self.xs
        self.constraints = _obs_dict(self.Y0, self.ys)

    def latents(self, w):
        lin = w.bernoulli(self.IS_LINEAR, 0.7)
        a = w.normal(self.A, 0.0, 1.0)
        b = w.normal(self.B, 0.0, 1.0)
        c = w.normal(self.C, 0.0, 1.0, when=~lin)
        return a, b, c

    def body(self, w):
        a, b, c = self.latents(w)
        for k, (x, y) in enumerate(zip(self.xs, self.ys)):
            w.observe(self.Y0 + k, y, [(a,), (b, x), (c, x, x)], 0.1)    # (c is 0 where the branch is linear)


class HierarchicalData(Hierarchical):
    """kind 105: the same model whose observations are declared data sites: four slots of trace, any number of observations (200 here);
    across the C ABI observation j is the constraint on site id 4 + j of the creating call."""
    kind, name, ns = 105, "hier_data", 4
    CURV = 0.11      # P(quadratic | y) = 0.39; x in [-0.7, 0.7] leaves c a posterior wide enough for the joint mask {is_linear, c} to cross

    def __init__(self):
        n = 200
        self.xs = np.linspace(-0.7, 0.7, n)
        noise = np.random.default_rng(105).standard_normal(n)
        self.ys = 0.3 + 0.4 * self.xs + self.CURV * self.xs ** 2 + 0.1 * noise
        self.params = self.xs
        self.constraints = _obs_dict(4, self.ys)

    def obs_table(self):
        return {}

    def body(self, w):
        a, b, c = self.latents(w)
        if w.mp:
            for x, y in zip(self.xs, self.ys):
                w.observe(None, y, [(a,), (b, x), (c, x, x)], 0.1)
            return
        # the same 200 terms as one [chains, observations] array
        x = self.xs.astype(w.dt)[None, :]
        t = [np.broadcast_to(a[:, None], (w.n, x.shape[1])), b[:, None] * x, c[:, None] * x * x]
        mu_err = 5 * U * (np.abs(t[0]) + np.abs(t[1]) + np.abs(t[2]))          # three multiplications, two additions, as _Walk._mean counts them
        lp, tol = w._normal_lp(self.ys.astype(w.dt)[None, :], t[0] + t[1] + t[2], mu_err, 0.1)
        w.data_lp = w.data_lp + lp.sum(axis=1)
        w.tol += tol.sum(axis=1)
        w.mag += np.abs(lp).sum(axis=1)
        w.nterm += x.shape[1]


class RobustLine(Law):
    """kind 102:  slope, intercept ~ normal(0, 2);  per point k: is_outlier_k ~ bernoulli(0.1),  y_k ~ normal(slope x_k + intercept,
    is_outlier_k ? 5 : 0.5).  Sites: 0 slope, 1 intercept, 2 + k is_outlier_k (12 slots), 14 + k y_k."""
    kind, name, ns = 102, "robust", 26
    SLOPE, INTERCEPT, OUT0, Y0 = 0, 1, 2, 14

    def __init__(self):
        self.xs = np.array([-2.5, -1.5, -0.5, 0.5, 1.5, 2.5])
        self.ys = 0.8 * self.xs - 0.3 + 0.85 * np.array([1.0, -1.0, -1.0, 1.0, 1.0, -1.0])
        self.params = self.xs
        self.discrete = tuple(self.OUT0 + k for k in range(self.xs.size))
        self.constraints = _obs_dict(self.Y0, self.ys)

    def body(self, w):
        slope = w.normal(self.SLOPE, 0.0, 2.0)
        icpt = w.normal(self.INTERCEPT, 0.0, 2.0)
        for k, (x, y) in enumerate(zip(self.xs, self.ys)):
            out = w.bernoulli(self.OUT0 + k, 0.1)
            _observe_two_sds(w, self.Y0 + k, y, [(slope, x), (icpt,)], out, 5.0, 0.5)


def _observe_two_sds(w, site, y, mean, flag, sd_true, sd_false):
    """y ~ normal(mean, flag ? sd_true : sd_false): the two densities, each where it applies"""
    mu, mu_err = w._mean(mean)
    if site is not None:
        if w.rng is None and w.strict and not (w.has(site).all() and np.all(w.v[:, site] == y)):
            raise LawError(f"observation site {site} does not hold its datum")
        w.v[:, site] = y
        w.new |= np.uint64(1 << site)
    yy = w.num(np.full(w.n, y))
    lt, tt = w._normal_lp(yy, mu, mu_err, sd_true)
    lf, tf = w._normal_lp(yy, mu, mu_err, sd_false)
    w._put(site, np.ones(w.n, dtype=bool), np.where(flag, lt, lf), np.where(flag, tt, tf))


class ScaledLine(Law):
    """kind 103:  big ~ bernoulli(0.3);  slope, intercept ~ normal(0, 2);  y_k ~ normal(slope x_k + intercept, big ? 2 : 0.5).
    Sites: 0 big, 1 slope, 2 intercept, 3 + k y_k."""
    kind, name, ns, discrete = 103, "scaled", 13, (0,)
    BIG, SLOPE, INTERCEPT, Y0 = 0, 1, 2, 3

    def __init__(self):
        self.xs = np.linspace(-1.0, 3.0, 7)
        self.ys = 1.2 * self.xs + 0.4 + np.array([1.1, -0.9, 0.4, -1.3, 1.0, 0.2, -0.8])
        self.params = self.xs
        self.constraints = _obs_dict(self.Y0, self.ys)

    def body(self, w):
        big = w.bernoulli(self.BIG, 0.3)
        slope = w.normal(self.SLOPE, 0.0, 2.0)
        icpt = w.normal(self.INTERCEPT, 0.0, 2.0)
        for k, (x, y) in enumerate(zip(self.xs, self.ys)):
            _observe_two_sds(w, self.Y0 + k, y, [(slope, x), (icpt,)], big, 2.0, 0.5)


class Nested(Law):
    """kind 113:  a ~ normal(0, 2);  b ~ normal(a, 1);  c ~ normal(b, 0.5);  f ~ bernoulli(0.3);  d ~ normal(c, 1) under f only;
    e ~ normal(c + b + (f ? d : 0), 0.7);  y_j ~ normal(e x_j, 0.3).  Sites: 0 a, 1 b, 2 c, 3 f, 4 d, 5 e, 6 + j y_j.  Without f, no d."""
    kind, name, ns, discrete = 113, "nested", 10, (3,)
    A, B, C, F, D, E, Y0 = 0, 1, 2, 3, 4, 5, 6

    def __init__(self):
        self.xs = np.array([0.5, -0.4, 0.3])
        self.ys = 1.6 * self.xs + np.array([0.2, 0.25, -0.3])
        self.params = self.xs
        self.constraints = _obs_dict(self.Y0, self.ys)

    def body(self, w):
        a = w.normal(self.A, 0.0, 2.0)
        b = w.normal(self.B, a, 1.0)
        c = w.normal(self.C, b, 0.5)
        f = w.bernoulli(self.F, 0.3)
        d = w.normal(self.D, c, 1.0, when=f)
        e = w.normal(self.E, [(c,), (b,), (d,)], 0.7)
        for j, (x, y) in enumerate(zip(self.xs, self.ys)):
            w.observe(self.Y0 + j, y, [(e, x)], 0.3)


class Wide(Law):
    """kind 114:  slope, intercept ~ normal(0, 2);  big ~ bernoulli(0.3);  y_j ~ normal(slope x_j + intercept, big ? 2 : 0.5), j < 30;
    o1 ~ normal(0, 1);  o2 ~ normal(o1, 1) under big only;  z_k ~ normal(o1 + (big ? o2 : 0) + 0.1 k, 0.5), k < 6.
    Sites: 0 slope, 1 intercept, 2 big, 3 + j y_j, 33 o1, 34 o2, 35 + k z_k.  Without big, no o2."""
    kind, name, ns, discrete = 114, "wide", 41, (2,)
    SLOPE, INTERCEPT, BIG, Y0, O1, O2, Z0 = 0, 1, 2, 3, 33, 34, 35

    def __init__(self):
        r = np.random.default_rng(114)
        self.xs = np.linspace(-2.0, 2.0, 30)
        self.ys = 0.7 * self.xs - 0.2 + 1.05 * r.standard_normal(30)
        self.zs = 0.4 + 0.1 * np.arange(6) + 0.5 * r.standard_normal(6)
        self.params = self.xs
        self.constraints = {**_obs_dict(self.Y0, self.ys), **_obs_dict(self.Z0, self.zs)}

    def body(self, w):
        slope = w.normal(self.SLOPE, 0.0, 2.0)
        icpt = w.normal(self.INTERCEPT, 0.0, 2.0)
        big = w.bernoulli(self.BIG, 0.3)
        for j, (x, y) in enumerate(zip(self.xs, self.ys)):
            _observe_two_sds(w, self.Y0 + j, y, [(slope, x), (icpt,)], big, 2.0, 0.5)
        o1 = w.normal(self.O1, 0.0, 1.0)
        o2 = w.normal(self.O2, o1, 1.0, when=big)
        for k, z in enumerate(self.zs):
            w.observe(self.Z0 + k, z, [(o1,), (o2,), (0.1, float(k))], 0.5)


class Pointed(Law):
    """simple.rs:27-34 / kind 120:  latent ~ uniform on the box;  obs ~ mvnormal(latent, cov).  Slots: 1, 2 latent; 3, 4 obs.
    The posterior is N(obs, cov) truncated to the box."""
    kind, name, ns, discrete = 120, "pointed", 5, ()
    LATENT, OBS = 1, 3

    def __init__(self):
        self.box = (-5.0, 5.0, -5.0, 5.0)
        self.cov = np.array([[1.0, -0.6], [-0.6, 2.0]])
        self.obs = np.array([4.3, -3.9])
        self.params = np.concatenate([self.box, self.cov.ravel()])
        self.constraints = {3: float(self.obs[0]), 4: float(self.obs[1])}

    def body(self, w):
        x, y = w.uniform_2d(self.LATENT, self.box)
        w.mvnormal2(self.OBS, (x, y), self.cov, datum=self.obs)

    # ---- exact posterior: one configuration, not Gaussian ----
    def _cond(self):
        s1, s2 = math.sqrt(self.cov[0, 0]), math.sqrt(self.cov[1, 1])
        rho = self.cov[0, 1] / (s1 * s2)
        return s1, s2, rho, s2 * math.sqrt(1 - rho * rho)

    def _x_marginal(self):
        """the x-marginal of the truncated law on a grid: phi((x - o1)/s1)/s1 (Phi(hi(x)) - Phi(lo(x))), the inner integral exact;
        Simpson's rule over 2^16 intervals (h = 1.5e-4: error ~ h^4 max|f''''| / 180 < 1e-13) gives the box mass"""
        if getattr(self, "_grid", None) is None:
            s1, s2, rho, sc = self._cond()
            xmin, xmax, ymin, ymax = self.box
            x = np.linspace(xmin, xmax, (1 << 16) + 1)
            m = self.obs[1] + rho * s2 / s1 * (x - self.obs[0])
            g = stats.norm.pdf((x - self.obs[0]) / s1) / s1 * (stats.norm.cdf((ymax - m) / sc) - stats.norm.cdf((ymin - m) / sc))
            h = x[1] - x[0]
            # cumulative Simpson at the even nodes
            seg = h / 3 * (g[0:-2:2] + 4 * g[1:-1:2] + g[2::2])
            self._grid = (x[::2], np.concatenate([[0.0], np.cumsum(seg)]), g[::2])
            self.box_mass = float(self._grid[1][-1])
        return self._grid

    def configs(self):
        if getattr(self, "_configs", None) is None:
            c = Config()
            c.cfg, c.prior, c.post, c.cont = (), 1.0, 1.0, [1, 2]
            c.present = 0b11110
            self._x_marginal()
            self._configs = [c]
        return self._configs

    def sample(self, rng, n):
        """rejection from N(obs, cov)"""
        L = np.linalg.cholesky(self.cov)
        xmin, xmax, ymin, ymax = self.box
        got = np.zeros((0, 2))
        while got.shape[0] < n:
            z = self.obs + rng.standard_normal((2 * n + 1024, 2)) @ L.T
            z = z[(z[:, 0] >= xmin) & (z[:, 0] <= xmax) & (z[:, 1] >= ymin) & (z[:, 1] <= ymax)]
            got = np.concatenate([got, z])
        v = np.zeros((n, 5))
        v[:, 1:3] = got[:n]
        v[:, 3:5] = self.obs
        return v, np.full(n, 0b11110, dtype=np.uint64)

    def whiten(self, values, k=0):
        """Rosenblatt: u1 = G(x), the x-marginal's distribution function (Hermite interpolation of the Simpson nodes: value and slope are
        exact at the nodes, error ~ h^4), u2 = the truncated normal y | x in closed form; then the normal quantile of each"""
        gx, G, g = self._x_marginal()
        s1, s2, rho, sc = self._cond()
        x, y = values[:, 1], values[:, 2]
        h = gx[1] - gx[0]
        i = np.clip(((x - gx[0]) / h).astype(np.int64), 0, gx.size - 2)
        t = (x - gx[i]) / h
        h00, h10, h01, h11 = (1 + 2 * t) * (1 - t) ** 2, t * (1 - t) ** 2, t * t * (3 - 2 * t), t * t * (t - 1)
        u1 = (h00 * G[i] + h10 * h * g[i] + h01 * G[i + 1] + h11 * h * g[i + 1]) / G[-1]
        m = self.obs[1] + rho * s2 / s1 * (x - self.obs[0])
        lo, hi = stats.norm.cdf((self.box[2] - m) / sc), stats.norm.cdf((self.box[3] - m) / sc)
        u2 = (stats.norm.cdf((y - m) / sc) - lo) / (hi - lo)
        return np.stack([stats.norm.ppf(u1), stats.norm.ppf(u2)], axis=1)


# =========================================================================================================================
# Proposals as densities
# =========================================================================================================================
class Proposal:
    """kind, args: what the engines are called with.  body(w, tr): the proposal's prose over a walker whose table is the CHOICES.
    Which old sites fall into the discard is mh.rs:17-27 for every proposal alike: the old value of every site the choices overwrite,
    and every old site the new branch no longer holds (`mh_alpha`)."""

    def __init__(self, law, kind, args, body, name, changes=None):
        self.law, self.kind, self.args, self.body, self.name = law, kind, list(args), body, name
        self.changes = changes       # the discrete site a structure-changing move may flip (None: no structure change)

    def _walk(self, choices, trace, **kw):
        w = _Walk(self.law.ns, choices[0], choices[1], **kw)
        self.body(w, _TraceView(w, trace[0], trace[1]))
        return w.finish()

    def log_q(self, choices, trace, mp=False, dt=LD):
        """ln q(choices | trace) and its rounding allowance; choices that are not the ones the proposal makes from this trace: LawError"""
        w = self._walk(choices, trace, mp=mp, dt=dt)
        return w.total(), w.total_tol()

    def sample(self, rng, trace):
        n = trace[0].shape[0]
        w = self._walk((np.zeros((n, self.law.ns)), np.zeros(n, dtype=np.uint64)), trace, rng=rng)
        return w.v, w.new


def proposals(law):
    H, R, S, N, W = Hierarchical, RobustLine, ScaledLine, Nested, Wide

    def drift(sites, sd):
        def body(w, tr):
            for s in sites:
                w.normal(s, tr.val(s), sd)
        return body

    if law.kind in (101, 105):
        def hier_drift(sd):
            def body(w, tr):          # hierarchical.rs:62-70: a, b, and c where the trace is quadratic
                w.normal(H.A, tr.val(H.A), sd)
                w.normal(H.B, tr.val(H.B), sd)
                w.normal(H.C, tr.val(H.C), sd, when=~tr.flag(H.IS_LINEAR))
            return body

        def add_or_remove(w, tr):     # hierarchical.rs:48-61: a, b at 0.025; is_linear ~ bernoulli(0.5); c ~ normal(the old c or 0, 0.025) when not linear
            w.normal(H.A, tr.val(H.A), 0.025)
            w.normal(H.B, tr.val(H.B), 0.025)
            lin = w.bernoulli(H.IS_LINEAR, 0.5)
            w.normal(H.C, tr.get(H.C, 0.0), 0.025, when=~lin)
        return [Proposal(law, 1, [0.1], hier_drift(0.1), "drift 0.1"), Proposal(law, 1, [0.02], hier_drift(0.02), "drift 0.02"),
                Proposal(law, 2, [], add_or_remove, "add_or_remove", changes=H.IS_LINEAR)]
    if law.kind == 102:
        def flip(k):
            def body(w, tr):          # the other value of is_outlier_k with probability 0.95
                w.bernoulli(R.OUT0 + k, np.where(tr.flag(R.OUT0 + k), 0.05, 0.95))
            return body
        return [Proposal(law, 1, [0.25], drift((R.SLOPE, R.INTERCEPT), 0.25), "drift 0.25")] + \
               [Proposal(law, 2, [float(k)], flip(k), f"flip {k}", changes=R.OUT0 + k) for k in (0, 3, 5)]
    if law.kind == 103:
        def toggle(w, tr):            # the other value of big with probability 0.9
            w.bernoulli(S.BIG, np.where(tr.flag(S.BIG), 0.1, 0.9))
        return [Proposal(law, 1, [], toggle, "toggle", changes=S.BIG), Proposal(law, 2, [0.3], drift((S.SLOPE, S.INTERCEPT), 0.3), "drift 0.3")]
    if law.kind == 113:
        def flip_f(w, tr):            # the other value of f with probability 0.8, and d ~ normal(c, 1) with a true f
            f = w.bernoulli(N.F, np.where(tr.flag(N.F), 0.2, 0.8))
            w.normal(N.D, tr.val(N.C), 1.0, when=f)
        return [Proposal(law, 1, [0.2], drift((N.B, N.C), 0.2), "drift_bc 0.2"), Proposal(law, 2, [], flip_f, "flip", changes=N.F),
                Proposal(law, 3, [0.5], drift((N.A,), 0.5), "drift_a 0.5")]
    if law.kind == 114:
        def toggle_big(w, tr):        # the other value of big with probability 0.8, and o2 ~ normal(o1, 1) with a true big
            big = w.bernoulli(W.BIG, np.where(tr.flag(W.BIG), 0.2, 0.8))
            w.normal(W.O2, tr.val(W.O1), 1.0, when=big)
        return [Proposal(law, 1, [0.1], drift((W.SLOPE, W.INTERCEPT, W.O1), 0.1), "drift 0.1"), Proposal(law, 2, [], toggle_big, "toggle", changes=W.BIG)]
    if law.kind == 120:
        def pointed_drift(noise):
            def body(w, tr):          # simple.rs:36-41: mvnormal(the old latent, noise)
                w.mvnormal2(Pointed.LATENT, (tr.val(1), tr.val(2)), noise)
            return body
        return [Proposal(law, 1, list(np.ravel(nz)), pointed_drift(np.array(nz)), f"drift {i}") for i, nz in enumerate(POINTED_NOISES)]
    raise KeyError(law.kind)


POINTED_NOISES = [[[0.25, 0.0], [0.0, 0.25]], [[1.0, 0.5], [0.5, 2.0]], [[0.04, -0.01], [-0.01, 0.09]]]


def regen_masks(law):
    """(single-site masks, joint structure-changing mask, cycle).  A single-site mask on the discrete choice that decides a later
    site's existence is left out where the move that drops the site is the reference's panic (an unmasked leftover: is_linear of
    kinds 101/105 -- tests/test_gpu_mh.py pins that error --, f of kind 113, big of kind 114): the joint mask covers those moves."""
    H, R, S, N, W = Hierarchical, RobustLine, ScaledLine, Nested, Wide
    return {101: ([[H.A], [H.B], [H.C]], [H.IS_LINEAR, H.C], [H.A, H.B, H.C]),
            105: ([[H.A], [H.B], [H.C]], [H.IS_LINEAR, H.C], [H.A, H.B, H.C]),
            102: ([[R.SLOPE], [R.INTERCEPT], [R.OUT0 + 1], [R.OUT0 + 4]], [R.OUT0 + 2, R.INTERCEPT], [R.SLOPE, R.OUT0 + 3, R.INTERCEPT]),
            103: ([[S.BIG], [S.SLOPE], [S.INTERCEPT]], [S.BIG, S.SLOPE], [S.BIG, S.INTERCEPT, S.SLOPE]),
            113: ([[N.A], [N.B], [N.C], [N.D], [N.E]], [N.F, N.D], [N.A, N.E, N.B, N.C]),
            114: ([[W.SLOPE], [W.INTERCEPT], [W.O1], [W.O2]], [W.BIG, W.O2], [W.O1, W.SLOPE, W.O2]),
            120: ([[Pointed.LATENT]], None, None)}[law.kind]


LAWS = {101: Hierarchical, 105: HierarchicalData, 102: RobustLine, 103: ScaledLine, 113: Nested, 114: Wide, 120: Pointed}
_LAW_CACHE = {}


def make_law(kind):
    if kind not in _LAW_CACHE:
        _LAW_CACHE[kind] = LAWS[kind]()
    return _LAW_CACHE[kind]


# =========================================================================================================================
# mh.rs:9-40 and :54-67 as mathematics
# =========================================================================================================================
def apply_choices(law, old, choices):
    ov, op = old
    cv, cp = choices
    nv = ov.copy()
    for k in range(law.ns):
        sel = bit(cp, k)
        nv[sel, k] = cv[sel, k]
    return law.structure(nv, op | cp)


def mh_alpha(law, prop, old, choices, dt=LD):
    """alpha = ln p(new) - ln p(old) + ln q(discard and overwritten | new) - ln q(choices | old), the textbook ratio.
    -> (alpha, new trace, rounding allowance)"""
    ov, op = old
    cv, cp = choices
    new = apply_choices(law, old, choices)
    back = (ov, (cp & op) | (op & ~new[1]))         # the old values of what was overwritten, and of what the new branch dropped
    l_new, t1 = law.logjoint(*new, dt=dt)
    l_old, t2 = law.logjoint(ov, op, dt=dt)
    fwd, t3 = prop.log_q(choices, old, dt=dt)
    bwd, t4 = prop.log_q(back, new, dt=dt)
    return l_new - l_old + bwd - fwd, new, t1 + t2 + t3 + t4


def mh_move(law, prop, rng, old, dt=LD):
    """one mh move of the numpy kernel -> (trace, accepted)"""
    choices = prop.sample(rng, old)
    alpha, new, _ = mh_alpha(law, prop, old, choices, dt=dt)
    acc = np.log(rng.random(old[0].shape[0])) < alpha
    v, p = old[0].copy(), old[1].copy()
    v[acc], p[acc] = new[0][acc], new[1][acc]
    return (v, p), acc


def regen_alpha(law, old, new, mask, dt=LD):
    """regen_mh as a kernel: the masked sites, and whatever the new branch needs and lacks, are redrawn from the model given the rest;
    q(new | old) is the product of the stated densities of the freshly drawn sites, the reverse move draws the old values of the
    masked sites and of the sites the new branch dropped; alpha = ln p(new) - ln p(old) + ln q(old | new) - ln q(new | old)."""
    m = np.uint64(mask)
    wo, wn = law.walk(*old, dt=dt), law.walk(*new, dt=dt)
    fresh_new, fresh_old = new[1] & (m | ~old[1]), old[1] & (m | ~new[1])
    qf, qb = np.zeros(old[0].shape[0], dtype=dt), np.zeros(old[0].shape[0], dtype=dt)
    for k in range(law.ns):
        qf += np.where(bit(fresh_new, k), wn.lp[:, k], 0)
        qb += np.where(bit(fresh_old, k), wo.lp[:, k], 0)
    return wn.total() - wo.total() + qb - qf


def regen_move(law, rng, old, mask_sites, dt=LD):
    mask = bits_of(mask_sites)
    new = law.redraw(rng, old[0], old[1], mask)
    alpha = regen_alpha(law, old, new, mask, dt=dt)
    acc = np.log(rng.random(old[0].shape[0])) < alpha
    v, p = old[0].copy(), old[1].copy()
    v[acc], p[acc] = new[0][acc], new[1][acc]
    return (v, p), acc


# =========================================================================================================================
# Engines
# =========================================================================================================================
class Engine:
    """which: "tries" (the checker's dynamic machinery), "host" (the product's static handlers compiled for the host), "device"."""
    PLANT_STEP = 1 << 24      # the Philox step of a planting generate (nothing is drawn: every site is constrained; no iteration is consumed)

    def __init__(self, which, law, n, seed):
        self.which, self.law, self.n, self.seed, self.iterations = which, law, n, seed, 0
        if which == "device":
            import modppl_amd
            self.g = modppl_amd.FunctionChains(law.kind, law.params, law.constraints, n, seed)
        else:
            from tests import oracle_lib as O
            cls = O.OracleFunctionChains if which == "tries" else O.HostStaticFunctionChains
            self.g = cls(law.kind, law.params, law.constraints, n, seed)

    def trace(self):
        v, p = self.g.trace()
        return v, p.astype(np.uint64)

    def logjp(self):
        return self.g.logjp()

    def mh(self, prop, n_iters=1):
        self.iterations += n_iters
        return self.g.mh(prop.kind, prop.args, n_iters)

    def regen_mh(self, mask, n_iters=1, cycle=False):
        self.iterations += n_iters
        return self.g.regen_mh(mask, n_iters, cycle)

    def propose(self, prop, step):
        (cv, cp), w = self.g.propose(prop.kind, prop.args, rng_step=step)
        return (cv, cp.astype(np.uint64)), w

    def plant(self, v, p):
        """generate((values, present)) with every latent constrained per chain; observations stay constrained as at creation"""
        w = self.g.generate((v, p), rng_step=self.PLANT_STEP)
        assert np.all(np.isfinite(w))

    def accept_uniforms(self, step):
        from tests import oracle_lib as O
        L = O.load()
        u, tmp = np.empty(self.n), np.empty(1)
        for i in range(self.n):
            L.oracle_u01_stream(self.seed, i, step, 2, 0, 1, O.dptr(tmp))   # (DOM_ACCEPT, site 0) of MH iteration `step`
            u[i] = tmp[0]
        return u


# =========================================================================================================================
# Checks
# =========================================================================================================================
def check_logjoint(eng, what):
    """(a) logjp() of every chain equals the statement.  Bound, per chain (Law.logjoint): every normal site K_NORMAL U times the magnitudes
    of its terms, plus |z| / sd times the mean's own roundings; a bernoulli K_BERN U (1 + |lp|); nterm - 1 additions of partial sums; the
    statement's own long-double error is 2^-11 of that.  Asserted as well: it never exceeds the 1e-12 relative + 1e-10 absolute the suite used before."""
    v, p = eng.trace()
    ref, tol = eng.law.logjoint(v, p)
    got = eng.logjp()
    assert np.all(np.isfinite(got)), what
    assert np.all(tol <= 1e-10 + 1e-12 * np.abs(ref)), (what, "the derived bound exceeds the ceiling", float(np.max(tol)))
    err = np.abs(got.astype(LD) - ref)
    worst = int(np.argmax(err / tol))
    assert np.all(err <= tol), (eng.law.name, eng.which, what, worst, float(err[worst]), float(tol[worst]), float(got[worst]))
    return float((err / tol).max())


def check_logjoint_mp(law, v, p, n=48):
    """the long-double statement against the same statement in mpmath at 160 bits: within 2^-58 of the magnitudes"""
    with mpmath.workprec(MP_BITS):
        ref, _ = law.logjoint(v[:n], p[:n], mp=True)
        got, _ = law.logjoint(v[:n], p[:n])
        mag = law.walk(v[:n], p[:n]).mag
        for i in range(min(n, v.shape[0])):
            hi = float(got[i])
            lo = float(got[i] - LD(hi))
            assert abs(mpmath.mpf(hi) + mpmath.mpf(lo) - ref[i]) <= 2.0 ** -58 * float(mag[i]) * law.ns, (law.name, i)


class Tally:
    """both outcomes, and both directions of every structure change, must be met by at least 50 chains"""

    def __init__(self):
        self.acc = self.rej = 0
        self.dirs = {}

    def require(self, structure_sites):
        assert self.acc >= 50 and self.rej >= 50, (self.acc, self.rej)
        for s in structure_sites:
            for d in ((s, 0, 1), (s, 1, 0)):
                assert self.dirs.get(d, 0) >= 50, (d, self.dirs)


def check_accept_decisions(eng, prop, tally):
    """(b) one mh move: every chain's decision is the one the textbook ratio gives."""
    law = eng.law
    step = eng.iterations + 1
    old = eng.trace()
    choices, _ = eng.propose(prop, step)
    alpha, new, tol = mh_alpha(law, prop, old, choices)
    lnu = np.log(eng.accept_uniforms(step).astype(LD))
    # undecided: |ln u - alpha| within the bound of (a) for the four log-densities alpha is made of, plus the engine's own ln u (< 1 ulp)
    clear = np.abs(lnu - alpha) > tol + U * np.abs(lnu)
    assert (~clear).sum() <= 1e-6 * eng.n, ("undecided chains", int((~clear).sum()))
    want = lnu < alpha
    got_count = eng.mh(prop, 1)
    now = eng.trace()
    moved = np.any(now[0] != old[0], axis=1) | (now[1] != old[1])
    same = np.all(new[0] == old[0], axis=1) & (new[1] == old[1])        # a proposal of the current trace: accepted or not, nothing moves
    ck = clear & ~same
    bad = np.flatnonzero(ck & (moved != want))
    assert bad.size == 0, (law.name, eng.which, prop.name, "decisions differ", bad[:5], [float(alpha[i]) for i in bad[:5]], [float(lnu[i]) for i in bad[:5]])
    assert np.array_equal(now[0][moved], new[0][moved]) and np.array_equal(now[1][moved], new[1][moved]), (prop.name, "moved chains do not hold the proposal")
    dropped = old[1] & ~new[1]
    assert not np.any(now[1][moved] & dropped[moved]), "a dropped site is still present"
    assert abs(got_count - int(want.sum())) <= int((~clear).sum()), (prop.name, got_count, int(want.sum()))
    tally.acc += int((want & ck).sum())
    tally.rej += int((~want & ck).sum())
    if prop.changes is not None:
        a, b = old[0][:, prop.changes] != 0, new[0][:, prop.changes] != 0
        for d in ((0, 1), (1, 0)):
            key = (prop.changes, *d)
            tally.dirs[key] = tally.dirs.get(key, 0) + int((want & ck & (a == bool(d[0])) & (b == bool(d[1]))).sum())
    return check_logjoint(eng, f"after {prop.name}")


def ks_crit(n):
    """Dvoretzky-Kiefer-Wolfowitz: P(D > d) <= 2 exp(-2 n d^2)"""
    return math.sqrt(math.log(2.0 / ALPHA) / (2.0 * n))


def _moment_tests(z, what):
    """z [n, d], i.i.d. N(0, 1) under the hypothesis: Kolmogorov-Smirnov per coordinate (DKW bound); mean (variance 1/n), second moment
    (n m2 is chi-square with n degrees of freedom: its exact quantiles), every pairwise product (variance 1/n).  -> assertions made"""
    n, d = z.shape
    made = 0
    for j in range(d):
        x = np.sort(z[:, j])
        cdf = stats.norm.cdf(x)
        D = max(np.max(np.arange(1, n + 1) / n - cdf), np.max(cdf - np.arange(0, n) / n))
        assert D < ks_crit(n), (what, "KS", j, float(D), ks_crit(n))
        assert abs(x.mean()) * math.sqrt(n) < Z_CRIT, (what, "mean", j, float(x.mean() * math.sqrt(n)))
        s2 = float(np.sum(x * x))
        assert stats.chi2.ppf(ALPHA / 2, n) < s2 < stats.chi2.isf(ALPHA / 2, n), (what, "variance", j, s2 / n)
        made += 3
        for k in range(j + 1, d):
            c = float(np.mean(z[:, j] * z[:, k])) * math.sqrt(n)
            assert abs(c) < Z_CRIT, (what, "product", j, k, c)
            made += 1
    return made


def check_exact_sample(law, trace, what):
    """the chains against the exact posterior.  -> assertions made"""
    v, p = trace
    n = v.shape[0]
    cs = law.configs()
    idx = law.config_index(v)
    made = 0
    for k, c in enumerate(cs):
        assert np.all(p[idx == k] == np.uint64(c.present)), (what, "presence word of configuration", c.cfg)
    if len(cs) > 1:
        counts = np.bincount(idx, minlength=len(cs)).astype(np.float64)
        expect = n * np.array([c.post for c in cs])
        big = expect >= MIN_EXPECT
        O_, E_ = list(counts[big]), list(expect[big])
        if (~big).any():
            if expect[~big].sum() >= MIN_EXPECT:
                O_.append(counts[~big].sum()); E_.append(expect[~big].sum())
            else:                                   # pooled with the smallest kept cell
                j = int(np.argmin(E_))
                O_[j] += counts[~big].sum(); E_[j] += expect[~big].sum()
        O_, E_ = np.array(O_), np.array(E_)
        x2 = float(np.sum((O_ - E_) ** 2 / E_))
        assert x2 < stats.chi2.isf(ALPHA, len(E_) - 1), (what, "configuration counts", x2, counts[:8], expect[:8])
        made += 1
        for s in law.discrete:
            q = sum(c.post for c in cs if c.cfg[law.discrete.index(s)])
            z = ((v[:, s] != 0).sum() - n * q) / math.sqrt(n * q * (1 - q))
            assert abs(z) < Z_CRIT, (what, "marginal of site", s, float(z), q)
            made += 1
    # whitened coordinates: pooled over all chains for the coordinates every configuration has, and per configuration where it expects
    # MIN_CELL chains or more (kind 102's 64 configurations: the larger ones only; the rest are held by the counts and the pooled test)
    dmin = min(len(c.cont) for c in cs)
    pooled = np.empty((n, dmin))
    for k, c in enumerate(cs):
        sel = idx == k
        if not sel.any():
            continue
        z = law.whiten(v[sel], k)
        pooled[sel] = z[:, :dmin]
        if len(cs) > 1 and c.post * n >= MIN_CELL and sel.sum() >= MIN_CELL // 2:
            made += _moment_tests(z, (what, c.cfg))
    made += _moment_tests(pooled, (what, "pooled"))
    return made


def predicted_accepts(eng, prop, dt=LD):
    """sum of min(1, e^alpha_i) over the engine's chains for the proposals it is about to make -> (mean, variance)"""
    old = eng.trace()
    choices, _ = eng.propose(prop, eng.iterations + 1)
    alpha, _, _ = mh_alpha(eng.law, prop, old, choices, dt=dt)
    pa = np.minimum(1.0, np.exp(np.minimum(alpha, 0).astype(np.float64)))
    return float(pa.sum()), float((pa * (1 - pa)).sum())


def check_stationarity(eng, move, k, rng_seed, dt=LD):
    """(c) plant exact posterior draws, apply k moves of one type: the chains are still exact posterior draws.
    move = ("mh", Proposal) | ("regen", sites) | ("cycle", sites).  -> assertions made"""
    law = eng.law
    rng = np.random.default_rng(rng_seed)
    v, p = law.sample(rng, eng.n)
    eng.plant(v, p)
    tv, tp = eng.trace()
    assert np.array_equal(tv, v) and np.array_equal(tp, p), "planting"
    check_logjoint(eng, "after planting")
    what = (law.name, eng.which, move[0], getattr(move[1], "name", move[1]), k)
    made = 2
    if move[0] == "mh":
        mean, var = predicted_accepts(eng, move[1], dt=dt)
        got = eng.mh(move[1], 1)
        assert abs(got - mean) <= 6 * math.sqrt(var), (what, "accept count", got, mean, math.sqrt(var))
        if k > 1:
            eng.mh(move[1], k - 1)
    else:
        cycle = move[0] == "cycle"
        sites = move[1]
        first = [sites[eng.iterations % len(sites)]] if cycle else sites
        _, acc = regen_move(law, rng, (v, p), first, dt=dt)                     # the numpy kernel on the same planted sample
        got = eng.regen_mh(sites, 1, cycle)
        r1, r2 = acc.sum() / eng.n, got / eng.n
        # two independent counts: 6 sigma of the two binomial errors combined
        assert abs(got - acc.sum()) <= 6 * math.sqrt(eng.n * r1 * (1 - r1) + eng.n * r2 * (1 - r2)), (what, "accept count against the numpy kernel", got, int(acc.sum()))
        if k > 1:
            eng.regen_mh(sites, k - 1, cycle)
    check_logjoint(eng, "after the moves")
    return made + 1 + check_exact_sample(law, eng.trace(), what)


def moves_of(law):
    single, joint, cycle = regen_masks(law)
    out = [("mh", pr) for pr in proposals(law)] + [("regen", m) for m in single]
    if joint is not None:
        out += [("regen", joint), ("cycle", cycle)]
    return out


# =========================================================================================================================
# (d) the hand-written engines from the prior: one sweep of the schedule, for the numpy kernel and for an engine
# =========================================================================================================================
def sweep_schedule(law):
    """hierarchical: add_or_remove, three drifts at 0.1, two at 0.02 (the reference's own loop, tests/mh.rs:93-106, with its second drift
    at this data's scale); pointed: each of the three noise matrices once"""
    pr = proposals(law)
    if law.kind == 120:
        return [(q, 1) for q in pr]
    by = {q.name: q for q in pr}
    return [(by["add_or_remove"], 1), (by["drift 0.1"], 3), (by["drift 0.02"], 2)]


def numpy_sweeps_to_converge(law, n, seed, k_max):
    """the numpy kernel from prior draws: the first number of sweeps after which every statistic of (c) passes"""
    rng = np.random.default_rng(seed)
    cur = law.prior_sample(rng, n)
    for k in range(1, k_max + 1):
        for q, reps in sweep_schedule(law):
            for _ in range(reps):
                cur, _ = mh_move(law, q, rng, cur, dt=np.float64)
        try:
            check_exact_sample(law, cur, ("numpy from the prior", k))
            return k
        except AssertionError:
            pass
    return None
