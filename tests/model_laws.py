"""The filter models written down a second time, in Python, from their prose: the comment block above each functor in
modppl_amd/csrc/mp_models.h and the reference's own text (modppl/tests/dyngenfns/unfold.rs, tests/hmm/model.rs,
src/modeling/dists/mvnormal.rs).  Nothing here includes, parses or calls the C++: the device and the CPU checker compile
the same functors, so parity between them cannot see a mistake in a functor; these statements can.

Each law gives the observation log-density per particle (np.longdouble, and mpmath at 160 bits for a subset), the
deterministic part of the transition, the law of the noise a step adds and the law of the t = 0 draw.  The checks at
the bottom take an engine adapter (`OracleEngine` for the CPU checker, `DeviceEngine` for the GPU) and a law; they are
called from tests/test_model_laws.py (CPU) and tests/test_gpu_model_laws.py (GPU).  No test functions here.

Statistical conventions are the project's: fixed seeds, p > 1e-4, 5 sigma for moments.
"""
import math

import mpmath
import numpy as np
from scipy import stats

LD = np.longdouble
U = 2.0 ** -52            # one ulp of 1.0: every rounding (2^-53 relative) and every "< 1 ulp" bound is counted as one U
P_MIN = 1e-4
MP_BITS = 160
MP_SUBSET = 2048
LN_2PI = LD(2) * np.arctan2(LD(0), LD(-1))   # 2 pi in long double ...
LN_2PI = np.log(LN_2PI)                      # ... and its logarithm

# Roundings in the chain of one normal log-density, -(z*z + ln 2pi)/2 - ln sd with z = (x - mu)/sd (mp_dists.h,
# mp_normal_logpdf_ln):  x - mu (1) and the division (1) give z two roundings; z*z carries them twice (4) and adds its own (1);
# + ln 2pi (1); the constant ln 2pi is an mp_log value, < 1 ulp (tests/test_math.py) (1); the halving is exact; - ln sd (1);
# ln sd itself is an mp_log value (1).  Total 9.
K_NORMAL = 9
# ulp bounds asserted elsewhere in the suite (tests/test_trig_exact.py): mp_atan2 <= 2 ulp, mp_sin / mp_cos < 1 ulp
ULP_ATAN2 = 2.0
ULP_SINCOS = 1.0


def _normal_terms(x, mu, sd):
    """-> (logpdf, M, |z|) in long double; M = the sum of the magnitudes of the formula's terms"""
    x, mu, sd = LD(1) * x, LD(1) * mu, LD(sd)
    z = (x - mu) / sd
    lp = -(z * z + LN_2PI) / 2 - np.log(sd)
    return lp, z * z / 2 + LN_2PI / 2 + abs(np.log(sd)), np.abs(z)


def _mp_normal(x, mu, sd):
    z = (mpmath.mpf(float(x)) - mu) / mpmath.mpf(float(sd))
    return -(z * z + mpmath.log(2 * mpmath.pi)) / 2 - mpmath.log(mpmath.mpf(float(sd)))


class Law:
    """kind / dims / params: what both engines are created from.  noise_sd[j]: the stated standard deviation of residual
    coordinate j; free: the coordinates whose noises are independent draws (bearings: the two velocities; the positions
    are tied to them exactly)."""
    args0 = None
    categorical = False

    def obs_logpdf(self, states, obs):
        return self.obs_terms(states, obs)[0]

    def residual(self, nxt, prev_of_parent):
        return nxt - self.drift(prev_of_parent)


class Lgssm1(Law):
    """t==0: x ~ normal(mu0, sig0); t>0: x ~ normal(a x_prev, sig_x); y ~ normal(x, sig_y) observed."""
    name, kind, dim_state, dim_obs = "lgssm1", 1, 1, 1
    K_OBS = K_NORMAL + 2    # the site's value is added to the handler's weight (1) and that to the particle's log-weight (1)

    def __init__(self, mu0=0.0, sig0=1.0, a=0.9, sig_x=0.5, sig_y=1.0):
        self.mu0, self.sig0, self.a, self.sig_x, self.sig_y = mu0, sig0, a, sig_x, sig_y
        self.params = np.array([mu0, sig0, a, sig_x, sig_y])
        self.noise_sd, self.free = np.array([sig_x]), [0]

    def device_model(self):
        import modppl_amd
        return modppl_amd.lgssm_model(self.mu0, self.sig0, self.a, self.sig_x, self.sig_y)

    def obs_terms(self, x, y):
        return _normal_terms(y[0], x[:, 0], self.sig_y)

    def obs_logpdf_mp(self, x, y):
        return [_mp_normal(y[0], mpmath.mpf(float(v)), self.sig_y) for v in x[:, 0]]

    def drift(self, prev):
        return self.a * prev

    def init_dists(self):
        return [stats.norm(self.mu0, self.sig0)]

    def simulate(self, rng, T):
        x, out = self.mu0 + self.sig0 * rng.normal(), []
        for t in range(T):
            if t:
                x = self.a * x + self.sig_x * rng.normal()
            out.append([x + self.sig_y * rng.normal()])
        return np.array(out)


class Spiral(Law):
    """t==0: r ~ uniform(0,1), theta ~ uniform(0, 2pi); t>0: pol = prev + (dr, dtheta), dr ~ normal(0, 0.1),
    dtheta ~ normal(0.4, 0.2); obs ~ mvnormal((r cos theta, r sin theta), 0.001 I)."""
    name, kind, dim_state, dim_obs = "spiral", 2, 2, 2
    args0 = [0.0, 0.0]
    VAR = 0.001
    # per coordinate: c = x - mu (1), carried twice by the quadratic (2); the inverse-covariance entry, a division and at most one
    # elimination step when the engine derives it per call (2); two products (2) -> 6.  Two accumulations of the quadratic form (2);
    # the constant ln 2pi (1); ln det: the determinant's product (1, as an absolute error it is far below 1 ulp of 13.8) and mp_log (1);
    # two additions (2); the halving is exact; the addition to the log-weight (1).  Total 6 + 2 + 1 + 2 + 2 + 1 = 14.
    K_OBS = 14
    # mean_k = r * cos/sin(theta): the function < 1 ulp, the product half an ulp more -> 2 ulp of |mean_k| bounds it
    ULP_MEAN = ULP_SINCOS + 1.0

    def __init__(self):
        self.params = np.zeros(0)
        self.noise_sd, self.free = np.array([0.1, 0.2]), [0, 1]

    def device_model(self):
        import modppl_amd
        return modppl_amd.spiral_model()

    def obs_terms(self, x, y):
        r, th = LD(1) * x[:, 0], LD(1) * x[:, 1]
        mean = np.stack([r * np.cos(th), r * np.sin(th)], axis=1)
        sd = np.sqrt(LD(self.VAR))
        z = (LD(1) * np.asarray(y)[None, :] - mean) / sd
        ln_det = 2 * np.log(LD(self.VAR))
        lp = -(2 * LN_2PI + ln_det + (z * z).sum(1)) / 2
        M = (z * z).sum(1) / 2 + LN_2PI + abs(ln_det) / 2 + (np.abs(z) / sd * self.ULP_MEAN * np.abs(mean)).sum(1)
        return lp, M, np.abs(z).max(1)

    def obs_logpdf_mp(self, x, y):
        out, var = [], mpmath.mpf(self.VAR)
        for r, th in x:
            r, th = mpmath.mpf(float(r)), mpmath.mpf(float(th))
            q = ((mpmath.mpf(float(y[0])) - r * mpmath.cos(th)) ** 2 + (mpmath.mpf(float(y[1])) - r * mpmath.sin(th)) ** 2) / var
            out.append(-(2 * mpmath.log(2 * mpmath.pi) + 2 * mpmath.log(var) + q) / 2)
        return out

    def drift(self, prev):
        return prev + np.array([0.0, 0.4])

    def init_dists(self):
        return [stats.uniform(0, 1), stats.uniform(0, 2 * math.pi)]

    def simulate(self, rng, T):
        pol, out = np.array([rng.uniform(0, 1), rng.uniform(0, 2 * math.pi)]), []
        for t in range(T):
            if t:
                pol = pol + np.array([0.1 * rng.normal(), 0.4 + 0.2 * rng.normal()])
            out.append(pol[0] * np.array([math.cos(pol[1]), math.sin(pol[1])]) + math.sqrt(self.VAR) * rng.normal(size=2))
        return np.array(out)

    # --- one-step evidence: Z(y) = int_0^1 int_0^2pi (1 / 2pi) N(y; (r cos th, r sin th), 0.001 I) dth dr
    Y_EVIDENCE = np.array([0.15, 0.2])   # r = 0.25: relative variance of a weight ~ r / (2 var) = 125, s.e. 0.022 at 2^18 particles

    def log_evidence(self, y, order):
        xr, wr = _gauss_legendre(order, 0.0, 1.0)
        xt, wt = _gauss_legendre(2 * order, 0.0, 2 * math.pi)
        R, T = xr[:, None], xt[None, :]
        q = ((y[0] - R * np.cos(T)) ** 2 + (y[1] - R * np.sin(T)) ** 2) / self.VAR
        dens = np.exp(-q / 2) / (2 * math.pi * self.VAR) / (2 * math.pi)
        return math.log(float(wr @ dens @ wt))


class Hmm(Law):
    """state ~ categorical(prior | transition column of the previous state); weight = ln emission[obs][state].
    Column-stochastic tables: emission[o, s] = p(o | s), transition[s2, s1] = p(s2 | s1)."""
    name, kind, dim_state, dim_obs = "hmm", 3, 1, 1
    categorical = True
    K_OBS = 2   # mp_log of the table entry, < 1 ulp (tests/test_math.py) (1); the addition to the log-weight (1)

    def __init__(self, prior, emis, trans):
        self.prior, self.emis, self.trans = np.asarray(prior, float), np.asarray(emis, float), np.asarray(trans, float)
        self.S, self.O = self.prior.size, self.emis.shape[0]
        self.params = np.concatenate([[self.S, self.O], self.prior, self.emis.reshape(-1), self.trans.reshape(-1)])

    def device_model(self):
        import modppl_amd
        return modppl_amd.hmm_model(self.prior, self.emis, self.trans)

    def obs_terms(self, x, y):
        p = self.emis[int(y[0]), x[:, 0].astype(np.int64)]
        lp = np.log(LD(1) * p)
        return lp, np.abs(lp), np.abs(lp)

    def obs_logpdf_mp(self, x, y):
        return [mpmath.log(mpmath.mpf(float(self.emis[int(y[0]), int(s)]))) for s in x[:, 0]]

    def simulate(self, rng, T):
        s, out = rng.choice(self.S, p=self.prior), []
        for t in range(T):
            if t:
                s = rng.choice(self.S, p=self.trans[:, s])
            out.append([float(rng.choice(self.O, p=self.emis[:, s]))])
        return np.array(out)


class Bearings(Law):
    """t==0: px ~ normal(p0x, sig_p0), py ~ normal(p0y, sig_p0), vx, vy ~ normal(0, sig_v0);
    t>0: a ~ normal(0, sig_a)^2, v' = v + a, p' = (p + v) + 0.5 a; theta ~ normal(atan2(py, px), sig_theta) observed, no wrap."""
    name, kind, dim_state, dim_obs = "bearings", 4, 4, 1
    K_OBS = K_NORMAL + 2

    def __init__(self, p0x=1.0, p0y=1.0, sig_p0=1.0, sig_v0=0.1, sig_a=0.05, sig_theta=0.02):
        self.p0x, self.p0y, self.sig_p0, self.sig_v0, self.sig_a, self.sig_theta = p0x, p0y, sig_p0, sig_v0, sig_a, sig_theta
        self.params = np.array([p0x, p0y, sig_p0, sig_v0, sig_a, sig_theta])
        self.noise_sd, self.free = np.array([0.5 * sig_a, 0.5 * sig_a, sig_a, sig_a]), [2, 3]

    def device_model(self):
        import modppl_amd
        return modppl_amd.bearings_model(*self.params)

    def obs_terms(self, x, y):
        mean = np.arctan2(LD(1) * x[:, 1], LD(1) * x[:, 0])
        lp, M, az = _normal_terms(y[0], mean, self.sig_theta)
        return lp, M + az / LD(self.sig_theta) * ULP_ATAN2 * np.abs(mean), az

    def obs_logpdf_mp(self, x, y):
        return [_mp_normal(y[0], mpmath.atan2(mpmath.mpf(float(r[1])), mpmath.mpf(float(r[0]))), self.sig_theta) for r in x]

    def drift(self, prev):
        return np.concatenate([prev[:, :2] + prev[:, 2:], prev[:, 2:]], axis=1)

    def init_dists(self):
        return [stats.norm(self.p0x, self.sig_p0), stats.norm(self.p0y, self.sig_p0), stats.norm(0, self.sig_v0), stats.norm(0, self.sig_v0)]

    def simulate(self, rng, T):
        p, v, out = np.array([self.p0x + 0.2, self.p0y - 0.2]), np.array([0.05, 0.08]), []
        for t in range(T):
            if t:
                a = self.sig_a * rng.normal(size=2)
                p, v = p + v + 0.5 * a, v + a
            out.append([math.atan2(p[1], p[0]) + self.sig_theta * rng.normal()])
        return np.array(out)

    # --- one-step evidence in polar coordinates about the origin (px, py) = rho (cos phi, sin phi):
    # Z(theta) = int int N(theta; phi, sig_theta) N2((px, py); (p0x, p0y), sig_p0^2 I) rho drho dphi.  phi is cut at theta +- 12 sig_theta
    # (the normal's tail beyond: 1e-32) and rho at |p0| + 12 sig_p0 (1e-32); theta = 0.8 keeps the window inside (-pi, pi): no wrap.
    Y_EVIDENCE = np.array([0.8])   # the prior's mean direction is pi/4

    def log_evidence(self, y, order):
        s = self.sig_theta
        xp, wp = _gauss_legendre(order, y[0] - 12 * s, y[0] + 12 * s)
        xr, wr = _gauss_legendre(order, 0.0, math.hypot(self.p0x, self.p0y) + 12 * self.sig_p0)
        Ph, Rh = xp[:, None], xr[None, :]
        prior = np.exp(-((Rh * np.cos(Ph) - self.p0x) ** 2 + (Rh * np.sin(Ph) - self.p0y) ** 2) / (2 * self.sig_p0 ** 2)) / (2 * math.pi * self.sig_p0 ** 2)
        lik = np.exp(-((y[0] - xp) / s) ** 2 / 2) / (s * math.sqrt(2 * math.pi))
        return math.log(float((wp * lik) @ (prior * Rh) @ wr))


class Band(Law):
    """A = a (I + band B), B = ones on the two off-diagonals: t==0: x_j ~ normal(0, sig0);
    t>0: x_j ~ normal(a (x_j + band (x_{j-1} + x_{j+1})), sig_x), zero beyond both ends; y_j ~ normal(x_j, sig_y) observed."""
    kind = 5

    def __init__(self, D, a=0.9, band=0.05, sig0=1.0, sig_x=0.5, sig_y=1.0):
        self.D, self.a, self.band, self.sig0, self.sig_x, self.sig_y = D, a, band, sig0, sig_x, sig_y
        self.name, self.dim_state, self.dim_obs = f"band{D}", D, D
        self.params = np.array([D, a, band, sig0, sig_x, sig_y])
        self.noise_sd, self.free = np.full(D, sig_x), list(range(D))
        self.K_OBS = K_NORMAL + D + 1   # D sites added one after the other to the handler's weight (D), that to the log-weight (1)

    def device_model(self):
        import modppl_amd
        return modppl_amd.lgssm_band_model(self.D, self.a, self.band, self.sig0, self.sig_x, self.sig_y)

    def obs_terms(self, x, y):
        lp, M, az = _normal_terms(np.asarray(y)[None, :], x, self.sig_y)
        return lp.sum(1), M.sum(1), az.max(1)

    def obs_logpdf_mp(self, x, y):
        return [mpmath.fsum(_mp_normal(y[j], mpmath.mpf(float(r[j])), self.sig_y) for j in range(self.D)) for r in x]

    def drift(self, prev):
        nb = np.zeros_like(prev)
        nb[:, 1:] += prev[:, :-1]
        nb[:, :-1] += prev[:, 1:]
        return self.a * (prev + self.band * nb)

    def init_dists(self):
        return [stats.norm(0, self.sig0)] * self.D

    def simulate(self, rng, T):
        x, out = self.sig0 * rng.normal(size=self.D), []
        for t in range(T):
            if t:
                x = self.drift(x[None, :])[0] + self.sig_x * rng.normal(size=self.D)
            out.append(x + self.sig_y * rng.normal(size=self.D))
        return np.array(out)


class Dense(Law):
    """t==0: x ~ mvnormal(0, sig0^2 I); t>0: x ~ mvnormal(A x_prev, Q); y ~ mvnormal(x, R) observed.  Q may be singular."""
    kind = 8
    # The engines hold R^-1 from a Gauss-Jordan elimination in double.  Higham, Accuracy and Stability of Numerical Algorithms
    # (2nd ed.), Theorem 14.5: its forward error is bounded by 8 D u cond(R) to first order for a matrix without pivot growth (R is
    # symmetric positive definite), which the quadratic form inherits: c = 8.  The rest of the chain, y - x (1 rounding per coordinate),
    # the two D-long fma chains of the quadratic form and the four closing operations, is 2 D + 5 <= 3 D roundings: c = 3.  c = 11.
    C_DENSE = 11

    def __init__(self, A, Q, R, sig0=1.0, name="dense16"):
        self.A, self.Q, self.R = (np.ascontiguousarray(m, float) for m in (A, Q, R))
        self.sig0 = sig0
        self.D = D = self.A.shape[0]
        self.name, self.dim_state, self.dim_obs = name, D, D
        self.params = np.concatenate([[D, sig0], self.A.reshape(-1), self.Q.reshape(-1), self.R.reshape(-1)])
        self.noise_sd, self.free = np.sqrt(np.diag(self.Q)), list(range(D))
        with mpmath.workprec(MP_BITS):
            Rm = mpmath.matrix(self.R.tolist())
            self._Rinv_mp = Rm ** -1
            self._lndet_mp = mpmath.log(mpmath.det(Rm))
            self._Rinv = np.array([[LD(mpmath.nstr(self._Rinv_mp[i, j], 25)) for j in range(D)] for i in range(D)], dtype=LD)
            self._lndet = LD(mpmath.nstr(self._lndet_mp, 25))
        self.cond = float(np.linalg.cond(self.R, 2))
        assert self.cond < 100, self.cond   # keeps the bound below far under any real error
        lam, V = np.linalg.eigh(self.Q)
        self.q_rank = int((lam > 1e-10 * lam.max()).sum())
        self.q_null = V[:, : D - self.q_rank]          # columns spanning the null space of Q (empty for a full-rank Q)
        self._q_sqrt = V * np.sqrt(np.maximum(lam, 0.0))

    def device_model(self):
        import modppl_amd
        return modppl_amd.lgssm_dense_model(self.A, self.Q, self.R, self.sig0)

    def obs_terms(self, x, y):
        c = LD(1) * np.asarray(y)[None, :] - x
        quad = np.einsum("ni,ij,nj->n", c, self._Rinv, c)
        lp = -(self.D * LN_2PI + self._lndet + quad) / 2
        return lp, np.abs(quad) + abs(self._lndet), np.sqrt(quad)

    def weight_tolerance(self, M):
        """c D 2^-52 cond_2(R) (|quad| + |ln det R|); the D ln 2pi term the formula leaves out costs three roundings at a magnitude of
        29.4 + M, which this bound covers as soon as M >= 1 (c D cond >= 176): asserted."""
        assert np.all(M >= 1.0)
        return self.C_DENSE * self.D * U * self.cond * M

    def obs_logpdf_mp(self, x, y):
        out, D = [], self.D
        rows = [[self._Rinv_mp[i, j] for j in range(D)] for i in range(D)]
        for r in x:
            c = [mpmath.mpf(float(y[j])) - mpmath.mpf(float(r[j])) for j in range(D)]
            quad = mpmath.fdot(c, [mpmath.fdot(rows[i], c) for i in range(D)])
            out.append(-(D * mpmath.log(2 * mpmath.pi) + self._lndet_mp + quad) / 2)
        return out

    def drift(self, prev):
        return prev @ self.A.T

    def init_dists(self):
        return [stats.norm(0, self.sig0)] * self.D

    def simulate(self, rng, T):
        x, out, Lr = self.sig0 * rng.normal(size=self.D), [], np.linalg.cholesky(self.R)
        for t in range(T):
            if t:
                x = self.A @ x + self._q_sqrt @ rng.normal(size=self.D)
            out.append(x + Lr @ rng.normal(size=self.D))
        return np.array(out)


def _gauss_legendre(order, a, b):
    x, w = np.polynomial.legendre.leggauss(order)
    return 0.5 * (b - a) * x + 0.5 * (a + b), 0.5 * (b - a) * w


def make_law(name):
    from tests.test_gpu_dense import dense_problem
    from tests.test_oracle_kats import HMM3   # the HMM of the reference's own particle filter test, tables as it builds them

    if name == "lgssm1":
        return Lgssm1()
    if name == "spiral":
        return Spiral()
    if name == "hmm":
        return Hmm(HMM3["prior"], HMM3["emis"], HMM3["trans"])
    if name == "bearings":
        return Bearings()
    if name == "band2":
        return Band(2)
    if name == "band4":
        return Band(4)
    if name == "band16":
        return Band(16)
    if name == "dense16":
        return Dense(*dense_problem(1), name="dense16")
    if name == "dense16_singular":
        return Dense(*dense_problem(2, singular_q=True), name="dense16_singular")
    raise KeyError(name)


LAW_NAMES = ["lgssm1", "spiral", "hmm", "bearings", "band2", "band16", "dense16", "dense16_singular"]


# ---------------------------------------------------------------------------------------------------------------------------
# one adapter over both engines
# ---------------------------------------------------------------------------------------------------------------------------
class OracleEngine:
    """the CPU checker; soa=False: its structure-faithful dynamic engine.  functor=True: not the checker's own restatement of the
    model but the product's functor (modppl_amd/csrc/mp_models.h) run through the checker's adapter, which
    oracle/src/functor_adapter.hpp registers under kind + 1000 for lgssm1, spiral, bearings and band D = 4: the code the device
    compiles, executed without a GPU."""
    FUNCTOR_LAWS = ("lgssm1", "spiral", "bearings", "band4")

    def __init__(self, law, n, seed, soa=True, threads=4, functor=False):
        from tests import oracle_lib as O

        v = O.VARIANT_CANONICAL | (O.VARIANT_SOA if soa else 0)
        self.law, self.n = law, n
        assert not functor or law.name in self.FUNCTOR_LAWS
        self.e = O.OraclePF(law.kind + (1000 if functor else 0), law.dim_state, law.dim_obs, law.params, n, seed, v, threads=threads if soa else 1)

    def init_step(self, y):
        self.e.init_step(np.asarray(y, float)[None, :], self.law.args0)

    def step(self, y):
        self.e.step(np.asarray(y, float)[None, :])

    def resample(self, sync=True):
        return self.e.resample()

    def states(self):
        return self.e.state()

    def log_weights(self):
        return self.e.log_weights()

    def parents(self):
        return self.e.parents().astype(np.int64)

    def log_ml(self):
        return self.e.log_marginal_likelihood_estimate()

    def form(self):
        return None


class DeviceEngine:
    def __init__(self, law, n, seed):
        import modppl_amd

        self.law, self.n = law, n
        self.e = modppl_amd.ParticleSystem(law.device_model(), n, seed)

    def init_step(self, y):
        self.e.init_step(self.law.args0, np.asarray(y, float)[None, :])

    def step(self, y):
        self.e.step(np.ascontiguousarray(np.asarray(y, float)[None, :]))

    def resample(self, sync=True):
        return self.e.resample(sync=sync)

    def states(self):
        return self.e.states()

    def log_weights(self):
        return self.e.log_weights

    def parents(self):
        return self.e.parents.astype(np.int64)

    def log_ml(self):
        return self.e.log_marginal_likelihood_estimate()

    def form(self):
        return self.e.last_propagate_form()


# ---------------------------------------------------------------------------------------------------------------------------
# (a) weights are the stated density
# ---------------------------------------------------------------------------------------------------------------------------
def _mp_subset(n, absz):
    """a fixed subset of at most MP_SUBSET particles: an even stride through the slots, and the 64 with the largest |z|"""
    if n <= MP_SUBSET:
        return np.arange(n)
    stride = np.arange(MP_SUBSET - 64) * (n // (MP_SUBSET - 64))
    return np.unique(np.concatenate([stride, np.argsort(absz)[-64:]]))


def _compare_weights(law, lw, pieces, what):
    """lw against the sum over `pieces` = [(states, obs), ...] of the stated density.

    Tolerance per particle K 2^-52 M_i: M_i the sum of the magnitudes of the formula's terms over the pieces (with the propagated error
    of the mean, |z|/sigma (ulp bound) |mean|, where the mean goes through atan2, cos or sin), K = law.K_OBS (the count is written
    next to each law) plus one for the addition that joins two steps' weights.  The dense law brings its own bound
    (Dense.weight_tolerance).  Every particle in long double; a subset in mpmath at 160 bits, where the long-double value itself
    must be within 64 long-double roundings (2^-58 M_i) of it.  Nothing here is taken from an engine's output."""
    ref, M, az = LD(0), LD(0), 0
    for x, y in pieces:
        lp, m, a = law.obs_terms(x, y)
        ref, M, az = ref + lp, M + m, np.maximum(az, a)
    assert np.all(np.isfinite(lw)), what
    dense = isinstance(law, Dense)
    tol = law.weight_tolerance(M) if dense else (law.K_OBS + len(pieces) - 1) * U * M
    ref_tol = 2.0 ** -58 * M * (law.cond if dense else 1.0)   # (the dense quadratic form's own conditioning)
    err = np.abs(LD(1) * lw - ref)
    worst = int(np.argmax(err / tol))
    assert np.all(err <= tol), (law.name, what, "long double", worst, float(err[worst]), float(tol[worst]), float(lw[worst]))
    idx = _mp_subset(lw.size, az)
    with mpmath.workprec(MP_BITS):
        tot = [mpmath.mpf(0)] * idx.size
        for x, y in pieces:
            tot = [a + b for a, b in zip(tot, law.obs_logpdf_mp(x[idx], y))]
        for k, i in enumerate(idx):
            assert abs(mpmath.mpf(float(lw[i])) - tot[k]) <= float(tol[i]), (law.name, what, "mpmath", int(i), float(lw[i]), mpmath.nstr(tot[k], 20))
            hi = float(ref[i])
            lo = float(ref[i] - LD(hi))
            assert abs(mpmath.mpf(hi) + mpmath.mpf(lo) - tot[k]) <= float(ref_tol[i]), (law.name, what, "reference", int(i))
    return float((err / tol).max())


def check_weights(eng, law, obs_seed, sync=True):
    """init_step: log_weights == obs_logpdf(states, obs[0]); resample, step: == obs_logpdf(states, obs[1]); a second step without a
    resample: the sum of the two.  Observations drawn from the model by numpy."""
    obs = law.simulate(np.random.default_rng(obs_seed), 3)
    eng.init_step(obs[0])
    x0 = eng.states()
    _compare_weights(law, eng.log_weights(), [(x0, obs[0])], "init_step")
    eng.resample(sync)
    eng.step(obs[1])
    x1 = eng.states()
    _compare_weights(law, eng.log_weights(), [(x1, obs[1])], "resample, step")
    eng.step(obs[2])
    x2 = eng.states()
    _compare_weights(law, eng.log_weights(), [(x1, obs[1]), (x2, obs[2])], "second step without a resample")


# ---------------------------------------------------------------------------------------------------------------------------
# the run the other checks share: init, resample, step, resample, step
# ---------------------------------------------------------------------------------------------------------------------------
class Run:
    pass


def two_steps(eng, law, obs_seed, sync=True):
    obs = law.simulate(np.random.default_rng(obs_seed), 3)
    r = Run()
    r.obs = obs
    eng.init_step(obs[0])
    r.x0 = eng.states()
    eng.resample(sync)
    if sync:
        r.x0_resampled = eng.states()
    eng.step(obs[1])
    r.form1 = eng.form()
    r.x1, r.par1 = eng.states(), eng.parents()
    eng.resample(sync)
    eng.step(obs[2])
    r.form2 = eng.form()
    r.x2, r.par2 = eng.states(), eng.parents()
    assert r.par1.min() >= 0 and r.par1.max() < eng.n and r.par2.max() < eng.n
    if not law.categorical:
        r.r1 = law.residual(r.x1, r.x0[r.par1])
        r.r2 = law.residual(r.x2, r.x1[r.par2])
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# (b) exact structure
# ---------------------------------------------------------------------------------------------------------------------------
def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def check_structure(eng, law, obs_seed):
    r = two_steps(eng, law, obs_seed, sync=True)
    # after a resample every state row is the pre-resample row of its parent, bit for bit
    assert np.array_equal(_bits(r.x0_resampled), _bits(r.x0[r.par1])), law.name
    for x in (r.x0, r.x1, r.x2):
        assert np.all(np.isfinite(x))
    if law.categorical:
        for x in (r.x0, r.x1, r.x2):
            assert np.array_equal(x, np.floor(x)) and x.min() >= 0 and x.max() <= law.S - 1
    if isinstance(law, Bearings):
        for nxt, prev in ((r.x1, r.x0[r.par1]), (r.x2, r.x1[r.par2])):
            nxt, prev = LD(1) * nxt, LD(1) * prev
            for k in (0, 1):
                s = prev[:, k] + prev[:, 2 + k]                     # long double: exact up to 2^-64
                lhs = nxt[:, k] - s                                 # = 0.5 a + the roundings of (p + v) and of its sum with 0.5 a
                rhs = 0.5 * (nxt[:, 2 + k] - prev[:, 2 + k])        # = 0.5 (a + the rounding of v + a); the halving is exact
                # three roundings, each half an ulp of its result: |p + v|, |p'|, and half of |v'|
                bound = 0.5 * U * (np.abs(s) + np.abs(nxt[:, k]) + 0.5 * np.abs(nxt[:, 2 + k])) * (1 + 2.0 ** -10)
                assert np.all(np.abs(lhs - rhs) <= bound), (law.name, k, float(np.abs(lhs - rhs).max()))
    if isinstance(law, Dense) and law.q_rank < law.D:
        for nxt, prev in ((r.x1, r.x0[r.par1]), (r.x2, r.x1[r.par2])):
            res = LD(1) * nxt - (LD(1) * prev) @ (LD(1) * law.A.T)
            null = np.abs(res @ (LD(1) * law.q_null)).max(1)
            norm = np.sqrt((res * res).sum(1))
            assert np.all(null <= 64 * U * norm), (law.name, float((null / norm).max() / U))
    return r


# ---------------------------------------------------------------------------------------------------------------------------
# (c) the noise law, (d) the keying of the draws
# ---------------------------------------------------------------------------------------------------------------------------
def _ks(sample, dist, what):
    p = stats.kstest(sample, dist.cdf).pvalue
    assert p > P_MIN, (what, p)


def _corr(a, b):
    a, b = a - a.mean(), b - b.mean()
    d = math.sqrt(float(a @ a) * float(b @ b))
    return float(a @ b) / d if d > 0 else 0.0


def check_init_law(law, x0):
    n = x0.shape[0]
    if law.categorical:
        counts = np.bincount(x0[:, 0].astype(np.int64), minlength=law.S)
        p = stats.chisquare(counts, law.prior * n).pvalue
        assert p > P_MIN, (law.name, "prior", p)
        return
    for j, d in enumerate(law.init_dists()):
        _ks(x0[:, j], d, (law.name, "t = 0", j))
        assert abs(x0[:, j].mean() - d.mean()) <= 5 * d.std() / math.sqrt(n), (law.name, "t = 0 mean", j)


def check_noise_law(law, nxt, prev_of_parent, res):
    n = nxt.shape[0]
    if law.categorical:
        prev, new = prev_of_parent[:, 0].astype(np.int64), nxt[:, 0].astype(np.int64)
        for s in range(law.S):
            counts = np.bincount(new[prev == s], minlength=law.S)
            if counts.sum() >= 50 * law.S:      # enough for the chi-square approximation (expected counts of 5 at p = 0.1 would need 50)
                p = stats.chisquare(counts, law.trans[:, s] * counts.sum()).pvalue
                assert p > P_MIN, (law.name, "transition column", s, p)
        return
    for j, sd in enumerate(law.noise_sd):
        _ks(res[:, j], stats.norm(0, sd), (law.name, "residual", j))
        assert abs(res[:, j].mean()) <= 5 * sd / math.sqrt(n), (law.name, "residual mean", j, float(res[:, j].mean()))
        m2 = float(np.mean((res[:, j] / sd) ** 2))       # a chi-square(1) per particle: mean 1, variance 2
        assert abs(m2 - 1.0) <= 5 * math.sqrt(2.0 / n), (law.name, "residual second moment", j, m2)
    if isinstance(law, (Band, Spiral)):
        c = np.corrcoef(res.T)
        off = np.abs(c - np.eye(c.shape[0])).max()
        assert off <= 5 / math.sqrt(n), (law.name, "correlation", off)     # s.e. of a sample correlation of independent normals: 1/sqrt(n)
    if isinstance(law, Bearings):
        assert abs(_corr(res[:, 2], res[:, 3])) <= 5 / math.sqrt(n)
    if isinstance(law, Dense):
        S = res.T @ res / n
        qd = np.diag(law.Q)
        se = np.sqrt((np.outer(qd, qd) + law.Q ** 2) / n)                    # Var(r_i r_j) = Q_ii Q_jj + Q_ij^2 for a zero-mean normal
        assert np.all(np.abs(S - law.Q) <= 5 * se), (law.name, "covariance", float((np.abs(S - law.Q) / se).max()))
        if law.q_rank == law.D:
            m = np.einsum("ni,ni->n", res, np.linalg.solve(law.Q, res.T).T)
            _ks(m, stats.chi2(law.D), (law.name, "r' Q^-1 r"))


def _sibling_pairs(par):
    order = np.argsort(par, kind="stable")
    _, first, counts = np.unique(par[order], return_index=True, return_counts=True)
    first = first[counts >= 2]
    return order[first], order[first + 1]


def check_independence(law, r, other):
    """r: a Run; other: the Run of the same filter under another seed"""
    n = r.x1.shape[0]
    assert not np.array_equal(r.x0, other.x0), (law.name, "another seed gave the same t = 0 states")
    assert not np.array_equal(r.x1, other.x1), (law.name, "another seed gave the same states")
    a, b = _sibling_pairs(r.par1)
    assert a.size >= 100, (law.name, "sibling pairs", a.size)
    if law.categorical:
        # siblings draw independently from the parent's transition column: chi-square of the pair counts against the product law
        ps, sa, sb = r.x0[r.par1[a], 0].astype(np.int64), r.x1[a, 0].astype(np.int64), r.x1[b, 0].astype(np.int64)
        for s in range(law.S):
            m = ps == s
            expected = np.outer(law.trans[:, s], law.trans[:, s]).reshape(-1) * m.sum()
            if expected.min() >= 5:
                counts = np.bincount(sa[m] * law.S + sb[m], minlength=law.S ** 2)
                p = stats.chisquare(counts, expected).pvalue
                assert p > P_MIN, (law.name, "sibling pairs of parent state", s, p)
        # a slot's state at t + 1 given its parent's at t does not depend on what the slot drew at t: same-slot pairs (x1[i], x2[i]) with
        # parent state fixed follow the transition column
        prev, own, new = r.x1[r.par2, 0].astype(np.int64), r.x1[:, 0].astype(np.int64), r.x2[:, 0].astype(np.int64)
        for s in range(law.S):
            for o in range(law.S):
                m = (prev == s) & (own == o)
                if (law.trans[:, s] * m.sum()).min() >= 5:
                    p = stats.chisquare(np.bincount(new[m], minlength=law.S), law.trans[:, s] * m.sum()).pvalue
                    assert p > P_MIN / (law.S ** 2), (law.name, "slot's own previous draw", s, o, p)   # S^2 tests share the level
        return
    assert not np.any(np.all(_bits(r.x1[a]) == _bits(r.x1[b]), axis=1)), (law.name, "two siblings drew the same noise")
    prev = r.x0[r.par1]
    for j in law.free:
        c = _corr(r.r1[a, j], r.r1[b, j])
        assert abs(c) <= 5 / math.sqrt(a.size), (law.name, "siblings", j, c, a.size)
        c = _corr(r.r1[:, j], r.r2[:, j])
        assert abs(c) <= 5 / math.sqrt(n), (law.name, "step t against t + 1", j, c)
        assert not np.array_equal(r.r1[:, j], other.r1[:, j])
        for k in range(prev.shape[1]):
            c = _corr(r.r1[:, j], prev[:, k])
            assert abs(c) <= 5 / math.sqrt(n), (law.name, "residual against the parent's state", j, k, c)


# ---------------------------------------------------------------------------------------------------------------------------
# (e) one-step evidence against a quadrature over the prior
# ---------------------------------------------------------------------------------------------------------------------------
EVIDENCE_ORDER = 256    # nodes per axis (twice that in the spiral's angle); the rule's own error is stated by doubling it


def check_one_step_evidence(eng, law):
    y = law.Y_EVIDENCE
    exact, finer = law.log_evidence(y, EVIDENCE_ORDER), law.log_evidence(y, 2 * EVIDENCE_ORDER)
    rule_err = abs(exact - finer)
    assert rule_err < 1e-9, (law.name, exact, finer)
    eng.init_step(y)
    lw = eng.log_weights()
    n = lw.size
    eng.resample()
    lml = eng.log_ml()
    w = np.exp(LD(1) * lw - (LD(1) * lw).max())
    w /= w.sum()
    se = math.sqrt(max(n * float(np.sum(w * w)) - 1.0, 0.0) / n)   # delta method: Var(log Z_hat) ~ (E w^2 / (E w)^2 - 1) / n
    assert abs(lml - finer) <= 4 * se + rule_err, (law.name, lml, finer, se)
    assert se < 0.05, (law.name, se)
    return lml, finer, se
