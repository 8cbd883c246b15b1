// mp_dists.h — the distributions of the hot path as inlinable host/device functions, same
// operations in the same order as modppl's CPU code:
//   normal      modppl/src/modeling/dists/normal.rs:13-27   (logpdf; Marsaglia polar sampler)
//   uniform     modppl/src/modeling/dists/uniform.rs:21-33
//   bernoulli   modppl/src/modeling/dists/bernoulli.rs:11-19
//   categorical modppl/src/modeling/dists/categorical.rs:22-32 (small fixed-size tables)
// Transcendentals are mp_exp/mp_log (mp_math.h); compile with -ffp-contract=off.
#pragma once
#include "mp_math.h"
#include "mp_philox.h"

// Sequential uniform stream of ONE site: the n-th uniform is half (n & 1) of Philox block n >> 1
// (counter layout: mp_philox.h).  `blk` counts whole blocks for samplers that use both halves.
struct mp_site {
    mp_stream s;
    uint32_t domain, site;
    uint32_t blk;
    MP_PHD mp_site(const mp_stream& s_, uint32_t domain_, uint32_t site_) : s(s_), domain(domain_), site(site_), blk(0) {}
    MP_PHD mp_u64x2 next_block() { return s.draw(domain, site, blk++); }
};

// mp_log(2*pi) evaluated once (tests/test_math.py checks the bits against mp_log itself).
#define MP_LN_2PI_CANON (mp_u2f(0x3FFD67F1C864BEB4ull))

// normal.rs:13-17; `ln_sd` = mp_log(sd), hoisted by callers whose sd is a model constant.
MP_HD double mp_normal_logpdf_ln(double x, double mu, double sd, double ln_sd) {
    const double z = (x - mu) / sd;
    const double az = fabs(z);
    return -(az * az + MP_LN_2PI_CANON) / 2. - ln_sd;
}
MP_HD double mp_normal_logpdf(double x, double mu, double sd) { return mp_normal_logpdf_ln(x, mu, sd, mp_log(sd)); }
// ... with the reciprocal of sd hoisted as well (mp_rcp_hoist; 0 = not hoisted): same bits, no division (mp_div_hoisted)
MP_HD double mp_normal_logpdf_h(double x, double mu, double sd, double ln_sd, double rcp_sd) {
    // (the branch-free core: outside its exact range — |x - mu| < 2^-960, or a quotient that overflows — z * z is 0 or infinite
    // whichever of the two quotients it is computed from, and an infinite x - mu stays infinite: the same log-density bits for every
    // input, without the division's code in every site of a model.  mp_probe op MP_PROBE_NORMAL_LOGPDF_H holds it to that.)
    const double z = rcp_sd != 0. ? mp_div_hoisted_core(x - mu, sd, rcp_sd) : (x - mu) / sd;
    const double az = fabs(z);
    return -(az * az + MP_LN_2PI_CANON) / 2. - ln_sd;
}

// The accepted pair (u, r = u*u + v*v) of the polar method does not depend on (mu, sd), so the
// rejection loop can run ahead of the model (mp_pf.hip, k_propagate) and the model consumes it here.
// normal.rs:25-26: c = sqrt(-2 ln r / r); u*c*std + mu.
// The standard deviate z = u*c is the parameter-free part: `u * c * std + mu` evaluates as ((u*c)*std) + mu, so a kernel may
// produce z anywhere (another lane, another launch) and the model finishes with z*sd + mu — same operations, same order.
// (SC: mp_log_'s choice of where its constants live, mp_math.h — true in the propagate kernels of the models with few deviates per particle)
template <bool SC = false> MP_HD double mp_std_normal_from_pair(double u, double r) {
    const double c = mp_sqrt(-2. * mp_log_<SC>(r) / r);
    return u * c;
}
MP_HD double mp_normal_from_pair(double u, double r, double mu, double sd) { return mp_std_normal_from_pair(u, r) * sd + mu; }
// one attempt of the polar method on a Philox block: (u, r) and whether normal.rs:22 accepts it
MP_HD bool mp_polar_attempt(const mp_u64x2& b, double* u_out, double* r_out) {
    const double u = mp_u01(b.a) * 2. - 1.;
    const double v = mp_u01(b.b) * 2. - 1.;
    const double r = u * u + v * v;
    *u_out = u;
    *r_out = r;
    return !(r == 0. || r > 1.);
}

// normal.rs:19-27: u,v = 2*u01-1; r = u*u+v*v; reject r == 0 or r > 1 (the reference recurses);
// c = sqrt(-2 ln r / r); return u*c*std + mu.  Only u*c is used, as in the reference.
MP_HD double mp_normal_sample(mp_site& st, double mu, double sd) {
    for (;;) {
        const mp_u64x2 b = st.next_block();
        const double u = mp_u01(b.a) * 2. - 1.;
        const double v = mp_u01(b.b) * 2. - 1.;
        const double r = u * u + v * v;
        if (r == 0. || r > 1.) continue;
        return mp_normal_from_pair(u, r, mu, sd);
    }
}

// uniform.rs:21-33 (bounds are model constants here; a >= b is rejected on the host)
MP_HD double mp_uniform_logpdf(double x, double a, double b) { return (a <= x && x <= b) ? -mp_log(b - a) : MP_NEG_INF; }
MP_HD double mp_uniform_sample(mp_site& st, double a, double b) {
    const mp_u64x2 blk = st.next_block();
    return mp_u01(blk.a) * (b - a) + a;
}

// bernoulli.rs:11-19
MP_HD double mp_bernoulli_logpdf(bool v, double p) { return mp_log(v ? p : 1. - p); }
MP_HD bool mp_bernoulli_sample(mp_site& st, double p) {
    const mp_u64x2 blk = st.next_block();
    return p > mp_u01(blk.a);
}

// categorical.rs:22-32 over a small table: t=0; x=0; while t<u {t+=p[x]; x+=1}; return x-1.
// u == 0 returns -1 in the reference (and then panics as a usize index); here it is clamped to 0.
// Running past the table (sum < u) is an index panic there; here it is clamped to n-1.
MP_HD int mp_categorical_scan(double u, const double* probs, int n) {
    double t = 0.;
    int x = 0;
    while (t < u && x < n) {
        t += probs[x];
        x += 1;
    }
    return x > 0 ? x - 1 : 0;
}

// mvnormal.rs:14-22 with the per-call determinant/inverse hoisted: cov_inv (row-major KxK) and
// ln_det = mp_log(det cov) are model constants.  Quadratic form in the reference's order:
// (c^T * cov_inv) first, then dotted with c.
template <int K>
MP_HD double mp_mvnormal_logpdf_pre(const double* x, const double* mu, const double* cov_inv, double ln_det) {
    double c[K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = x[i] - mu[i];
    double maha = 0.;
#pragma unroll
    for (int j = 0; j < K; ++j) {
        double r = 0.;
#pragma unroll
        for (int i = 0; i < K; ++i) r += c[i] * cov_inv[i * K + j];
        maha += r * c[j];
    }
    return -((double)K * MP_LN_2PI_CANON + ln_det + maha) / 2.;
}

// ---- dense K x K forms in the MATRIX CORE's accumulation order --------------------------------------------------------
// v_mfma_f64_16x16x4_f64 computes D = fma(a_3, b_3, fma(a_2, b_2, fma(a_1, b_1, fma(a_0, b_0, C)))): a k-ascending fma chain
// from C (pinned on the device by tests/test_gpu_math.py::test_mfma_f64_accumulation_order).  Models whose transition is a
// dense matvec (mp_lgssm_dense) define their products as that chain, so the scalar form below, the MFMA kernel
// (k_propagate_dense16) and the CPU checker's canonical arithmetic give the same bits; the literal checker keeps
// nalgebra's multiply-then-add.
template <int K>
MP_HD double mp_dot_chain(const double* a, int stride_a, const double* b, int stride_b, double c0) {
    double acc = c0;
#pragma unroll
    for (int k = 0; k < K; ++k) acc = fma(a[k * stride_a], b[k * stride_b], acc);
    return acc;
}
// mvnormal.rs:14-22, covariance constants hoisted (cov_inv row-major, ln_det): r_j = sum_i c_i inv[i][j]; maha = sum_j r_j c_j
template <int K>
MP_HD double mp_mvnormal_logpdf_chain(const double* x, const double* mu, const double* cov_inv, double ln_det) {
    double c[K], r[K];
#pragma unroll
    for (int i = 0; i < K; ++i) c[i] = x[i] - mu[i];
#pragma unroll
    for (int j = 0; j < K; ++j) r[j] = mp_dot_chain<K>(c, 1, cov_inv + j, K, 0.);
    const double maha = mp_dot_chain<K>(r, 1, c, 1, 0.);
    return -((double)K * MP_LN_2PI_CANON + ln_det + maha) / 2.;
}
// mvnormal.rs:24-37: transform * z + mu with z_j ~ normal(0, 1) in index order from ONE site's stream (`transform` = lower
// Cholesky factor, or the eigen form V sqrt(diag) when the covariance has no Cholesky factor: any K x K matrix here)
template <int K>
MP_HD void mp_mvnormal_sample_chain(mp_site& st, const double* mu, const double* transform, double* out) {
    double z[K];
#pragma unroll 1
    for (int j = 0; j < K; ++j) z[j] = mp_normal_sample(st, 0., 1.);
#pragma unroll
    for (int i = 0; i < K; ++i) out[i] = mp_dot_chain<K>(transform + i * K, 1, z, 1, 0.) + mu[i];
}

// categorical.rs:12-32 over a small probability table
MP_HD double mp_categorical_logpdf(int x, const double* probs, int n) { return (x >= 0 && x < n) ? mp_log(probs[x]) : MP_NEG_INF; }
MP_HD int mp_categorical_sample(mp_site& st, const double* probs, int n) {
    const mp_u64x2 blk = st.next_block();
    return mp_categorical_scan(mp_u01(blk.a), probs, n);
}

// ---- counts and positive reals: poisson, gamma, beta, geometric, uniform_discrete ------------------------------------------
//   poisson          modppl/src/modeling/dists/poisson.rs    rate r > 0                 k = 0, 1, ...
//   gamma            modppl/src/modeling/dists/gamma.rs      shape a > 0, SCALE b > 0   x > 0
//   beta             modppl/src/modeling/dists/beta.rs       a, b > 0                   0 < x < 1
//   geometric        modppl/src/modeling/dists/geometric.rs  0 < p < 1                  k = 0, 1, ... (failures before the first success)
//   uniform_discrete modppl/src/modeling/dists/uniform.rs    integers a <= b            a, ..., b
// Integer values travel as doubles (as bernoulli's 0 / 1 do).  Log-densities: a value outside the support (a negative or non-integer
// count, x <= 0, ...) is -inf; parameters outside the ranges above give NaN.  The reference's log-factorials (a sum of logs) and
// gamma-function ratios become mp_lgamma; log(1 - p) is mp_log1p(-p).
// Samplers draw whole Philox blocks from their own site's stream (mp_site), one after the other: how many attempts a rejection
// sampler needs changes no other site's draws.  Continuous samples lie strictly inside the support: an underflowed gamma or beta
// variate is clamped to the smallest positive normal double, a beta variate that rounds to 1 to 1 - 2^-53.
#include "mp_binomial.h"   // mp_stirling_tail

#define MP_NAN (mp_u2f(0x7FF8000000000000ull))
#define MP_MIN_NORMAL 0x1p-1022
#define MP_ONE_MINUS_ULP 0x1.fffffffffffffp-1   // 1 - 2^-53, the largest double below 1
constexpr uint32_t MP_DIST_MAX_ATTEMPTS = 256u; // rejection samplers: acceptance >= 0.6 per attempt, so never reached in practice

// a count: a finite, non-negative integer
MP_HD bool mp_is_count(double k) { return k >= 0. && k - floor(k) == 0.; }

// poisson.rs:17-19: k ln r - r - ln k!; k = 0 gives -r (no 0 * ln r term: an underflowed rate of 0 scores a zero count as 0)
MP_HD double mp_poisson_logpdf(double k, double r) {
    if (!(r >= 0.)) return MP_NAN;
    if (!mp_is_count(k) || r == MP_INF) return MP_NEG_INF;
    if (k == 0.) return -r;
    return k * mp_log(r) - r - mp_lgamma(k + 1.);
}
// r < 10: inversion by sequential search from 0 (one block; the search stops at 64, where the remaining mass is < 1e-30);
// r >= 10: PTRS, the transformed rejection sampler with squeeze of W. Hoermann, "The transformed rejection method for generating
// Poisson random variables", Insurance: Math. Econ. 12 (1993), restated from the published steps: attempt j takes block j as (U, V).
// A rate of 0 gives 0; a negative, non-finite or >= 2^52 rate gives NaN.
MP_HD double mp_poisson_sample(mp_site& st, double r) {
    if (!(r >= 0.) || !(r < 0x1p52)) return MP_NAN;
    if (r < 10.) {
        const double u = mp_u01(st.next_block().a);
        double p = mp_exp(-r), F = p, k = 0.;
        while (u > F && k < 64.) {
            k += 1.;
            p = p * r / k;
            F += p;
        }
        return k;
    }
    const double slam = mp_sqrt(r), loglam = mp_log(r);
    const double b = 0.931 + 2.53 * slam;
    const double a = -0.059 + 0.02483 * b;
    const double ln_inv_alpha = mp_log(1.1239 + 1.1328 / (b - 3.4));
    const double vr = 0.9277 - 3.6224 / (b - 2.);
    for (uint32_t att = 0; att < MP_DIST_MAX_ATTEMPTS; ++att) {
        const mp_u64x2 blk = st.next_block();
        const double U = mp_u01(blk.a) - 0.5;
        const double V = mp_u01(blk.b);
        const double us = 0.5 - fabs(U);
        const double k = floor((2. * a / us + b) * U + r + 0.43);
        if (us >= 0.07 && V <= vr) return k;                       // the squeeze: ~ 87 % of the attempts
        if (k < 0. || (us < 0.013 && V > us)) continue;
        // ln(V alpha^-1 / (a / us^2 + b)) <= k ln r - r - ln k!, ln k! by Stirling with its tabulated tail (mp_binomial.h)
        const double lfact = 0.91893853320467274178 + (k + 0.5) * mp_log(k + 1.) - (k + 1.) + mp_stirling_tail(k);
        if (mp_log(V) + ln_inv_alpha - mp_log(a / (us * us) + b) <= -r + k * loglam - lfact) return k;
    }
    return floor(r);
}

// gamma.rs:17-20 with the scale parameterisation: (a - 1) ln x - x / b - ln Gamma(a) - a ln b
MP_HD double mp_gamma_logpdf(double x, double a, double b) {
    if (!(a > 0.) || !(b > 0.) || a == MP_INF || b == MP_INF || x != x) return MP_NAN;
    if (!(x > 0.) || x == MP_INF) return MP_NEG_INF;
    return (a - 1.) * mp_log(x) - x / b - mp_lgamma(a) - a * mp_log(b);
}
// Gamma(d + 1/3, 1) for d + 1/3 >= 1: G. Marsaglia and W. W. Tsang, "A simple method for generating gamma variables", ACM TOMS 26
// (2000).  An attempt takes one block for the normal deviate (the polar method's pair, mp_polar_attempt: a rejected pair ends the
// attempt) and, when 1 + c x > 0, the next block's first half for the acceptance uniform.
MP_HD double mp_gamma_mt(mp_site& st, double d) {
    const double c = 1. / mp_sqrt(9. * d);
    for (uint32_t att = 0; att < MP_DIST_MAX_ATTEMPTS; ++att) {
        double pu, pr;
        if (!mp_polar_attempt(st.next_block(), &pu, &pr)) continue;
        const double x = mp_std_normal_from_pair(pu, pr);
        double v = 1. + c * x;
        if (!(v > 0.)) continue;
        v = v * v * v;
        const double u = mp_u01(st.next_block().a);
        const double x2 = x * x;
        if (u < 1. - 0.0331 * (x2 * x2)) return d * v;
        if (mp_log(u) < 0.5 * x2 + d * (1. - v + mp_log(v))) return d * v;
    }
    return d;
}
// Gamma(a, 1): a >= 1 directly; a < 1 as Gamma(a + 1) U^(1/a), formed in log space (ln G + ln U / a, U = 1 - u01 in (0, 1]: the next
// block after the ones of Gamma(a + 1)) so that U^(1/a) does not underflow on its own.  mp_gamma_std_log_sample puts the variate in *x
// and returns its logarithm, which stays finite where the variate itself underflows to 0; mp_gamma_std_sample is its variate.
MP_HD double mp_gamma_std_log_sample(mp_site& st, double a, double* x) {
    if (a >= 1.) {
        *x = mp_gamma_mt(st, a - 1. / 3.);
        return mp_log(*x);
    }
    const double g = mp_gamma_mt(st, (a + 1.) - 1. / 3.);
    const double lu = mp_log(1. - mp_u01(st.next_block().a));
    const double l = mp_log(g) + lu / a;
    *x = mp_exp(l);
    return l;
}
MP_HD double mp_gamma_std_sample(mp_site& st, double a) {
    if (a >= 1.) return mp_gamma_mt(st, a - 1. / 3.);
    double x;
    mp_gamma_std_log_sample(st, a, &x);
    return x;
}
MP_HD double mp_gamma_sample(mp_site& st, double a, double b) {
    if (!(a > 0.) || !(b > 0.) || a == MP_INF || b == MP_INF) return MP_NAN;
    const double x = mp_gamma_std_sample(st, a) * b;
    return x < MP_MIN_NORMAL ? MP_MIN_NORMAL : x;
}

// beta.rs:17-21, in log form: ln Gamma(a + b) - ln Gamma(a) - ln Gamma(b) + (a - 1) ln x + (b - 1) log1p(-x)
MP_HD double mp_beta_logpdf(double x, double a, double b) {
    if (!(a > 0.) || !(b > 0.) || a == MP_INF || b == MP_INF || x != x) return MP_NAN;
    if (!(x > 0. && x < 1.)) return MP_NEG_INF;
    return mp_lgamma(a + b) - mp_lgamma(a) - mp_lgamma(b) + (a - 1.) * mp_log(x) + (b - 1.) * mp_log1p(-x);
}
// X / (X + Y), X ~ Gamma(a, 1) then Y ~ Gamma(b, 1) from the same stream.  Where that quotient cannot be formed (for small shapes
// both gammas can underflow to 0, and 0 / 0 would fail both clamps), the same pair in log form: 1 / (1 + exp(ln Y - ln X)).
MP_HD double mp_beta_sample(mp_site& st, double a, double b) {
    if (!(a > 0.) || !(b > 0.) || a == MP_INF || b == MP_INF) return MP_NAN;
    double X, Y;
    const double lX = mp_gamma_std_log_sample(st, a, &X);
    const double lY = mp_gamma_std_log_sample(st, b, &Y);
    const double s = X + Y;
    const double x = (X > 0. && Y > 0. && s < MP_INF) ? X / s : 1. / (1. + mp_exp(lY - lX));
    return x < MP_MIN_NORMAL ? MP_MIN_NORMAL : (x < 1. ? x : MP_ONE_MINUS_ULP);
}

// geometric.rs:16-19: ln((1 - p)^k p) = k log1p(-p) + ln p
MP_HD double mp_geometric_logpdf(double k, double p) {
    if (!(p > 0. && p < 1.)) return MP_NAN;
    if (!mp_is_count(k)) return MP_NEG_INF;
    return k * mp_log1p(-p) + mp_log(p);
}
// inversion: floor(ln U / log1p(-p)), U = 1 - u01 in (0, 1] (P(k >= n) = P(U <= (1 - p)^n) = (1 - p)^n); + 0. turns U = 1's -0 into 0
MP_HD double mp_geometric_sample(mp_site& st, double p) {
    if (!(p > 0. && p < 1.)) return MP_NAN;
    const double u = 1. - mp_u01(st.next_block().a);
    return floor(mp_log(u) / mp_log1p(-p)) + 0.;
}

// uniform.rs:36-54, bounds inclusive: -ln(b - a + 1) on a, ..., b
MP_HD bool mp_uniform_discrete_ok(double a, double b) { return a - floor(a) == 0. && b - floor(b) == 0. && a <= b; }
MP_HD double mp_uniform_discrete_logpdf(double x, double a, double b) {
    if (!mp_uniform_discrete_ok(a, b)) return MP_NAN;
    return (a <= x && x <= b && x - floor(x) == 0.) ? -mp_log(b - a + 1.) : MP_NEG_INF;
}
// uniform.rs:48-52: trunc(u01 (b - a + 1)) + a (u01 (b - a + 1) >= 0: trunc = floor)
MP_HD double mp_uniform_discrete_sample(mp_site& st, double a, double b) {
    if (!mp_uniform_discrete_ok(a, b)) return MP_NAN;
    const double x = floor(mp_u01(st.next_block().a) * (b - a + 1.)) + a;
    return x > b ? b : x;
}
