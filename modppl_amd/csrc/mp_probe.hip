// mp_probe.hip — device self-test probes (include/modppl_hip_probe.h).
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/modppl_hip.h"
#include "../../include/modppl_hip_probe.h"
#include <vector>

#include "mp_dists.h"
#include "mp_err.h"
#include "mp_hip_own.h"
#include "mp_linalg.h"

__global__ void k_probe_math(int op, const double* a, const double* b, const double* c, long long n, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double r = 0.;
    switch (op) {
    case MP_PROBE_EXP: r = mp_exp(a[i]); break;
    case MP_PROBE_LOG: r = mp_log(a[i]); break;
    case MP_PROBE_SQRT: r = mp_sqrt(a[i]); break;
    case MP_PROBE_DIV: r = a[i] / b[i]; break;
    case MP_PROBE_NORMAL_LOGPDF: r = mp_normal_logpdf(a[i], b[i], c[i]); break;
    case MP_PROBE_NORMAL_LOGPDF_H: r = mp_normal_logpdf_h(a[i], b[i], c[i], mp_log(c[i]), mp_rcp_hoist(c[i])); break;
    case MP_PROBE_DIV_HOISTED: r = mp_rcp_hoistable(b[i]) ? mp_div_hoisted(a[i], b[i], 1.0 / b[i]) : a[i] / b[i]; break;
    case MP_PROBE_SIN: r = mp_sin(a[i]); break;
    case MP_PROBE_COS: r = mp_cos(a[i]); break;
    case MP_PROBE_ATAN2: r = mp_atan2(a[i], b[i]); break;
    }
    out[i] = r;
}
__global__ void k_probe_normal(uint32_t k0, uint32_t k1, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, double mu, double sd,
                               long long n, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mp_stream s;
    s.k0 = k0; s.k1 = k1; s.slot = slot0 + (uint32_t)i; s.step = step;
    mp_site st(s, domain, site);
    out[i] = mp_normal_sample(st, mu, sd);
}
__global__ void k_probe_u01(uint32_t k0, uint32_t k1, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, uint32_t attempt,
                            long long n, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mp_u64x2 b = mp_philox4x32_10(slot0 + (uint32_t)i, step, (domain << 16) | site, attempt, k0, k1);
    out[2 * i] = mp_u01(b.a);
    out[2 * i + 1] = mp_u01(b.b);
}

// the count and positive-real distributions of mp_dists.h (dist / op: include/modppl_hip_probe.h mp_probe_dist)
__global__ void k_probe_dist(int dist, int op, const double* x, const double* p0, const double* p1, long long n, uint32_t k0, uint32_t k1,
                             uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const double a = p0 ? p0[i] : 0., b = p1 ? p1[i] : 0.;
    double r = 0.;
    if (op == 0) {
        const double v = x[i];
        switch (dist) {
        case MP_PROBE_DIST_POISSON: r = mp_poisson_logpdf(v, a); break;
        case MP_PROBE_DIST_GAMMA: r = mp_gamma_logpdf(v, a, b); break;
        case MP_PROBE_DIST_BETA: r = mp_beta_logpdf(v, a, b); break;
        case MP_PROBE_DIST_GEOMETRIC: r = mp_geometric_logpdf(v, a); break;
        case MP_PROBE_DIST_UNIFORM_DISCRETE: r = mp_uniform_discrete_logpdf(v, a, b); break;
        case MP_PROBE_DIST_LGAMMA: r = mp_lgamma(v); break;
        case MP_PROBE_DIST_LOG1P: r = mp_log1p(v); break;
        }
    } else {
        mp_stream s;
        s.k0 = k0; s.k1 = k1; s.slot = slot0 + (uint32_t)i; s.step = step;
        mp_site st(s, domain, site);
        switch (dist) {
        case MP_PROBE_DIST_POISSON: r = mp_poisson_sample(st, a); break;
        case MP_PROBE_DIST_GAMMA: r = mp_gamma_sample(st, a, b); break;
        case MP_PROBE_DIST_BETA: r = mp_beta_sample(st, a, b); break;
        case MP_PROBE_DIST_GEOMETRIC: r = mp_geometric_sample(st, a); break;
        case MP_PROBE_DIST_UNIFORM_DISCRETE: r = mp_uniform_discrete_sample(st, a, b); break;
        }
    }
    out[i] = r;
}

// mvnormal (mvnormal.rs:14-38) of dimension k <= MP_PROBE_MAX_K with the covariance constants hoisted by the host (mp_linalg.h;
// the reference takes any k; model sites are compiled for k <= 16, this general-k form serves the distribution on its own):
#define MP_PROBE_MAX_K 64
// out[i] = logpdf(x_i; mu, cov) in the reference's operation order (chain = 0) or as the matrix cores' fma chain (chain = 1)
__global__ void k_probe_mvnormal_logpdf(int k, int chain, const double* x, const double* mu, const double* cov_inv, double ln_det, long long n, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double c[MP_PROBE_MAX_K];
    for (int a = 0; a < k; ++a) c[a] = x[i * k + a] - mu[a];
    double maha = 0.;
    for (int j = 0; j < k; ++j) {
        double r = 0.;
        for (int a = 0; a < k; ++a) r = chain ? fma(c[a], cov_inv[a * k + j], r) : r + c[a] * cov_inv[a * k + j];
        maha = chain ? fma(r, c[j], maha) : maha + r * c[j];
    }
    out[i] = -((double)k * MP_LN_2PI_CANON + ln_det + maha) / 2.;
}
// out[i][0..k) = transform * z + mu, z_j ~ normal(0, 1) in index order from the stream of (slot0 + i, step, domain, site)
__global__ void k_probe_mvnormal_sample(int k, int chain, uint32_t k0, uint32_t k1, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site,
                                        const double* mu, const double* transform, long long n, double* out) {
    const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mp_stream s;
    s.k0 = k0; s.k1 = k1; s.slot = slot0 + (uint32_t)i; s.step = step;
    mp_site st(s, domain, site);
    double z[MP_PROBE_MAX_K];
    for (int j = 0; j < k; ++j) z[j] = mp_normal_sample(st, 0., 1.);
    for (int a = 0; a < k; ++a) {
        double acc = 0.;
        for (int j = 0; j < k; ++j) acc = chain ? fma(transform[a * k + j], z[j], acc) : acc + transform[a * k + j] * z[j];
        out[i * k + a] = acc + mu[a];
    }
}

// One v_mfma_f64_16x16x4_f64: D[16][16] = A[16][4] * B[4][16] + C[16][16] (row-major host arrays), by one wave.
// Operand lanes (cdna_hip_programming.md §3): A lane l = A[l & 15][l >> 4]; B lane l = B[l >> 4][l & 15];
// C/D lane l, register r = [(l >> 4) + 4 r][l & 15].
typedef double mp_f64x4 __attribute__((ext_vector_type(4)));
__global__ void k_probe_mfma_f64(const double* A, const double* B, const double* C, double* D) {
    const int l = threadIdx.x;
    const double a = A[(l & 15) * 4 + (l >> 4)];
    const double b = B[(l >> 4) * 16 + (l & 15)];
    mp_f64x4 c;
    for (int r = 0; r < 4; ++r) c[r] = C[((l >> 4) + 4 * r) * 16 + (l & 15)];
    const mp_f64x4 d = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[((l >> 4) + 4 * r) * 16 + (l & 15)] = d[r];
}

extern "C" {

int32_t mp_probe_math(int32_t op, const double* a, const double* b, const double* c, int64_t n, double* out, int32_t device) {
    if (op < MP_PROBE_EXP || op > MP_PROBE_ATAN2 || !a || !out || n < 1) return MP_ERR_INVALID_ARG;
    mp_dev<double> da, db, dc, dout;
    const size_t bytes = sizeof(double) * (size_t)n;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(da, bytes / sizeof(double))); HIPCK(mp_hipMalloc(db, bytes / sizeof(double))); HIPCK(mp_hipMalloc(dc, bytes / sizeof(double))); HIPCK(mp_hipMalloc(dout, bytes / sizeof(double)));
    HIPCK(hipMemcpy(da, a, bytes, hipMemcpyHostToDevice));
    if (b) HIPCK(hipMemcpy(db, b, bytes, hipMemcpyHostToDevice)); else HIPCK(hipMemset(db, 0, bytes));
    if (c) HIPCK(hipMemcpy(dc, c, bytes, hipMemcpyHostToDevice)); else HIPCK(hipMemset(dc, 0, bytes));
    hipLaunchKernelGGL(k_probe_math, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, op, da, db, dc, (long long)n, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return MP_OK;
}

int32_t mp_probe_normal_sample(uint64_t seed, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, double mu, double sd,
                               int64_t n, double* out, int32_t device) {
    mp_dev<double> dout;
    const size_t bytes = sizeof(double) * (size_t)n;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(dout, bytes / sizeof(double)));
    hipLaunchKernelGGL(k_probe_normal, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), slot0, step,
                       domain, site, mu, sd, (long long)n, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return MP_OK;
}

int32_t mp_probe_u01(uint64_t seed, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, uint32_t attempt, int64_t n,
                     double* out, int32_t device) {
    mp_dev<double> dout;
    const size_t bytes = sizeof(double) * 2 * (size_t)n;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(dout, bytes / sizeof(double)));
    hipLaunchKernelGGL(k_probe_u01, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (uint32_t)seed, (uint32_t)(seed >> 32), slot0, step,
                       domain, site, attempt, (long long)n, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return MP_OK;
}

int32_t mp_probe_mvnormal(int32_t k, int32_t chain, const double* x, const double* mu, const double* cov, int64_t n, double* logpdf_out,
                          uint64_t seed, uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, double* sample_out, int32_t device) {
    if (k < 1 || k > MP_PROBE_MAX_K || !mu || !cov || n < 1) return MP_ERR_INVALID_ARG;
    const std::vector<double> c(cov, cov + (size_t)k * k);
    std::vector<double> inv, T;
    const double det = mp_host_det(c, k);
    mp_dev<double> dx, dmu, dm, dout;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(dmu, k)); HIPCK(mp_hipMalloc(dm, (size_t)k * k)); HIPCK(mp_hipMalloc(dout, (size_t)n * k));
    HIPCK(hipMemcpy(dmu, mu, sizeof(double) * k, hipMemcpyHostToDevice));
    if (logpdf_out) {
        if (!x || !mp_host_inverse(c, k, inv)) return MP_ERR_INVALID_ARG;   // try_inverse().unwrap() panics (mvnormal.rs:18)
        HIPCK(mp_hipMalloc(dx, (size_t)n * k));
        HIPCK(hipMemcpy(dx, x, sizeof(double) * (size_t)n * k, hipMemcpyHostToDevice));
        HIPCK(hipMemcpy(dm, inv.data(), sizeof(double) * k * k, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_probe_mvnormal_logpdf, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, k, chain, dx, dmu, dm, mp_log(det), (long long)n, dout);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpy(logpdf_out, dout, sizeof(double) * (size_t)n, hipMemcpyDeviceToHost));
    }
    if (sample_out) {
        mp_host_mvnormal_transform(c, k, T);   // Cholesky factor, or the eigen form when there is none (mvnormal.rs:26-34)
        HIPCK(hipMemcpy(dm, T.data(), sizeof(double) * k * k, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_probe_mvnormal_sample, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, k, chain, (uint32_t)seed, (uint32_t)(seed >> 32), slot0, step,
                           domain, site, dmu, dm, (long long)n, dout);
        HIPCK(hipGetLastError());
        HIPCK(hipMemcpy(sample_out, dout, sizeof(double) * (size_t)n * k, hipMemcpyDeviceToHost));
    }
    return MP_OK;
}

int32_t mp_probe_dist(int32_t dist, int32_t op, const double* x, const double* p0, const double* p1, int64_t n, uint64_t seed, uint32_t slot0,
                      uint32_t step, uint32_t domain, uint32_t site, double* out, int32_t device) {
    if (dist < 0 || dist > MP_PROBE_DIST_LOG1P || (op != 0 && op != 1) || (op == 0 && !x) || (op == 1 && dist > MP_PROBE_DIST_UNIFORM_DISCRETE) ||
        n < 1 || !out)
        return MP_ERR_INVALID_ARG;
    mp_dev<double> dx, dp0, dp1, dout;
    const size_t bytes = sizeof(double) * (size_t)n;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(dout, bytes / sizeof(double)));
    if (op == 0) { HIPCK(mp_hipMalloc(dx, bytes / sizeof(double))); HIPCK(hipMemcpy(dx, x, bytes, hipMemcpyHostToDevice)); }
    if (p0) { HIPCK(mp_hipMalloc(dp0, bytes / sizeof(double))); HIPCK(hipMemcpy(dp0, p0, bytes, hipMemcpyHostToDevice)); }
    if (p1) { HIPCK(mp_hipMalloc(dp1, bytes / sizeof(double))); HIPCK(hipMemcpy(dp1, p1, bytes, hipMemcpyHostToDevice)); }
    hipLaunchKernelGGL(k_probe_dist, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, (int)dist, (int)op, dx, dp0, dp1, (long long)n,
                       (uint32_t)seed, (uint32_t)(seed >> 32), slot0, step, domain, site, dout);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(out, dout, bytes, hipMemcpyDeviceToHost));
    return MP_OK;
}

int32_t mp_probe_mfma_f64(const double* A16x4, const double* B4x16, const double* C16x16, double* D16x16, int32_t device) {
    mp_dev<double> da, db, dc, dd;
    HIPCK(hipSetDevice(device));
    HIPCK(mp_hipMalloc(da, 64)); HIPCK(mp_hipMalloc(db, 64)); HIPCK(mp_hipMalloc(dc, 256)); HIPCK(mp_hipMalloc(dd, 256));
    HIPCK(hipMemcpy(da, A16x4, sizeof(double) * 64, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(db, B4x16, sizeof(double) * 64, hipMemcpyHostToDevice));
    HIPCK(hipMemcpy(dc, C16x16, sizeof(double) * 256, hipMemcpyHostToDevice));
    hipLaunchKernelGGL(k_probe_mfma_f64, dim3(1), dim3(64), 0, 0, da, db, dc, dd);
    HIPCK(hipGetLastError());
    HIPCK(hipMemcpy(D16x16, dd, sizeof(double) * 256, hipMemcpyDeviceToHost));
    return MP_OK;
}

}  // extern "C"
