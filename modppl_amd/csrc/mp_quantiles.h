// mp_quantiles.h — on-device weighted quantiles of a particle cloud, of its smoothed paths and of the chains of a registered function
// (gfx950, wave64).
//
// ONE definition ("Quantiles"), restated in numpy and Python integers by tests/quantiles_ref.py and compared bit for bit.
// It is stated in integers only, so no order of summation has to be reproduced:
//
//   key(x)   the order-preserving 64-bit image of a double: b = bits(x); key = sign(b) ? ~b : b | 2^63
//   W_i      particle filter: m = max lw;  a_i = mom_weight(lw_i, m) (mp_moments.h);  l = ceil_log2(n);  S = 2^min(52, 63 - l);
//            W_i = a_i > 0 ? (uint64) trunc(a_i S) : 0       (a NaN compares false; a_i S is exact, only the truncation rounds)
//            MH chains, per site: W_i = the presence bit
//   A        sum of W_i (<= n S <= 2^63: an exact uint64 sum in any order)
//   tau(q)   max(1, ceil(q A)), q the exact rational value of the double: q = mant 2^-sh, the 117-bit product mant A shifted with a ceil
//   Q(q)     the smallest key k with sum_{key_i <= k} W_i >= tau(q), returned as its double (one of the stored values, its own bits)
//
// Method: a most-significant-digit radix select, 8 passes of 8 bits.  Pass p makes, for every selector (a quantile of a column; of a
// column at a time step; of a site), the histogram of digit p of the keys whose higher digits equal the selector's prefix — uint64 sums
// of W_i, per workgroup in LDS (ds_add_u64), the non-zero bins flushed to the global bins with 64-bit integer adds.  k_q_scan then
// picks, per selector, the first digit whose running sum reaches the target, appends it to the prefix and leaves the remaining target on
// the device for the next pass; after the last pass the prefix is the key.  Pass 0 has no prefix, so all quantiles of a column share
// ONE histogram (the bins of quantile 0) and the scan forms A and tau(q) from it.  No floating-point atomics, no sort, nothing of size
// n Q or n T, no host round trip between passes.  Every bin index is a digit (0 .. 255): in range by construction; a selector nothing
// reaches (A = 0: a site nobody holds, a NaN max) is clamped to the last bin and returns NaN.
//
// LDS: a workgroup holds Q_SEL_CHUNK = 16 histograms (32 KiB) whatever Q and d are: 16 / d quantiles of all d columns; grid row y takes
// the y-th such chunk of quantiles and reads the data again.  See DESIGN.md §5 for registers, LDS, launches and measured cost.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cmath>
#include <cstring>
#include "mp_math.h"

#define Q_THREADS 256
#define Q_BINS 256                  // 8-bit digits
#define Q_PASSES 8
#define Q_SEL_CHUNK 16              // histograms per workgroup
#define Q_MAX_Q 16                  // quantiles per call
#define Q_MAX_SEL (1 << 18)         // selectors per call (time steps * levels * columns): 0.5 GiB of bins; beyond it MP_ERR_UNSUPPORTED
#define Q_ROWS 8                    // elements per lane of the cloud and site kernels

typedef unsigned long long q_u64;

// the quantile levels as exact rationals: q = mant * 2^-sh, mant < 2^53 (host: q_make_spec)
struct q_spec { q_u64 mant[Q_MAX_Q]; int sh[Q_MAX_Q]; };
// where a call keeps its selectors: bins[nsel][256], the prefix, the remaining target and the total weight of each
struct q_bufs { q_u64* bins; q_u64* pre; q_u64* tgt; q_u64* tot; double* out; };

__device__ __forceinline__ q_u64 q_key(double x) {
    const q_u64 b = (q_u64)__double_as_longlong(x);
    return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ __forceinline__ double q_unkey(q_u64 k) {
    const q_u64 b = (k >> 63) ? (k & 0x7fffffffffffffffull) : ~k;
    return __longlong_as_double((long long)b);
}
// ceil(mant * A / 2^sh): the product in two 64-bit halves, shifted with a ceil (mant < 2^53, A <= 2^63; the result is <= A when q <= 1)
__device__ __forceinline__ q_u64 q_ceil_mul(q_u64 mant, int sh, q_u64 A) {
    const q_u64 hi = __umul64hi(mant, A), lo = mant * A;
    if (sh >= 128) return (hi | lo) ? 1ull : 0ull;
    if (sh >= 64) {
        const int s = sh - 64;
        const q_u64 fl = s ? (hi >> s) : hi;
        const bool rem = lo != 0 || (s && (hi & ((1ull << s) - 1)) != 0);
        return fl + (rem ? 1ull : 0ull);
    }
    if (sh == 0) return lo;
    return ((hi << (64 - sh)) | (lo >> sh)) + ((lo & ((1ull << sh) - 1)) ? 1ull : 0ull);
}

// LDS histograms of a workgroup: all zero / flush the non-zero ones of the first `count` to `dst` (and leave them zero)
__device__ __forceinline__ void q_hist_zero(q_u64* s_h) {
#pragma unroll
    for (int e = 0; e < Q_SEL_CHUNK * Q_BINS / Q_THREADS; ++e) s_h[e * Q_THREADS + threadIdx.x] = 0;
}
__device__ __forceinline__ void q_hist_flush(q_u64* s_h, int count, q_u64* __restrict__ dst) {
    for (int e = threadIdx.x; e < count; e += Q_THREADS) {
        const q_u64 v = s_h[e];
        if (v) { atomicAdd(&dst[e], v); s_h[e] = 0; }
    }
}
// one key into those of the histograms sel0, sel0 + stride, .. (nqc of them) whose prefix it carries
__device__ __forceinline__ void q_hist_add(q_u64* s_h, const q_u64* s_pre, int sel0, int stride, int nqc, int pass, int shift, q_u64 k, q_u64 w) {
    const int dg = (int)((k >> shift) & (Q_BINS - 1));
    const q_u64 high = pass ? (k >> (shift + 8)) : 0ull;
    for (int ql = 0; ql < nqc; ++ql) {
        const int sl = sel0 + ql * stride;
        if (pass == 0 || high == s_pre[sl]) atomicAdd(&s_h[sl * Q_BINS + dg], w);
    }
}

// ---- the scan: one workgroup per selector sel = (t Q + q) d + j; thread = digit ---------------------------------------------------------
// pass 0 reads the bins of quantile 0 of its column (shared), forms tot = A and the target tau(q); the thread whose digit is the first
// to reach the target appends it to the prefix and stores the remaining target (>= 1 always).  Nothing reaches it (A = 0): digit 255.
// (a template, as k_mom_tree is: both translation units that include this header instantiate it, and the linker keeps one)
template <int PASSES>
__global__ __launch_bounds__(Q_THREADS) void k_q_scan(int pass, int Q, int d, q_spec spec, q_bufs b) {
    __shared__ q_u64 s_w[Q_THREADS / 64];
    const q_u64 sel = blockIdx.x;
    const int q = (int)((sel / (q_u64)d) % (q_u64)Q);
    const q_u64 src = pass == 0 ? sel - (q_u64)q * d : sel;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const q_u64 v = b.bins[src * Q_BINS + threadIdx.x];
    q_u64 c = v;
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) {
        const q_u64 o = __shfl_up(c, s, 64);
        if (lane >= s) c += o;
    }
    if (lane == 63) s_w[wave] = c;
    __syncthreads();
    for (int w = 0; w < wave; ++w) c += s_w[w];
    const q_u64 total = (s_w[0] + s_w[1]) + (s_w[2] + s_w[3]);
    q_u64 target;
    if (pass == 0) {
        const q_u64 t = q_ceil_mul(spec.mant[q], spec.sh[q], total);
        target = t ? t : 1ull;
    } else {
        target = b.tgt[sel];
    }
    const q_u64 below = c - v;
    const bool hit = (c >= target && below < target) || (threadIdx.x == Q_BINS - 1 && c < target);
    if (hit) {
        const q_u64 key = ((pass == 0 ? 0ull : b.pre[sel]) << 8) | (q_u64)threadIdx.x;
        b.pre[sel] = key;
        b.tgt[sel] = target - below;
        const q_u64 A = pass == 0 ? total : b.tot[sel];
        if (pass == 0) b.tot[sel] = total;
        if (pass == PASSES - 1) b.out[sel] = A ? q_unkey(key) : __longlong_as_double(0x7ff8000000000000ll);
    }
}

#ifdef MP_QUANTILES_PF   // (mp_pf.hip, after mp_moments.h: mom_weight, mom_run, mom_load_row, mp_hist_event)
// W_i of the definition, once per call: the one n-sized scratch array
__global__ __launch_bounds__(Q_THREADS) void k_q_weights(unsigned long long n, const double* __restrict__ lw, const double* __restrict__ m_ptr, double S,
                                                         q_u64* __restrict__ W) {
    const unsigned long long i = (unsigned long long)blockIdx.x * Q_THREADS + threadIdx.x;
    if (i >= n) return;
    const double a = mom_weight(lw[i], *m_ptr);
    W[i] = (a > 0.) ? (q_u64)(a * S) : 0ull;
}

// ---- the cloud: sel = q d + j.  Workgroup (x, y): rows [x 2048, x 2048 + 2048), quantiles [y QC, y QC + QC) of all DP columns -----------
template <int DP>
__global__ __launch_bounds__(Q_THREADS) void k_q_hist_pf(unsigned long long n, const double* __restrict__ x, const q_u64* __restrict__ W, int pass, int nq,
                                                         q_bufs b) {
    constexpr int QC = Q_SEL_CHUNK / DP;
    __shared__ q_u64 s_h[Q_SEL_CHUNK * Q_BINS];
    __shared__ q_u64 s_pre[Q_SEL_CHUNK];
    const int q0 = blockIdx.y * QC;
    const int nqc = min(QC, nq - q0);
    const int shift = 56 - 8 * pass;
    q_hist_zero(s_h);
    if ((int)threadIdx.x < nqc * DP) s_pre[threadIdx.x] = pass ? b.pre[q0 * DP + threadIdx.x] : 0ull;
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < Q_ROWS; ++r) {
        const unsigned long long i = ((unsigned long long)blockIdx.x * Q_ROWS + r) * Q_THREADS + threadIdx.x;
        if (i >= n) break;
        const q_u64 w = W[i];
        if (!w) continue;
        double v[DP];
        mom_load_row<DP>(x + i * DP, v);
#pragma unroll
        for (int j = 0; j < DP; ++j) q_hist_add(s_h, s_pre, j, DP, nqc, pass, shift, q_key(v[j]), w);
    }
    __syncthreads();
    q_hist_flush(s_h, nqc * DP * Q_BINS, b.bins + (q_u64)q0 * DP * Q_BINS);
}

// ---- the smoothed paths: sel = (t Q + q) d + j over v_ij(t) = x_t[anc_i(t)] -------------------------------------------------------------
// The walk of k_path_mom1 (mp_moments.h): a lane keeps R slots' weights and current ancestors in registers and reads the event log from
// the newest event back; a resample maps anc <- parents[anc], a step is time t read at anc.  The log is uniform, so every branch on it
// and both barriers of a step are taken by the whole workgroup.  Slots past n gather row 0 (in bounds) and carry W = 0: never added.
// Per step: the prefixes of time t -> LDS, barrier, histogram, barrier, flush (which leaves the LDS bins zero for the next step).
template <int DP>
__global__ __launch_bounds__(Q_THREADS) void k_q_hist_path(unsigned long long n, int n_events, int T, const mp_hist_event* __restrict__ ev,
                                                           const q_u64* __restrict__ W, int pass, int nq, int Q, q_bufs b) {
    constexpr int R = mom_run<DP>::R;
    constexpr int QC = Q_SEL_CHUNK / DP;
    __shared__ q_u64 s_h[Q_SEL_CHUNK * Q_BINS];
    __shared__ q_u64 s_pre[Q_SEL_CHUNK];
    const int q0 = blockIdx.y * QC;
    const int nqc = min(QC, nq - q0);
    const int shift = 56 - 8 * pass;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * Q_THREADS + threadIdx.x) * R;
    q_u64 w[R];
    uint32_t anc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        w[r] = (i0 + r < n) ? W[i0 + r] : 0ull;
        anc[r] = (i0 + r < n) ? (uint32_t)(i0 + r) : 0u;
    }
    q_hist_zero(s_h);
    int tt = T;
    for (int e = n_events - 1; e >= 0; --e) {
        const void* buf = ev[e].buf;
        if (ev[e].kind == 1) {
            const uint32_t* parents = static_cast<const uint32_t*>(buf);
#pragma unroll
            for (int r = 0; r < R; ++r) anc[r] = parents[anc[r]];
            continue;
        }
        --tt;
        const q_u64 sel0 = ((q_u64)tt * Q + q0) * DP;
        if ((int)threadIdx.x < nqc * DP) s_pre[threadIdx.x] = pass ? b.pre[sel0 + threadIdx.x] : 0ull;
        const double* x = static_cast<const double*>(buf);
        double v[R][DP];
#pragma unroll
        for (int r = 0; r < R; ++r) mom_load_row<DP>(x + (unsigned long long)anc[r] * DP, v[r]);
        __syncthreads();
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if (w[r]) {
#pragma unroll
                for (int j = 0; j < DP; ++j) q_hist_add(s_h, s_pre, j, DP, nqc, pass, shift, q_key(v[r][j]), w[r]);
            }
        }
        __syncthreads();
        q_hist_flush(s_h, nqc * DP * Q_BINS, b.bins + sel0 * Q_BINS);
    }
}
#endif   // MP_QUANTILES_PF

#ifdef MP_QUANTILES_MH   // (mp_mh.hip)
// ---- MH chains of a registered function: vals[site][chain], present[word][chain]; grid row = site s; sel = q ns + s; W_i = presence ------
__global__ __launch_bounds__(Q_THREADS) void k_q_hist_site(unsigned long long n, const double* __restrict__ vals, const uint32_t* __restrict__ present,
                                                           int pass, int nq, q_bufs b) {
    __shared__ q_u64 s_h[Q_SEL_CHUNK * Q_BINS];
    __shared__ q_u64 s_pre[Q_SEL_CHUNK];
    const unsigned int s = blockIdx.y, ns = gridDim.y;
    const int shift = 56 - 8 * pass;
    q_hist_zero(s_h);
    if ((int)threadIdx.x < nq) s_pre[threadIdx.x] = pass ? b.pre[(q_u64)threadIdx.x * ns + s] : 0ull;
    __syncthreads();
#pragma unroll 2
    for (int r = 0; r < Q_ROWS; ++r) {
        const unsigned long long i = ((unsigned long long)blockIdx.x * Q_ROWS + r) * Q_THREADS + threadIdx.x;
        if (i >= n) break;
        if (!((present[(unsigned long long)(s >> 5) * n + i] >> (s & 31u)) & 1u)) continue;
        q_hist_add(s_h, s_pre, 0, 1, nq, pass, shift, q_key(vals[(unsigned long long)s * n + i]), 1ull);
    }
    __syncthreads();
    for (int q = 0; q < nq; ++q) q_hist_flush(s_h + q * Q_BINS, Q_BINS, b.bins + ((q_u64)q * ns + s) * Q_BINS);
}
#endif   // MP_QUANTILES_MH

// ---- host side --------------------------------------------------------------------------------------------------------------------------
// the levels of a call as exact rationals; false for a count outside [1, 16], a NaN or a level outside [0, 1]
static inline bool q_make_spec(const double* qs, int32_t n_q, q_spec& spec) {
    if (n_q < 1 || n_q > Q_MAX_Q) return false;
    spec = q_spec{};
    for (int32_t k = 0; k < n_q; ++k) {
        const double q = qs[k];
        if (!(q >= 0. && q <= 1.)) return false;
        int e = 0;
        const double f = std::frexp(q, &e);   // q = f 2^e, f in [0.5, 1) or 0
        spec.mant[k] = (q_u64)std::ldexp(f, 53);
        spec.sh[k] = 53 - e;                  // (e <= 1: sh >= 52)
    }
    return true;
}
static inline int q_ceil_log2(unsigned long long n) {
    int l = 0;
    while (l < 64 && (1ull << l) < n) ++l;
    return l;
}
// S of the definition for a cloud of n
static inline double q_scale(unsigned long long n) { return std::ldexp(1.0, std::min(52, 63 - q_ceil_log2(n))); }

// the eight passes over nsel selectors (Q quantiles of d columns, per time step), all enqueued on `stream`:
// hist(pass, nq, bufs) launches the histogram of one pass for quantiles 0 .. nq - 1 (nq = 1 in pass 0: the shared histogram)
template <class LaunchHist>
static inline hipError_t q_select(hipStream_t stream, const q_bufs& b, size_t nsel, int Q, int d, const q_spec& spec, LaunchHist&& hist) {
    for (int pass = 0; pass < Q_PASSES; ++pass) {
        const hipError_t e = hipMemsetAsync(b.bins, 0, sizeof(q_u64) * nsel * Q_BINS, stream);
        if (e != hipSuccess) return e;
        hist(pass, pass == 0 ? 1 : Q, b);
        hipLaunchKernelGGL(k_q_scan<Q_PASSES>, dim3((unsigned)nsel), dim3(Q_THREADS), 0, stream, pass, Q, d, spec, b);
    }
    return hipGetLastError();
}
