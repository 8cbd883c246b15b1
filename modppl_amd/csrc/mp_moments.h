// mp_moments.h — on-device weighted moments of a particle cloud and of the chains of a registered function (gfx950, wave64).
//
// ONE definition ("Moments"), restated in numpy by tests/moments_ref.py and compared bit for bit:
//
//   TREE(v[0..n)):  pad v with +0.0 up to the next power of two; repeat v <- v[0::2] + v[1::2] until one element is left.
//                   IEEE fp64, no contraction (-ffp-contract=off), indices are GLOBAL slot / chain ids.
//
// a + b == b + a and x + (+0.0) == x (up to the sign of a zero), so the tree can be cut at any aligned power-of-two subtree:
//   lane        an aligned run of R consecutive slots, pairwise in registers                       (mom_lane_tree)
//   wave        xor butterfly over the 64 lanes: lane l and lane l ^ s add the same two numbers     (mom_block_tree)
//   workgroup   the 4 waves through LDS: (w0 + w1) + (w2 + w3) -> ONE partial per aligned run of 256 R slots
//   launch      k_mom_tree sums aligned runs of 1024 partials the same way, repeated until one value is left
// No floating-point atomics, no ticket: the combine over partials is a further launch on the same stream, so the result is a pure
// function of the stored values on any launch geometry.  The max of the log-weights is exact in any order and takes the same kernels.
//
// Particle filter (mp_pf_moments): m = max lw;  a_i = lw_i == -inf ? 0 : mp_exp(lw_i - m);  A = TREE(a);
//   mean_j = TREE(a_i x_ij) / A;   c_ij = x_ij - mean_j;   cov_jk = TREE(a_i (c_ij c_ik)) / A   (k <= j; the other half is a copy)
// Three passes (max, first moment, centred second moment); no one-pass covariance.
// MH chains of a registered function (mp_mh_site_moments), per site s with presence bit p_i:
//   count_s = TREE(p_i) (a sum of 0.0 / 1.0: exact);  mean_s = TREE(p_i ? v_i : +0.0) / count_s;
//   var_s = TREE(p_i ? (v_i - mean_s)^2 : +0.0) / count_s      (selected, never multiplied: a stale NaN in an absent slot cannot leak)
//
// Path moments (mp_pf_path_moments; DESIGN.md §4, "Path moments"): the same weights and trees over v_i(t) = x_t[anc_i(t)], the state of
//   slot i's ancestor at time t along the recorded history, for every t: mean_tj = TREE(a_i v_ij(t)) / A;
//   var_tj = TREE(a_i (v_ij(t) - mean_tj)^2) / A;  distinct_t = |{anc_i(t)}| (a bitmap and a popcount: integers).
//
// Registers (gfx950 code object, kernel-resource-usage): k_mom_pf2<16> holds c[R = 4][16] and a[4] per lane and walks the 136 (j, k)
// pairs one at a time — one accumulator tree per pair, never 136 live accumulators; see DESIGN.md §5 for the VGPR / scratch figures.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>
#include <type_traits>
#include "mp_hip_own.h"
#include "mp_math.h"

#define MOM_THREADS 256
#define MOM_WAVES (MOM_THREADS / 64)
#define MOM_TREE_R 4                          // k_mom_tree: inputs per lane
#define MOM_TREE_RUN (MOM_THREADS * MOM_TREE_R)   // ... and per workgroup
#define MOM_MAX_DIM 16                        // the widest compiled model
#define MOM_MAX_COLS (MOM_MAX_DIM * (MOM_MAX_DIM + 1) / 2)

struct mom_add { __device__ __forceinline__ static double id() { return 0.; } __device__ __forceinline__ static double op(double a, double b) { return a + b; } };
// (a NaN wins from either side, so the max stays a function of the set of values: a NaN log-weight gives m = NaN, as numpy's max does)
struct mom_max { __device__ __forceinline__ static double id() { return -MP_INF; } __device__ __forceinline__ static double op(double a, double b) { return (a > b || a != a) ? a : b; } };

// slots per lane of the level-0 kernels for a state width D (the compiled models' 1, 2, 4 or 16): R * D <= 64 doubles of centred state per lane
template <int D> struct mom_run { static constexpr int R = D <= 4 ? 8 : 4; };

// TREE of the lane's R values (R a power of two), in registers
template <class Op, int R>
__device__ __forceinline__ double mom_lane_tree(double (&t)[R]) {
#pragma unroll
    for (int w = R; w > 1; w >>= 1) {
#pragma unroll
        for (int i = 0; i < w / 2; ++i) t[i] = Op::op(t[2 * i], t[2 * i + 1]);
    }
    return t[0];
}
// the wave's subtree: after step s every lane holds the sum of its aligned group of 2 s lanes (both partners add the same two numbers)
template <class Op>
__device__ __forceinline__ double mom_wave_tree(double v) {
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) v = Op::op(v, __shfl_xor(v, s, 64));
    return v;
}
// column `col` of a workgroup: every wave leaves its subtree in s_part[col][wave]; after ONE __syncthreads mom_block_combine closes the tree
template <class Op>
__device__ __forceinline__ void mom_block_put(double v, int col, double* s_part) {
    v = mom_wave_tree<Op>(v);
    if ((threadIdx.x & 63) == 0) s_part[col * MOM_WAVES + (threadIdx.x >> 6)] = v;
}
template <class Op>
__device__ __forceinline__ double mom_block_combine(int col, const double* s_part) {
    const double* p = s_part + col * MOM_WAVES;
    return Op::op(Op::op(p[0], p[1]), Op::op(p[2], p[3]));
}

// ---- the combine over partials: out[c][b] = TREE(in[c][1024 b .. 1024 b + 1024)), missing entries = the identity -------------------
template <class Op>
__global__ __launch_bounds__(MOM_THREADS) void k_mom_tree(const double* __restrict__ in, unsigned long long n_in, double* __restrict__ out, unsigned long long n_out) {
    __shared__ double s_part[MOM_WAVES];
    const unsigned long long c = blockIdx.y;
    const unsigned long long i0 = (unsigned long long)blockIdx.x * MOM_TREE_RUN + (unsigned long long)threadIdx.x * MOM_TREE_R;
    double t[MOM_TREE_R];
#pragma unroll
    for (int r = 0; r < MOM_TREE_R; ++r) t[r] = (i0 + r < n_in) ? in[c * n_in + i0 + r] : Op::id();
    mom_block_put<Op>(mom_lane_tree<Op, MOM_TREE_R>(t), 0, s_part);
    __syncthreads();
    if (threadIdx.x == 0) out[c * n_out + blockIdx.x] = mom_block_combine<Op>(0, s_part);
}

#ifdef MP_MOMENTS_PF   // (mp_pf.hip)
// ---- pass 0: partial maxima of a column of n doubles -------------------------------------------------------------------------------
__global__ __launch_bounds__(MOM_THREADS) void k_mom_max0(unsigned long long n, const double* __restrict__ lw, double* __restrict__ out) {
    constexpr int R = 8;
    __shared__ double s_part[MOM_WAVES];
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = (i0 + r < n) ? lw[i0 + r] : -MP_INF;
    mom_block_put<mom_max>(mom_lane_tree<mom_max, R>(t), 0, s_part);
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = mom_block_combine<mom_max>(0, s_part);
}

__device__ __forceinline__ double mom_weight(double lw, double m) { return lw == -MP_INF ? 0. : mp_exp(lw - m); }

// ---- particle filter, pass 1: out[0][b] = subtree of a_i, out[1 + j][b] = subtree of a_i x_ij; nb = gridDim.x -------------------------
// DP = dim_state: a lane's R rows are R * DP consecutive doubles at a compile-time stride (wide loads).
template <int DP>
__global__ __launch_bounds__(MOM_THREADS) void k_mom_pf1(unsigned long long n, const double* __restrict__ x, const double* __restrict__ lw,
                                                         const double* __restrict__ m_ptr, double* __restrict__ out) {
    constexpr int R = mom_run<DP>::R;
    __shared__ double s_part[(DP + 1) * MOM_WAVES];
    constexpr int d = DP;
    const double m = *m_ptr;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double a[R], xv[R][DP], t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < DP; ++j) xv[r][j] = (i0 + r < n && j < d) ? x[(i0 + r) * (unsigned long long)d + j] : 0.;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = (i0 + r < n) ? mom_weight(lw[i0 + r], m) : 0.;
#pragma unroll
    for (int r = 0; r < R; ++r) t[r] = a[r];
    mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), 0, s_part);
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        if (j < d) {
#pragma unroll
            for (int r = 0; r < R; ++r) t[r] = (i0 + r < n) ? a[r] * xv[r][j] : 0.;
            mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), 1 + j, s_part);
        }
    }
    __syncthreads();
    if ((int)threadIdx.x <= d) out[(unsigned long long)threadIdx.x * gridDim.x + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, s_part);
}

// ---- particle filter, pass 2: column j (j + 1) / 2 + k (k <= j) = subtree of a_i ((x_ij - mean_j) (x_ik - mean_k)) ------------------------
// sums = the closed trees of pass 1 ({A, S_0 .. S_{d-1}}); every lane forms mean_j = S_j / A itself (same bits), workgroup 0 stores it.
template <int DP>
__global__ __launch_bounds__(MOM_THREADS) void k_mom_pf2(unsigned long long n, const double* __restrict__ x, const double* __restrict__ lw,
                                                         const double* __restrict__ m_ptr, const double* __restrict__ sums, double* __restrict__ mean_out,
                                                         double* __restrict__ out) {
    constexpr int R = mom_run<DP>::R;
    __shared__ double s_part[(DP * (DP + 1) / 2) * MOM_WAVES];
    constexpr int d = DP;
    const double m = *m_ptr;
    const double A = sums[0];
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double a[R], c[R][DP], t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
#pragma unroll
        for (int j = 0; j < DP; ++j) c[r][j] = (i0 + r < n && j < d) ? x[(i0 + r) * (unsigned long long)d + j] : 0.;
    }
#pragma unroll
    for (int r = 0; r < R; ++r) a[r] = (i0 + r < n) ? mom_weight(lw[i0 + r], m) : 0.;
#pragma unroll
    for (int j = 0; j < DP; ++j) {
        if (j < d) {
            const double mean = sums[1 + j] / A;
            if (blockIdx.x == 0 && threadIdx.x == 0) mean_out[j] = mean;
#pragma unroll
            for (int r = 0; r < R; ++r) c[r][j] = (i0 + r < n) ? c[r][j] - mean : 0.;
        }
    }
#pragma unroll
    for (int j = 0; j < DP; ++j) {
#pragma unroll
        for (int k = 0; k <= j; ++k) {
            if (j < d) {
#pragma unroll
                for (int r = 0; r < R; ++r) t[r] = (i0 + r < n) ? a[r] * (c[r][j] * c[r][k]) : 0.;
                mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), j * (j + 1) / 2 + k, s_part);
            }
        }
    }
    __syncthreads();
    const int ncols = d * (d + 1) / 2;
    if ((int)threadIdx.x < ncols) out[(unsigned long long)threadIdx.x * gridDim.x + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, s_part);
}

// ---- path moments (mp_pf_path_moments): the same trees over v_i(t) = x_t[anc_i(t)], gathered along the recorded ancestry ------------------
// A lane owns the aligned run of R slots k_mom_pf1 gives it (so the tree is cut where that kernel cuts it), keeps their weights and
// their current ancestor slots in registers and walks the event log (mp_hist_event, mp_pf_kernels.h) from the newest event back, as
// k_trajectories does: a resample maps anc <- parents[anc], a step is time t read at anc.  The log is uniform, so its entries are
// scalar loads and every branch on them is taken by the whole grid.  One partial per (t, j, workgroup): out[(t d + j) nb + b]; the
// LDS partials alternate between two buffers, so a step event costs one __syncthreads (a wave that runs ahead writes the buffer
// nobody reads before the next barrier).  Slots past n gather row 0 (in bounds) and are selected to +0.0, never multiplied.
template <int DP>
__device__ __forceinline__ void mom_load_row(const double* __restrict__ p, double (&v)[DP]) {
    if constexpr (DP == 1) {
        v[0] = p[0];
    } else {   // rows of an even width start on 16 bytes (the history buffers are 256-byte aligned): dwordx4 loads
        const double2* q = reinterpret_cast<const double2*>(p);
#pragma unroll
        for (int j = 0; j < DP / 2; ++j) { const double2 w = q[j]; v[2 * j] = w.x; v[2 * j + 1] = w.y; }
    }
}

// pass 1: out[(t d + j) nb + b] = subtree of a_i v_ij(t), out[T d nb + b] = subtree of a_i.  bitmap (or null): bit anc_i(t) of row t
// of [T][words] u32 is set for every slot i < n — integer ORs, exact in any order (k_path_distinct counts them).
template <int DP>
__global__ __launch_bounds__(MOM_THREADS) void k_path_mom1(unsigned long long n, int n_events, int T, const mp_hist_event* __restrict__ ev,
                                                           const double* __restrict__ lw, const double* __restrict__ m_ptr, double* __restrict__ out,
                                                           uint32_t* __restrict__ bitmap, unsigned long long words) {
    constexpr int R = mom_run<DP>::R;
    __shared__ double s_part[2][DP * MOM_WAVES];
    __shared__ double s_a[MOM_WAVES];
    const double m = *m_ptr;
    const unsigned long long nb = gridDim.x;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double a[R], t[R];
    uint32_t anc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        a[r] = (i0 + r < n) ? mom_weight(lw[i0 + r], m) : 0.;
        anc[r] = (i0 + r < n) ? (uint32_t)(i0 + r) : 0u;
        t[r] = a[r];
    }
    mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), 0, s_a);
    __syncthreads();
    if (threadIdx.x == 0) out[(unsigned long long)T * DP * nb + blockIdx.x] = mom_block_combine<mom_add>(0, s_a);
    int tt = T, pb = 0;
    for (int e = n_events - 1; e >= 0; --e) {
        const void* buf = ev[e].buf;
        if (ev[e].kind == 1) {
            const uint32_t* parents = static_cast<const uint32_t*>(buf);
#pragma unroll
            for (int r = 0; r < R; ++r) anc[r] = parents[anc[r]];
            continue;
        }
        --tt;
        const double* x = static_cast<const double*>(buf);
        double v[R][DP];
#pragma unroll
        for (int r = 0; r < R; ++r) mom_load_row<DP>(x + (unsigned long long)anc[r] * DP, v[r]);
        if (bitmap) {
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (i0 + r < n) atomicOr(&bitmap[(unsigned long long)tt * words + (anc[r] >> 5)], 1u << (anc[r] & 31u));
        }
        double* sp = s_part[pb];
#pragma unroll
        for (int j = 0; j < DP; ++j) {
#pragma unroll
            for (int r = 0; r < R; ++r) t[r] = (i0 + r < n) ? a[r] * v[r][j] : 0.;
            mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), j, sp);
        }
        __syncthreads();
        if ((int)threadIdx.x < DP) out[((unsigned long long)tt * DP + threadIdx.x) * nb + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, sp);
        pb ^= 1;
    }
}

// pass 2: out[(t d + j) nb + b] = subtree of a_i (v_ij(t) - mean_tj)^2.  sums = the closed trees of pass 1 ({S[T][d], A}); every lane
// forms mean_tj = S_tj / A itself (same bits), workgroup 0 stores it.  One component at a time: the gathered rows stay live (R DP
// doubles), the centred values never do.
template <int DP>
__global__ __launch_bounds__(MOM_THREADS) void k_path_mom2(unsigned long long n, int n_events, int T, const mp_hist_event* __restrict__ ev,
                                                           const double* __restrict__ lw, const double* __restrict__ m_ptr, const double* __restrict__ sums,
                                                           double* __restrict__ mean_out, double* __restrict__ out) {
    constexpr int R = mom_run<DP>::R;
    __shared__ double s_part[2][DP * MOM_WAVES];
    const double m = *m_ptr;
    const double A = sums[(unsigned long long)T * DP];
    const unsigned long long nb = gridDim.x;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double a[R], t[R];
    uint32_t anc[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        a[r] = (i0 + r < n) ? mom_weight(lw[i0 + r], m) : 0.;
        anc[r] = (i0 + r < n) ? (uint32_t)(i0 + r) : 0u;
    }
    int tt = T, pb = 0;
    for (int e = n_events - 1; e >= 0; --e) {
        const void* buf = ev[e].buf;
        if (ev[e].kind == 1) {
            const uint32_t* parents = static_cast<const uint32_t*>(buf);
#pragma unroll
            for (int r = 0; r < R; ++r) anc[r] = parents[anc[r]];
            continue;
        }
        --tt;
        const double* x = static_cast<const double*>(buf);
        double v[R][DP];
#pragma unroll
        for (int r = 0; r < R; ++r) mom_load_row<DP>(x + (unsigned long long)anc[r] * DP, v[r]);
        double* sp = s_part[pb];
#pragma unroll
        for (int j = 0; j < DP; ++j) {
            const double mean = sums[(unsigned long long)tt * DP + j] / A;
            if (blockIdx.x == 0 && threadIdx.x == 0) mean_out[(unsigned long long)tt * DP + j] = mean;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double c = (i0 + r < n) ? v[r][j] - mean : 0.;
                t[r] = (i0 + r < n) ? a[r] * (c * c) : 0.;
            }
            mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), j, sp);
        }
        __syncthreads();
        if ((int)threadIdx.x < DP) out[((unsigned long long)tt * DP + threadIdx.x) * nb + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, sp);
        pb ^= 1;
    }
}

// distinct[t] = the set bits of row t of the bitmap: one workgroup per t, integer adds (exact in any order)
__global__ __launch_bounds__(MOM_THREADS) void k_path_distinct(const uint32_t* __restrict__ bitmap, unsigned long long words, unsigned long long* __restrict__ out) {
    __shared__ unsigned long long s_cnt[MOM_WAVES];
    const uint32_t* row = bitmap + (unsigned long long)blockIdx.x * words;
    unsigned long long cnt = 0;
    for (unsigned long long w = threadIdx.x; w < words; w += MOM_THREADS) cnt += (unsigned long long)__popc(row[w]);
#pragma unroll
    for (int s = 1; s < 64; s <<= 1) cnt += __shfl_xor(cnt, s, 64);
    if ((threadIdx.x & 63) == 0) s_cnt[threadIdx.x >> 6] = cnt;
    __syncthreads();
    if (threadIdx.x == 0) out[blockIdx.x] = (s_cnt[0] + s_cnt[1]) + (s_cnt[2] + s_cnt[3]);
}

#endif   // MP_MOMENTS_PF

#ifdef MP_MOMENTS_MH   // (mp_mh.hip)
// ---- MH chains of a registered function: vals[site][chain], present[word][chain]; one grid row per site ------------------------------------
// pass 1: out[2 s][b] = subtree of (p_i ? v_i : +0.0), out[2 s + 1][b] = subtree of p_i
__global__ __launch_bounds__(MOM_THREADS) void k_mom_site1(unsigned long long n, const double* __restrict__ vals, const uint32_t* __restrict__ present,
                                                           double* __restrict__ out) {
    constexpr int R = 8;
    __shared__ double s_part[2 * MOM_WAVES];
    const unsigned int s = blockIdx.y;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double tv[R], tp[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool p = (i0 + r < n) && ((present[(unsigned long long)(s >> 5) * n + i0 + r] >> (s & 31u)) & 1u);
        tv[r] = p ? vals[(unsigned long long)s * n + i0 + r] : 0.;
        tp[r] = p ? 1. : 0.;
    }
    mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(tv), 0, s_part);
    mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(tp), 1, s_part);
    __syncthreads();
    if (threadIdx.x < 2) out[(unsigned long long)(2 * s + threadIdx.x) * gridDim.x + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, s_part);
}
// pass 2: out[s][b] = subtree of (p_i ? (v_i - mean_s)^2 : +0.0), mean_s = sums[2 s] / sums[2 s + 1] (0 / 0 = NaN for a site nobody has: no term is selected)
__global__ __launch_bounds__(MOM_THREADS) void k_mom_site2(unsigned long long n, const double* __restrict__ vals, const uint32_t* __restrict__ present,
                                                           const double* __restrict__ sums, double* __restrict__ mean_out, double* __restrict__ out) {
    constexpr int R = 8;
    __shared__ double s_part[MOM_WAVES];
    const unsigned int s = blockIdx.y;
    const double mean = sums[2 * s] / sums[2 * s + 1];
    if (blockIdx.x == 0 && threadIdx.x == 0) mean_out[s] = mean;
    const unsigned long long i0 = ((unsigned long long)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    double t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const bool p = (i0 + r < n) && ((present[(unsigned long long)(s >> 5) * n + i0 + r] >> (s & 31u)) & 1u);
        const double c = p ? vals[(unsigned long long)s * n + i0 + r] - mean : 0.;
        t[r] = p ? c * c : 0.;
    }
    mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), 0, s_part);
    __syncthreads();
    if (threadIdx.x == 0) out[(unsigned long long)s * gridDim.x + blockIdx.x] = mom_block_combine<mom_add>(0, s_part);
}

#endif   // MP_MOMENTS_MH

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static inline bool mom_width_ok(int d) { return d == 1 || d == 2 || d == 4 || d == MOM_MAX_DIM; }   // the compiled models' widths
// f(std::integral_constant<int, D>) for D = d: the one place that turns a run-time width into a kernel's template argument
template <class F>
static inline void mom_for_width(int d, F&& f) {
    switch (d) {
    case 1: f(std::integral_constant<int, 1>{}); break;
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    default: f(std::integral_constant<int, MOM_MAX_DIM>{}); break;
    }
}

// The grids of a reduction over n slots of width d: nb workgroups for the level-0 passes (R = mom_run<D>::R slots per lane, the kernels'
// own constant), nb_max <= nb for the max pass, nn partials per column after the first k_mom_tree level.
// k_mom_max0's slots per lane.  A known leftover: the kernel's own `constexpr int R = 8` is a literal in device text, which stays as it
// is, so this copy is tied to it by this comment only (unlike the moment passes' R, which comes from mom_run<D>::R below).
constexpr int MOM_MAX0_R = 8;
static inline unsigned long long mom_blocks(unsigned long long n, int R) {
    return (n + (unsigned long long)MOM_THREADS * R - 1) / ((unsigned long long)MOM_THREADS * R);
}
struct mom_grids { unsigned long long nb, nb_max, nn; };
static inline mom_grids mom_plan(unsigned long long n, int d) {
    mom_grids g{};
    mom_for_width(d, [&](auto D) {
        constexpr int R = mom_run<decltype(D)::value>::R;
        static_assert(R <= MOM_MAX0_R, "the max pass must not need more partials than a moment pass: one scratch holds both");
        g.nb = mom_blocks(n, R);
    });
    g.nb_max = mom_blocks(n, MOM_MAX0_R);
    g.nn = (g.nb + MOM_TREE_RUN - 1) / MOM_TREE_RUN;
    return g;
}

// The scratch of a reduction: partials of one pass ([columns][workgroups], two levels), the closed trees on the device and where they
// land on the host.  Grow-only; a capacity is zeroed before its block is replaced, so a failed allocation leaves a holder that
// allocates again next time.
struct mom_scratch {
    mp_dev<double> buf[2];
    mp_dev<double> res;
    mp_pinned<double> host;
    size_t cap[3] = {0, 0, 0};   // doubles in buf[0], in buf[1], and in res and host each
    bool holds(size_t cols, const mom_grids& g, size_t n_res) const { return cols * g.nb <= cap[0] && cols * g.nn <= cap[1] && n_res <= cap[2]; }
    // room for `cols` columns of g.nb partials each (the max pass's g.nb_max <= g.nb fit too) and for n_res results
    hipError_t reserve(size_t cols, const mom_grids& g, size_t n_res) {
        const size_t want[3] = {cols * (size_t)g.nb, cols * (size_t)g.nn, n_res};
        for (int k = 0; k < 3; ++k) {
            if (want[k] <= cap[k]) continue;
            cap[k] = 0;
            hipError_t e = k < 2 ? mp_hipMalloc(buf[k], want[k]) : mp_hipMalloc(res, want[k]);
            if (e == hipSuccess && k == 2) e = mp_hipHostMalloc(host, want[k]);
            if (e != hipSuccess) return e;
            cap[k] = want[k];
        }
        return hipSuccess;
    }
};

// Close the trees of `cols` columns of `nb` partials each ([cols][nb] in buf[0]) into dst[cols].  buf[0] holds cols * nb doubles, buf[1]
// cols * ceil(nb / 1024).  At least one launch: a single partial goes through the tree as v + 0.  A grid has at most 65535 rows, so
// the columns go in slices of that many, each closing inside its own part of the two buffers.
template <class Op>
static inline void mom_close(hipStream_t stream, double* const buf[2], unsigned long long nb, unsigned long long cols, double* dst) {
    const unsigned long long nn = (nb + MOM_TREE_RUN - 1) / MOM_TREE_RUN;
    for (unsigned long long c0 = 0; c0 < cols; c0 += 65535) {
        double* const part[2] = {buf[0] + c0 * nb, buf[1] + c0 * nn};
        const unsigned rows = (unsigned)std::min<unsigned long long>(65535, cols - c0);
        int cur = 0;
        for (unsigned long long in = nb, out = nn;; in = out, out = (out + MOM_TREE_RUN - 1) / MOM_TREE_RUN, cur ^= 1) {
            hipLaunchKernelGGL(k_mom_tree<Op>, dim3((unsigned)out, rows), dim3(MOM_THREADS), 0, stream, (const double*)part[cur], in, out == 1 ? dst + c0 : part[cur ^ 1], out);
            if (out == 1) break;
        }
    }
}
