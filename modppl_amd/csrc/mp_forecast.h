// mp_forecast.h — the filter's forecast on the device: predictive paths and their weighted moments (gfx950, wave64; included by
// mp_pf.hip after mp_moments.h).
//
// DynUnfold::update with ArgDiff::Extend and empty constraints for the new steps (modppl/src/modeling/dynunfold.rs:66-100) runs the
// kernel from each trace's last state; sample_at's unconstrained arm draws every site and the weight is 0.  Here (DESIGN.md §4,
// "Forecast"), with T = mp_pf_time and H the horizon: for k = 0 .. H-1 slot i runs the model kernel in Simulate mode
// (mp_simulate_handler: every site drawn, the observed ones too) at time T + k from its own current state (k = 0) or its previous
// forecast state:  v_i(k) [dim_state], y_i(k) [dim_obs].
//
// THE COUNTER RULE: Philox slot = the GLOBAL slot slot_offset + i, Philox step = T + k, kernel time argument = T + k — what
// mp_pf_step uses for its proposal at that time (k_propagate, k_propagate_mt) and what k_simulate uses at that t.  So
//   * the forecast states are the states the next H unresampled steps would propose, bit for bit, whatever they are given to observe;
//   * after init_step, slot i's forecast is trace i of mp_unfold_simulate(model, args0, 1 + H, n, seed) at steps 1 .. H, bit for bit.
// The forecast is a pure function of (seed, slot, step, state): nothing is stored on the handle and nothing of size n H anywhere —
// the variance pass SIMULATES AGAIN from the same counters instead of reading a scratch buffer.
//
// Moments: the weights and trees of mp_pf_moments (mp_moments.h), cut where k_mom_pf1 cuts them (mom_run<D>::R consecutive slots per
// lane), over the dim_state + dim_obs columns of every k:
//   mean[k][c] = TREE(a_i v_ic(k)) / A;   var[k][c] = TREE(a_i (v_ic(k) - mean[k][c])^2) / A      (population form, marginal only)
// A lane keeps its R weights and R current forecast states (registers up to d = 4; private memory at d = 16, see k_forecast_mom) and
// advances its slots ONE AFTER THE OTHER through the model body (one slot's temporaries live at a time); slots past n run no model code
// and are selected to +0.0, never multiplied.  One partial
// per (k, column, workgroup): out[(k C + c) nb + b], C = dim_state + dim_obs; LDS partials alternate between two buffers as in
// k_path_mom1, so a forecast step costs one __syncthreads.
#pragma once
#include "mp_moments.h"

struct mp_forecast_args {
    u64 n, slot_offset;
    uint32_t k0, k1;
    long long t;        // mp_pf_time: the time argument and Philox step of forecast step 0
    int horizon;
    const double* x;    // [n][dim_state] current states, slot order
};

// ---- paths: one lane per slot of the window [first, first + count), as in k_simulate ------------------------------------------------
// states [count][H][D] and obs [count][H][DO] (either may be null)
template <class Model>
__global__ __launch_bounds__(256) void k_forecast_paths(Model model, mp_forecast_args f, u64 first, u64 count, double* __restrict__ states,
                                                        double* __restrict__ obs) {
    constexpr int D = Model::DIM_STATE, DO = Model::DIM_OBS;
    const u64 i = (u64)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const u64 slot = first + i;   // (< n: the host checks first + count <= n)
    double prev[D];
    for (int d = 0; d < D; ++d) prev[d] = f.x[slot * D + d];
    mp_stream rng;
    rng.k0 = f.k0; rng.k1 = f.k1; rng.slot = (uint32_t)(f.slot_offset + slot);
    const u64 H = (u64)f.horizon;
    mp_simulate_trace(model, rng, f.t, f.horizon, prev, states ? states + i * H * D : nullptr, obs ? obs + i * H * DO : nullptr);
}

// ---- moments: pass 1 (PASS2 = false) out[(k C + c) nb + b] = subtree of a_i v_ic(k), out[H C nb + b] = subtree of a_i;
//               pass 2 (PASS2 = true)  out[(k C + c) nb + b] = subtree of a_i (v_ic(k) - mean_kc)^2, the same simulation run again.
// sums = the closed trees of pass 1 ({S[H][C], A}); every lane forms mean_kc = S_kc / A itself (same bits), workgroup 0 stores it.
template <class Model, bool PASS2>
__global__ __launch_bounds__(MOM_THREADS) void k_forecast_mom(Model model, mp_forecast_args f, const double* __restrict__ lw,
                                                              const double* __restrict__ m_ptr, const double* __restrict__ sums,
                                                              double* __restrict__ mean_out, double* __restrict__ out) {
    constexpr int D = Model::DIM_STATE, DO = Model::DIM_OBS, C = D + DO;
    constexpr int R = mom_run<D>::R;
    // wide models (d = 16: lane-serial 16 x 16 bodies, 140+ VGPRs on their own) keep ONE copy of the model body and walk their R slots
    // in a loop, the states and observations in private memory (1 KB per lane); unrolled R times the dense body took all 512 registers
    // and spilled 1000 dwords more
    constexpr int UNROLL_SLOTS = D > 4 ? 1 : R;
    static_assert(DO >= 1 && C <= MOM_THREADS, "one thread per column closes the workgroup's trees");
    __shared__ double s_part[2][C * MOM_WAVES];
    __shared__ double s_a[MOM_WAVES];
    const double m = *m_ptr;
    const u64 n = f.n;
    const unsigned long long nb = gridDim.x;
    const u64 i0 = ((u64)blockIdx.x * MOM_THREADS + threadIdx.x) * R;
    const int H = f.horizon;
    double a[R], v[R][D], y[R][DO], t[R];
#pragma unroll
    for (int r = 0; r < R; ++r) {
        a[r] = (i0 + r < n) ? mom_weight(lw[i0 + r], m) : 0.;
#pragma unroll
        for (int j = 0; j < D; ++j) v[r][j] = (i0 + r < n) ? f.x[(i0 + r) * D + j] : 0.;
    }
    double A = 0.;
    if constexpr (PASS2) {
        A = sums[(unsigned long long)H * C];
    } else {
#pragma unroll
        for (int r = 0; r < R; ++r) t[r] = a[r];
        mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), 0, s_a);
        __syncthreads();
        if (threadIdx.x == 0) out[(unsigned long long)H * C * nb + blockIdx.x] = mom_block_combine<mom_add>(0, s_a);
    }
    mp_stream rng;
    rng.k0 = f.k0; rng.k1 = f.k1;
    int pb = 0;
    for (int k = 0; k < H; ++k) {
#pragma unroll(UNROLL_SLOTS)
        for (int r = 0; r < R; ++r) {
            if (i0 + r < n) {
                double next[D];
                rng.slot = (uint32_t)(f.slot_offset + i0 + r);
                mp_simulate_step(model, rng, f.t + k, v[r], next, y[r]);
#pragma unroll
                for (int j = 0; j < D; ++j) v[r][j] = next[j];
            } else {
#pragma unroll
                for (int j = 0; j < DO; ++j) y[r][j] = 0.;
            }
        }
        double* sp = s_part[pb];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            double mean = 0.;
            if constexpr (PASS2) {
                mean = sums[(unsigned long long)k * C + c] / A;
                if (blockIdx.x == 0 && threadIdx.x == 0) mean_out[(unsigned long long)k * C + c] = mean;
            }
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const double val = c < D ? v[r][c < D ? c : 0] : y[r][c < D ? 0 : c - D];   // (c is a compile-time index)
                if constexpr (PASS2) {
                    const double ctr = (i0 + r < n) ? val - mean : 0.;
                    t[r] = (i0 + r < n) ? a[r] * (ctr * ctr) : 0.;
                } else {
                    t[r] = (i0 + r < n) ? a[r] * val : 0.;
                }
            }
            mom_block_put<mom_add>(mom_lane_tree<mom_add, R>(t), c, sp);
        }
        __syncthreads();
        if ((int)threadIdx.x < C) out[((unsigned long long)k * C + threadIdx.x) * nb + blockIdx.x] = mom_block_combine<mom_add>((int)threadIdx.x, sp);
        pb ^= 1;
    }
}
