// mp_pf_readouts.h — the filter's readouts beyond a plain copy: reduce or gather on the device, read back a handful of doubles.  Cloud
// moments, path moments, forecast paths and moments, cloud and path quantiles, trajectories.  Part of mp_pf.hip's translation unit
// (struct mp_pf is private to it), included after the handle and its helpers; host code only, the kernels are in mp_moments.h,
// mp_forecast.h, mp_quantiles.h and mp_pf_kernels.h.
//
// Every summary call has ONE shape, written down once each:
//   readout_begin    the handle's checks in a fixed order, then the handle brought to a readable state
//   mom_plan         the grids (mp_moments.h);  mp_pf::scratch, the one mom_scratch of the handle
//   max_pass         m = max log-weight, the first launches of every call
//   mom_for_width    the kernel for this dim_state;  mom_close, the trees of any number of columns
//   readout_finish   launch status, results to the host, the ONE wait (on the failure path too), the all -inf test
//   readout_mean     the mean of a call that ran no second pass
// All launches are enqueued before that one wait, so a cloud whose log-weights are all -inf still pays for every pass (its weights are
// selected to 0 and nothing is returned but the status): looking at m after the max pass would cost every healthy call a second wait.
// None of these calls changes anything the filter computes afterwards: no state, weight, parent, counter, time or history event.
#pragma once

// What a readout needs of the handle, checked in this order whichever are asked for (the order every call had on its own): not a
// shard of a larger world (MP_ERR_UNSUPPORTED), recorded history (MP_ERR_STATE), init_step done (MP_ERR_STATE; always), a reduction
// kernel for this dim_state (MP_ERR_UNSUPPORTED).  Then the device, materialize, ensure_x, ensure_lazy — every readout reads the
// states and the log-weights — and, with history, that the log holds one state per step.  Checks of a call's own arguments stay in the call.
enum : unsigned { RD_NO_SHARD = 1, RD_HISTORY = 2, RD_KERNEL = 4 };
static int32_t readout_begin(mp_pf* h, const char* who, unsigned needs) {
    const auto fail = [who](int32_t code, const char* what) { return mp_fail(code, std::string(who) + what); };
    if ((needs & RD_NO_SHARD) && h->sharded) return fail(MP_ERR_UNSUPPORTED, ": one shard of a larger world (n_global != n_particles); the summary of a sharded job needs an all-reduce of the max and of the partials, and its ancestors live on other ranks");
    if ((needs & RD_HISTORY) && !(h->flags & MP_PF_RECORD_HISTORY)) return fail(MP_ERR_STATE, " needs a filter created with MP_PF_RECORD_HISTORY");
    if (!h->initialised) return fail(MP_ERR_STATE, " before init_step");
    if ((needs & RD_KERNEL) && !mom_width_ok(h->ops->dim_state)) return fail(MP_ERR_UNSUPPORTED, ": no kernel for this dim_state (the compiled models have 1, 2, 4 or 16)");
    HIPCK(hipSetDevice(h->device));
    MPCK(materialize(h));
    MPCK(ensure_x(h));
    MPCK(ensure_lazy(h));
    if (needs & RD_HISTORY) {
        size_t n_step_events = 0;
        for (const auto& e : h->hist) n_step_events += e.kind == 0;
        if (n_step_events != (size_t)h->t) return fail(MP_ERR_STATE, ": the recorded history does not hold one state per step");
    }
    return MP_OK;
}

// scratch for `steps` time (or horizon) steps of `c` columns each, + A, and 2 + steps * res_per_step results: when short it grows to
// max(16, 2 steps) steps, so a filter that asks after every step reallocates a logarithmic number of times
static int32_t reserve_steps(mp_pf* h, size_t steps, size_t c, const mom_grids& g, size_t res_per_step) {
    if (h->scratch.holds(steps * c + 1, g, 2 + steps * res_per_step)) return MP_OK;
    const size_t cap = std::max<size_t>(16, 2 * steps);
    HIPCK(h->scratch.reserve(cap * c + 1, g, 2 + cap * res_per_step));
    return MP_OK;
}

// m = max log-weight -> dst[0], enqueued on the handle's stream (the scratch holds at least one column: every caller has reserved)
static void max_pass(mp_pf* h, const mom_grids& g, double* dst) {
    double* const buf[2] = {h->scratch.buf[0].get(), h->scratch.buf[1].get()};
    hipLaunchKernelGGL(k_mom_max0, dim3((unsigned)g.nb_max), dim3(MOM_THREADS), 0, h->stream, h->n, (const double*)h->logw, buf[0]);
    mom_close<mom_max>(h->stream, buf, g.nb_max, 1, dst);
}

// The end of a summary call: `e` is the status of its launches and copies so far; n_res doubles of scratch.res go to scratch.host.  The
// stream is idle when this returns, on every path: nothing the caller owns (a host vector of events) is read after it, and a failed
// call leaves no work behind.  r[0] is m: all log-weights -inf is MP_ERR_DEGENERATE.  (A NaN m: every weight is NaN or was clamped,
// and the results hold NaN already.)
static int32_t readout_finish(mp_pf* h, const char* who, hipError_t e, size_t n_res) {
    if (e == hipSuccess) e = hipMemcpyAsync(h->scratch.host, h->scratch.res, sizeof(double) * n_res, hipMemcpyDeviceToHost, h->stream);
    const hipError_t e2 = stream_wait(h->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return mp_fail(MP_ERR_HIP, std::string(who) + ": " + hipGetErrorString(e));
    if (h->scratch.host[0] == -MP_INF) return mp_fail_degenerate();
    return MP_OK;
}
// column c's mean: the second pass formed it on the device; without one nobody has, and the same IEEE division happens here
static inline double readout_mean(bool second_pass, const double* S, const double* mean, double A, size_t c) {
    return second_pass ? mean[c] : S[c] / A;
}

// the event log as the history kernels read it (k_trajectories, k_path_mom1/2, k_q_hist_path), enqueued on the handle's stream; `ev` is
// the caller's and stays alive until it has waited for the stream
static int32_t upload_hist_events(mp_pf* h, std::vector<mp_hist_event>& ev) {
    ev.resize(h->hist.size());
    for (size_t e = 0; e < h->hist.size(); ++e) { ev[e].buf = h->hist[e].buf; ev[e].kind = h->hist[e].kind; ev[e].pad = 0; }
    if (h->d_hist_events_cap < ev.size()) {
        h->d_hist_events_cap = 0;
        const size_t cap = std::max<size_t>(64, 2 * ev.size());
        HIPCK(mp_hipMalloc(h->d_hist_events, cap));
        h->d_hist_events_cap = cap;
    }
    HIPCK(hipMemcpyAsync(h->d_hist_events, ev.data(), sizeof(mp_hist_event) * ev.size(), hipMemcpyHostToDevice, h->stream));
    return MP_OK;
}

// mp_pf_moments: one level-0 launch of pass 1 (first moments) or 2 (centred second moments) for a state width D
template <int D>
static void launch_moments_pass(mp_pf* h, int pass, unsigned nb, const double* x, double* res) {
    if (pass == 1)
        hipLaunchKernelGGL((k_mom_pf1<D>), dim3(nb), dim3(MOM_THREADS), 0, h->stream, h->n, x, (const double*)h->logw, (const double*)res,
                           h->scratch.buf[0].get());
    else
        hipLaunchKernelGGL((k_mom_pf2<D>), dim3(nb), dim3(MOM_THREADS), 0, h->stream, h->n, x, (const double*)h->logw, (const double*)res,
                           (const double*)(res + 1), res + 2 + D, h->scratch.buf[0].get());
}
// mp_pf_path_moments: the level-0 walk of pass 1 or 2 for a state width D; res = {m, S[T][D], A, mean[T][D], ...}
template <int D>
static void launch_path_pass(mp_pf* h, int pass, unsigned nb, int T, double* res, uint32_t* bitmap, u64 words) {
    const mp_hist_event* ev = h->d_hist_events;
    if (pass == 1)
        hipLaunchKernelGGL((k_path_mom1<D>), dim3(nb), dim3(MOM_THREADS), 0, h->stream, h->n, (int)h->hist.size(), T, ev, (const double*)h->logw,
                           (const double*)res, h->scratch.buf[0].get(), bitmap, words);
    else
        hipLaunchKernelGGL((k_path_mom2<D>), dim3(nb), dim3(MOM_THREADS), 0, h->stream, h->n, (int)h->hist.size(), T, ev, (const double*)h->logw,
                           (const double*)res, (const double*)(res + 1), res + 2 + (size_t)T * D, h->scratch.buf[0].get());
}
template <int D>
static void launch_quantiles_hist(mp_pf* h, int pass, int nq, const q_bufs& b) {
    const unsigned nb = (unsigned)((h->n + (u64)Q_THREADS * Q_ROWS - 1) / ((u64)Q_THREADS * Q_ROWS));
    constexpr int QC = Q_SEL_CHUNK / D;
    hipLaunchKernelGGL((k_q_hist_pf<D>), dim3(nb, (unsigned)((nq + QC - 1) / QC)), dim3(Q_THREADS), 0, h->stream, h->n, (const double*)h->x[h->cur],
                       (const u64*)h->q_W.get(), pass, nq, b);
}
template <int D>
static void launch_path_quantiles_hist(mp_pf* h, int pass, int nq, int Q, const q_bufs& b) {
    constexpr int R = mom_run<D>::R, QC = Q_SEL_CHUNK / D;
    const unsigned nb = (unsigned)((h->n + (u64)Q_THREADS * R - 1) / ((u64)Q_THREADS * R));
    hipLaunchKernelGGL((k_q_hist_path<D>), dim3(nb, (unsigned)((nq + QC - 1) / QC)), dim3(Q_THREADS), 0, h->stream, h->n, (int)h->hist.size(), (int)h->t,
                       (const mp_hist_event*)h->d_hist_events, (const u64*)h->q_W.get(), pass, nq, Q, b);
}

// mp_pf_quantiles / mp_pf_path_quantiles: the checks both share, room for nsel_per_t * max(T, 1) selectors, then m = max lw ->
// scratch.res[0] and the integer weights -> q_W, enqueued on the handle's stream.  The selected values follow m: scratch.res[1 + selector].
static int32_t quantiles_begin(mp_pf* h, const char* who, const double* qs, int32_t n_q, bool path, q_spec& spec, q_bufs& b, size_t& nsel) {
    if (!q_make_spec(qs, n_q, spec)) return mp_fail(MP_ERR_INVALID_ARG, std::string(who) + ": n_q outside [1, 16], or a level that is NaN or outside [0, 1]");
    MPCK(readout_begin(h, who, RD_NO_SHARD | RD_KERNEL | (path ? RD_HISTORY : 0u)));
    nsel = (size_t)n_q * h->ops->dim_state * (path ? (size_t)h->t : 1);
    // every selector owns 2 KiB of bins, refilled on each pass: a call is held to Q_MAX_SEL of them (0.5 GiB) rather than left to hipMalloc
    if (nsel > (size_t)Q_MAX_SEL) return mp_fail(MP_ERR_UNSUPPORTED, std::string(who) + ": time steps * n_q * dim_state exceeds " + std::to_string(Q_MAX_SEL) + " selectors; ask for fewer levels per call");
    if (!h->q_W) HIPCK(mp_hipMalloc(h->q_W, h->n));
    if (h->q_cap < nsel) {
        const size_t cap = std::min<size_t>((size_t)Q_MAX_SEL, std::max<size_t>((size_t)Q_MAX_Q * MOM_MAX_DIM, 2 * nsel));
        h->q_cap = 0;
        HIPCK(mp_hipMalloc(h->q_bins, cap * Q_BINS));
        HIPCK(mp_hipMalloc(h->q_st, 3 * cap));
        h->q_cap = cap;
    }
    const mom_grids g = mom_plan(h->n, h->ops->dim_state);
    HIPCK(h->scratch.reserve(1, g, 1 + h->q_cap));
    double* res = h->scratch.res;
    b = q_bufs{h->q_bins.get(), h->q_st.get(), h->q_st.get() + h->q_cap, h->q_st.get() + 2 * h->q_cap, res + 1};
    if (nsel == 0) return MP_OK;   // (a history filter at time 0)
    max_pass(h, g, res);
    hipLaunchKernelGGL(k_q_weights, dim3((unsigned)((h->n + Q_THREADS - 1) / Q_THREADS)), dim3(Q_THREADS), 0, h->stream, h->n, (const double*)h->logw,
                       (const double*)res, q_scale(h->n), h->q_W.get());
    return check_launch("mp_pf quantile weights");
}

// The forecast (mp_forecast.h; DESIGN.md section 4, "Forecast"): DynUnfold::update with ArgDiff::Extend and EMPTY constraints for the new
// steps (modppl/src/modeling/dynunfold.rs:66-100) — every site of the next `horizon` kernel calls drawn, from each slot's own state,
// with the Philox counters the next steps would use.
static int32_t forecast_begin(mp_pf* h, const char* who, int32_t horizon, mp_forecast_args& f) {
    if (!h) return mp_fail(MP_ERR_INVALID_ARG, "null handle");
    if (h->model_kind == MP_MODEL_HMM) return mp_fail(MP_ERR_UNSUPPORTED, "the reference's HMM has no simulate (tests/hmm/model.rs: unimplemented)");
    if (!h->initialised) return mp_fail(MP_ERR_STATE, std::string(who) + " before init_step");
    if (horizon < 1) return mp_fail(MP_ERR_INVALID_ARG, std::string(who) + ": horizon must be at least 1");
    f.n = h->n; f.slot_offset = h->slot_offset;
    f.k0 = (uint32_t)h->seed; f.k1 = (uint32_t)(h->seed >> 32);
    f.t = h->t;
    f.horizon = horizon;
    return MP_OK;
}
// a grow-only device buffer of at least `want` doubles
static int32_t fc_grow(mp_dev<double>& buf, size_t& cap, size_t want) {
    if (cap >= want) return MP_OK;
    cap = 0;
    HIPCK(mp_hipMalloc(buf, want));
    cap = want;
    return MP_OK;
}

extern "C" {

// Weighted mean and covariance of the particle cloud, reduced on the device: replaces the host-side reduction a caller of the reference
// writes over its public `traces` / `log_weights` fields (particle_filter.rs:13-20) — here mp_pf_read_state + mp_pf_read_log_weights
// and a loop.  Definition (the tree sum, relative to the global max log-weight): mp_moments.h, DESIGN.md section 4.
int32_t mp_pf_moments(mp_pf* h, double* mean_out, double* cov_out) {
    if (!h || !mean_out) return mp_fail(MP_ERR_INVALID_ARG, "null argument");
    MPCK(readout_begin(h, "mp_pf_moments", RD_NO_SHARD | RD_KERNEL));
    const int d = h->ops->dim_state, npairs = d * (d + 1) / 2;
    const mom_grids g = mom_plan(h->n, d);
    const size_t n_res = 2 + 2 * (size_t)d + npairs;
    HIPCK(h->scratch.reserve((size_t)std::max(d + 1, npairs), g, n_res));
    double* const buf[2] = {h->scratch.buf[0].get(), h->scratch.buf[1].get()};
    double* res = h->scratch.res;   // {m, A, S[d], mean[d], C[d (d + 1) / 2]}
    const double* x = h->x[h->cur];
    max_pass(h, g, res);
    for (int pass = 1; pass <= (cov_out ? 2 : 1); ++pass) {
        mom_for_width(d, [&](auto D) { launch_moments_pass<decltype(D)::value>(h, pass, (unsigned)g.nb, x, res); });
        mom_close<mom_add>(h->stream, buf, g.nb, pass == 1 ? d + 1 : npairs, pass == 1 ? res + 1 : res + 2 + 2 * d);
    }
    MPCK(readout_finish(h, "mp_pf_moments", hipGetLastError(), n_res));
    const double* r = h->scratch.host;
    const double A = r[1];
    for (int j = 0; j < d; ++j) mean_out[j] = readout_mean(cov_out != nullptr, r + 2, r + 2 + d, A, j);
    if (cov_out) {
        const double* C = r + 2 + 2 * d;
        for (int j = 0; j < d; ++j)
            for (int k = 0; k <= j; ++k) cov_out[j * d + k] = cov_out[k * d + j] = C[j * (j + 1) / 2 + k] / A;
    }
    return MP_OK;
}

int32_t mp_pf_read_trajectories(mp_pf* h, uint64_t first, uint64_t count, double* out, int32_t* t_steps) {
    if (!h || !out || !t_steps) return mp_fail(MP_ERR_INVALID_ARG, "null argument");
    if (!(h->flags & MP_PF_RECORD_HISTORY)) return mp_fail(MP_ERR_STATE, "read_trajectory needs a filter created with MP_PF_RECORD_HISTORY");
    if (h->sharded) return mp_fail(MP_ERR_UNSUPPORTED, "read_trajectory: ancestors of a sharded filter live on other ranks");
    if (count == 0 || first >= h->n || count > h->n - first) return mp_fail(MP_ERR_INVALID_ARG, "particle range out of bounds");
    HIPCK(hipSetDevice(h->device));
    const int d = h->ops->dim_state;
    const int T = (int)h->t;
    *t_steps = (int32_t)h->t;
    if (T == 0) return MP_OK;
    std::vector<mp_hist_event> ev;
    MPCK(upload_hist_events(h, ev));
    mp_dev<double> d_out;
    const size_t bytes = sizeof(double) * (size_t)count * (size_t)T * (size_t)d;
    HIPCK(mp_hipMalloc(d_out, (size_t)count * (size_t)T * (size_t)d));
    hipLaunchKernelGGL(k_trajectories, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, h->stream, (u64)first, (u64)count, d, T, (int)ev.size(),
                       (const mp_hist_event*)h->d_hist_events, d_out.get());
    hipError_t e1 = hipGetLastError();
    if (e1 == hipSuccess) e1 = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, h->stream);
    if (e1 == hipSuccess) e1 = hipStreamSynchronize(h->stream);   // (ev / d_out stay alive until here)
    if (e1 != hipSuccess) return mp_fail(MP_ERR_HIP, std::string("mp_pf_read_trajectories: ") + hipGetErrorString(e1));
    return MP_OK;
}

int32_t mp_pf_read_trajectory(mp_pf* h, uint64_t i, double* out, int32_t* t_steps) {
    return mp_pf_read_trajectories(h, i, 1, out, t_steps);
}

// Smoothed mean and variance per time step over the recorded ancestry, and the number of distinct ancestors per step, reduced on the
// device: replaces walking `traces[i].retv` of every particle (particle_filter.rs:13; tests/smc.rs:67) — here mp_pf_read_trajectories,
// n * T * d doubles over the link — and a host loop.  Definition: mp_moments.h, DESIGN.md section 4, "Path moments".
int32_t mp_pf_path_moments(mp_pf* h, double* mean_out, double* var_out, uint64_t* distinct_out, int32_t* t_steps) {
    if (!h || !mean_out || !t_steps) return mp_fail(MP_ERR_INVALID_ARG, "null argument");
    MPCK(readout_begin(h, "mp_pf_path_moments", RD_NO_SHARD | RD_HISTORY | RD_KERNEL));
    const int d = h->ops->dim_state, T = (int)h->t;
    *t_steps = (int32_t)h->t;
    if (T == 0) return MP_OK;
    const mom_grids g = mom_plan(h->n, d);
    const size_t TD = (size_t)T * d;
    const size_t n_res = 2 + 3 * TD + (size_t)T;
    MPCK(reserve_steps(h, (size_t)T, (size_t)d, g, 3 * (size_t)d + 1));
    const u64 words = (h->n + 31) / 32;
    if (distinct_out && h->path_bits_cap_t < (size_t)T) {
        const size_t cap = std::max<size_t>(16, 2 * (size_t)T);
        h->path_bits_cap_t = 0;
        HIPCK(mp_hipMalloc(h->path_bits, cap * words));
        h->path_bits_cap_t = cap;
    }
    std::vector<mp_hist_event> ev;   // (stays alive until the stream is idle: readout_finish waits on every path)
    MPCK(upload_hist_events(h, ev));
    double* const buf[2] = {h->scratch.buf[0].get(), h->scratch.buf[1].get()};
    double* res = h->scratch.res;   // {m, S[T][d], A, mean[T][d], V[T][d], distinct u64[T]}
    unsigned long long* d_distinct = reinterpret_cast<unsigned long long*>(res + 2 + 3 * TD);
    uint32_t* bitmap = distinct_out ? h->path_bits.get() : nullptr;
    if (bitmap) HIPCK(hipMemsetAsync(bitmap, 0, sizeof(uint32_t) * (size_t)T * words, h->stream));
    max_pass(h, g, res);
    for (int pass = 1; pass <= (var_out ? 2 : 1); ++pass) {
        mom_for_width(d, [&](auto D) { launch_path_pass<decltype(D)::value>(h, pass, (unsigned)g.nb, T, res, bitmap, words); });
        mom_close<mom_add>(h->stream, buf, g.nb, pass == 1 ? TD + 1 : TD, pass == 1 ? res + 1 : res + 2 + 2 * TD);
    }
    if (bitmap) hipLaunchKernelGGL(k_path_distinct, dim3((unsigned)T), dim3(MOM_THREADS), 0, h->stream, (const uint32_t*)bitmap, words, d_distinct);
    MPCK(readout_finish(h, "mp_pf_path_moments", hipGetLastError(), n_res));
    const double* r = h->scratch.host;
    const double A = r[1 + TD];
    for (size_t c = 0; c < TD; ++c) mean_out[c] = readout_mean(var_out != nullptr, r + 1, r + 2 + TD, A, c);
    if (var_out)
        for (size_t c = 0; c < TD; ++c) var_out[c] = r[2 + 2 * TD + c] / A;
    if (distinct_out) memcpy(distinct_out, r + 2 + 3 * TD, sizeof(uint64_t) * (size_t)T);
    return MP_OK;
}

// Weighted quantiles of every state component of the cloud, selected on the device: replaces sorting what a caller of the reference
// collects from its public `traces` / `log_weights` fields (particle_filter.rs:13-20) — here mp_pf_read_state + mp_pf_read_log_weights
// and a host sort.  Definition (integers only: the weighted inverted CDF over order-preserving keys): mp_quantiles.h, DESIGN.md
// section 4, "Quantiles".
int32_t mp_pf_quantiles(mp_pf* h, const double* qs, int32_t n_q, double* out) {
    if (!h || !qs || !out) return mp_fail(MP_ERR_INVALID_ARG, "null argument");
    q_spec spec;
    q_bufs b;
    size_t nsel = 0;
    MPCK(quantiles_begin(h, "mp_pf_quantiles", qs, n_q, false, spec, b, nsel));
    const int d = h->ops->dim_state;
    const hipError_t e1 = q_select(h->stream, b, nsel, n_q, d, spec, [&](int pass, int nq, const q_bufs& bb) {
        mom_for_width(d, [&](auto D) { launch_quantiles_hist<decltype(D)::value>(h, pass, nq, bb); });
    });
    MPCK(readout_finish(h, "mp_pf_quantiles", e1, 1 + nsel));
    memcpy(out, h->scratch.host + 1, sizeof(double) * nsel);
    return MP_OK;
}

// Weighted quantiles of the state at EVERY time step over the recorded ancestry (the bands of a fan chart), selected on the device:
// replaces walking `traces[i].retv` of every particle (particle_filter.rs:13; tests/smc.rs:67) and sorting per step on the host — here
// mp_pf_read_trajectories, n * T * d doubles over the link.  The weights of mp_pf_quantiles over v_ij(t) = x_t[anc_i(t)]; the walk of
// mp_pf_path_moments, once per pass.  Definition: mp_quantiles.h, DESIGN.md section 4, "Quantiles".
int32_t mp_pf_path_quantiles(mp_pf* h, const double* qs, int32_t n_q, double* out, int32_t* t_out) {
    if (!h || !qs || !out || !t_out) return mp_fail(MP_ERR_INVALID_ARG, "null argument");
    q_spec spec;
    q_bufs b;
    size_t nsel = 0;
    MPCK(quantiles_begin(h, "mp_pf_path_quantiles", qs, n_q, true, spec, b, nsel));
    *t_out = (int32_t)h->t;
    if (h->t == 0) return MP_OK;
    const int d = h->ops->dim_state;
    std::vector<mp_hist_event> ev;   // (stays alive until the stream is idle: readout_finish waits on every path)
    const int32_t up = upload_hist_events(h, ev);
    if (up != MP_OK) { (void)hipStreamSynchronize(h->stream); return up; }   // (a copy out of ev may be in flight: wait, then the status as it came)
    const hipError_t e1 = q_select(h->stream, b, nsel, n_q, d, spec, [&](int pass, int nq, const q_bufs& bb) {
        mom_for_width(d, [&](auto D) { launch_path_quantiles_hist<decltype(D)::value>(h, pass, nq, n_q, bb); });
    });
    MPCK(readout_finish(h, "mp_pf_path_quantiles", e1, 1 + nsel));
    memcpy(out, h->scratch.host + 1, sizeof(double) * nsel);
    return MP_OK;
}

int32_t mp_pf_forecast_paths(mp_pf* h, int32_t horizon, uint64_t first, uint64_t count, double* states_out, double* obs_out) {
    mp_forecast_args f;
    MPCK(forecast_begin(h, "forecast_paths", horizon, f));
    if (!states_out && !obs_out) return mp_fail(MP_ERR_INVALID_ARG, "forecast_paths: every output is null");
    if (first > h->n || count > h->n - first) return mp_fail(MP_ERR_INVALID_ARG, "forecast_paths: first + count exceeds the number of particles");
    MPCK(readout_begin(h, "forecast_paths", 0));
    f.x = h->x[h->cur];
    const size_t D = (size_t)h->ops->dim_state, DO = (size_t)h->ops->dim_obs, H = (size_t)horizon;
    // slots per launch: 2^22 doubles of states + observations on the device at a time, but never fewer than 2^16 slots (a launch that
    // fills the device), whatever the window and the horizon
    const u64 chunk = std::max<u64>(1, std::min<u64>(count, std::max<u64>((u64)1 << 16, ((u64)1 << 22) / (H * (D + DO)))));
    if (states_out) MPCK(fc_grow(h->fc_paths[0], h->fc_paths_cap[0], (size_t)chunk * H * D));
    if (obs_out) MPCK(fc_grow(h->fc_paths[1], h->fc_paths_cap[1], (size_t)chunk * H * DO));
    double* dx = states_out ? h->fc_paths[0].get() : nullptr;
    double* dy = obs_out ? h->fc_paths[1].get() : nullptr;
    hipError_t e = hipSuccess;
    for (u64 c0 = 0; c0 < count && e == hipSuccess; c0 += chunk) {
        const u64 cn = std::min<u64>(chunk, count - c0);
        h->ops->forecast_paths(f, first + c0, cn, dx, dy, h->stream);
        e = hipGetLastError();
        if (e == hipSuccess && dx) e = hipMemcpyAsync(states_out + (size_t)c0 * H * D, dx, sizeof(double) * (size_t)cn * H * D, hipMemcpyDeviceToHost, h->stream);
        if (e == hipSuccess && dy) e = hipMemcpyAsync(obs_out + (size_t)c0 * H * DO, dy, sizeof(double) * (size_t)cn * H * DO, hipMemcpyDeviceToHost, h->stream);
    }
    const hipError_t e2 = hipStreamSynchronize(h->stream);
    if (e == hipSuccess) e = e2;
    if (e != hipSuccess) return mp_fail(MP_ERR_HIP, std::string("mp_pf_forecast_paths: ") + hipGetErrorString(e));
    return MP_OK;
}

// The kernels reduce the state and the observation columns alike (Simulate mode draws the observations anyway); what the caller did
// not ask for is not copied out.
int32_t mp_pf_forecast_moments(mp_pf* h, int32_t horizon, double* state_mean_out, double* state_var_out, double* obs_mean_out, double* obs_var_out) {
    mp_forecast_args f;
    MPCK(forecast_begin(h, "forecast_moments", horizon, f));
    if (!state_mean_out && !state_var_out && !obs_mean_out && !obs_var_out) return mp_fail(MP_ERR_INVALID_ARG, "forecast_moments: every output is null");
    MPCK(readout_begin(h, "mp_pf_forecast_moments", RD_NO_SHARD | RD_KERNEL));
    f.x = h->x[h->cur];
    const int d = h->ops->dim_state, dobs = h->ops->dim_obs;
    const mom_grids g = mom_plan(h->n, d);
    const size_t C = (size_t)(d + dobs), H = (size_t)horizon, HC = H * C;
    MPCK(reserve_steps(h, H, C, g, 3 * C));
    double* const buf[2] = {h->scratch.buf[0].get(), h->scratch.buf[1].get()};
    double* res = h->scratch.res;   // {m, S[H][C], A, mean[H][C], V[H][C]}
    const bool want_var = state_var_out || obs_var_out;
    max_pass(h, g, res);
    for (int pass = 1; pass <= (want_var ? 2 : 1); ++pass) {
        h->ops->forecast_moments(f, pass, (unsigned)g.nb, h->logw, res, buf[0], h->stream);
        mom_close<mom_add>(h->stream, buf, g.nb, pass == 1 ? HC + 1 : HC, pass == 1 ? res + 1 : res + 2 + 2 * HC);
    }
    MPCK(readout_finish(h, "mp_pf_forecast_moments", hipGetLastError(), 2 + 3 * HC));
    const double* r = h->scratch.host;
    const double A = r[1 + HC];
    for (size_t k = 0; k < H; ++k)
        for (size_t c = 0; c < C; ++c) {
            const size_t col = k * C + c;
            const bool is_state = c < (size_t)d;
            double* mo = is_state ? state_mean_out : obs_mean_out;
            double* vo = is_state ? state_var_out : obs_var_out;
            const size_t o = is_state ? k * d + c : k * dobs + (c - d);
            if (mo) mo[o] = readout_mean(want_var, r + 1, r + 2 + HC, A, col);
            if (vo) vo[o] = r[2 + 2 * HC + col] / A;
        }
    return MP_OK;
}

}   // extern "C"
