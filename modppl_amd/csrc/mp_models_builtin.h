// mp_models_builtin.h — the factories of the eight built-in Unfold models (MP_MODEL_* of include/modppl_hip.h), entered into the
// same registry MP_REGISTER_UNFOLD_MODEL fills (model_registry(), mp_pf.hip).  Included by mp_pf.hip only, after ModelOpsT and the
// registry, as mp_models_counts.h is.  A factory rather than a `parse` callback is the registered unit because MP_MODEL_LGSSM_BAND
// maps one kind to three types, MP_MODEL_LGSSM_DENSE allocates device memory its ModelOps must own, and a descriptor can be
// MP_ERR_UNSUPPORTED as well as MP_ERR_INVALID_ARG.  The functors themselves: mp_models.h.
// (compiled in the device pass too: `new ModelOpsT<M>` is what makes hipcc emit k_propagate<M, ...> and k_simulate<M>)
#pragma once

static int32_t make_lgssm1(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params != 5 || !m->params) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM1 takes 5 params {mu0,sig0,a,sig_x,sig_y}");
    if (m->dim_state != 1 || m->dim_obs != 1) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM1: dim_state = dim_obs = 1");
    mp_lgssm1 k{m->params[0], m->params[1], m->params[2], m->params[3], m->params[4], 0.};
    if (!(k.sig0 > 0.) || !(k.sig_x > 0.) || !(k.sig_y > 0.)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM1: standard deviations must be > 0");
    k.ln_sig_y = mp_log(k.sig_y);
    out.reset(new ModelOpsT<mp_lgssm1>(k));
    return MP_OK;
}

static int32_t make_spiral(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->dim_state != 2 || m->dim_obs != 2) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_SPIRAL: dim_state = dim_obs = 2");
    mp_spiral k;
    const std::vector<double> cov = {0.001, 0., 0., 0.001};  // unfold.rs:29
    std::vector<double> inv;
    if (!mp_host_inverse(cov, 2, inv)) return mp_fail(MP_ERR_INVALID_ARG, "covariance not invertible");
    for (int i = 0; i < 4; ++i) k.cov_inv[i] = inv[i];
    k.ln_det = mp_log(mp_host_det(cov, 2));
    std::vector<double> L;
    if (!mp_host_cholesky(cov, 2, L)) return mp_fail(MP_ERR_INVALID_ARG, "covariance not positive definite");
    for (int i = 0; i < 4; ++i) { k.chol[i] = L[i]; k.cov[i] = cov[i]; }
    out.reset(new ModelOpsT<mp_spiral>(k));
    return MP_OK;
}

static int32_t make_hmm(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params < 2 || !m->params) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: params = {S, O, prior[S], emission[O][S], transition[S][S]}");
    const int S = (int)m->params[0], O = (int)m->params[1];
    if (S < 1 || O < 1 || S > MP_HMM_MAX || O > MP_HMM_MAX) return mp_fail(MP_ERR_UNSUPPORTED, "MP_MODEL_HMM: 1..8 states / observations");
    if (m->n_params != 2 + S + O * S + S * S) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: params length mismatch");
    if (m->dim_state != 1 || m->dim_obs != 1) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: dim_state = dim_obs = 1");
    mp_hmm k{};
    k.n_states = S; k.n_obs = O;
    const double* prior = m->params + 2;
    const double* emis = prior + S;
    const double* trans = emis + O * S;
    auto sums_to_one = [](const double* p, int n, int stride) {  // categorical.rs:13,23: assert |sum - 1| <= 1e-8
        double s_ = 0.;
        for (int i = 0; i < n; ++i) s_ += p[i * stride];
        return std::fabs(s_ - 1.0) <= 1e-8;
    };
    if (!sums_to_one(prior, S, 1)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: prior does not sum to 1 (eps 1e-8)");
    for (int s_ = 0; s_ < S; ++s_) {
        if (!sums_to_one(emis + s_, O, S)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: emission column does not sum to 1");
        if (!sums_to_one(trans + s_, S, S)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_HMM: transition column does not sum to 1");
    }
    for (int s_ = 0; s_ < S; ++s_) k.prior[s_] = prior[s_];
    for (int s_ = 0; s_ < S; ++s_) {
        for (int o = 0; o < O; ++o) k.emission_col[s_][o] = emis[o * S + s_];
        for (int s2 = 0; s2 < S; ++s2) k.transition_col[s_][s2] = trans[s2 * S + s_];
    }
    out.reset(new ModelOpsT<mp_hmm>(k));
    return MP_OK;
}

static int32_t make_bearings(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params != 6 || !m->params) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_BEARINGS takes 6 params {p0x,p0y,sig_p0,sig_v0,sig_a,sig_theta}");
    if (m->dim_state != 4 || m->dim_obs != 1) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_BEARINGS: dim_state = 4, dim_obs = 1");
    mp_bearings k{m->params[0], m->params[1], m->params[2], m->params[3], m->params[4], m->params[5], 0.};
    if (!(k.sig_p0 > 0.) || !(k.sig_v0 > 0.) || !(k.sig_a > 0.) || !(k.sig_theta > 0.)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_BEARINGS: standard deviations must be > 0");
    k.ln_sig_theta = mp_log(k.sig_theta);
    out.reset(new ModelOpsT<mp_bearings>(k));
    return MP_OK;
}

template <int D>
static ModelOps* new_lgssm_band(const double* p, double ln_sy) {
    return new ModelOpsT<mp_lgssm_band<D>>(mp_lgssm_band<D>{p[1], p[2], p[3], p[4], p[5], ln_sy});
}
static int32_t make_lgssm_band(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params != 6 || !m->params) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_BAND takes 6 params {D,a,band,sig0,sig_x,sig_y}");
    const int D = (int)m->params[0];
    if (m->dim_state != D || m->dim_obs != D) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_BAND: dim_state = dim_obs = D");
    if (!(m->params[3] > 0.) || !(m->params[4] > 0.) || !(m->params[5] > 0.)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_BAND: standard deviations must be > 0");
    const double ln_sy = mp_log(m->params[5]);
    if (D == 16) out.reset(new_lgssm_band<16>(m->params, ln_sy));
    else if (D == 4) out.reset(new_lgssm_band<4>(m->params, ln_sy));
    else if (D == 2) out.reset(new_lgssm_band<2>(m->params, ln_sy));
    else return mp_fail(MP_ERR_UNSUPPORTED, "MP_MODEL_LGSSM_BAND: D in {2, 4, 16} is compiled in");
    return MP_OK;
}

static int32_t make_pointed2d(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params != 8 || !m->params) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_POINTED_2D takes 8 params {xmin,xmax,ymin,ymax, cov row-major}");
    if (m->dim_state != 2 || m->dim_obs != 2) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_POINTED_2D: dim_state = dim_obs = 2");
    if (!(m->params[1] > m->params[0]) || !(m->params[3] > m->params[2])) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_POINTED_2D: xmax > xmin and ymax > ymin");
    mp_pointed2d k{};
    k.xmin = m->params[0]; k.xmax = m->params[1]; k.ymin = m->params[2]; k.ymax = m->params[3];
    const std::vector<double> cov(m->params + 4, m->params + 8);
    std::vector<double> inv;
    const double det = mp_host_det(cov, 2);
    if (!(det > 0.) || !mp_host_inverse(cov, 2, inv)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_POINTED_2D: covariance must be invertible with a positive determinant");
    for (int i = 0; i < 4; ++i) k.cov_inv[i] = inv[i];
    k.ln_det = mp_log(det);
    std::vector<double> L;
    if (!mp_host_cholesky(cov, 2, L)) return mp_fail(MP_ERR_UNSUPPORTED, "MP_MODEL_POINTED_2D: covariance without a Cholesky factor (the reference's eigen fallback is not built)");
    for (int i = 0; i < 4; ++i) k.chol[i] = L[i];
    out.reset(new ModelOpsT<mp_pointed2d>(k));
    return MP_OK;
}

static int32_t make_line(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (m->n_params != 11 || !m->params || m->dim_obs != 11 || m->dim_state != 2)
        return mp_fail(MP_ERR_UNSUPPORTED, "MP_MODEL_LINE: the 11-point design of tests/importance.rs:62 is compiled in (params = xs[11], dim_state = 2, dim_obs = 11)");
    mp_line<11> k{};
    for (int i = 0; i < 11; ++i) k.xs[i] = m->params[i];
    k.ln_noise = mp_log(0.1);
    out.reset(new ModelOpsT<mp_line<11>>(k));
    return MP_OK;
}

static int32_t make_lgssm_dense(const mp_model_desc* m, std::unique_ptr<ModelOps>& out) {
    if (!m->params || m->n_params < 2) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_DENSE: params = {D, sig0, A[D*D], Q[D*D], R[D*D]}");
    const int D = (int)m->params[0];
    if (D != 16) return mp_fail(MP_ERR_UNSUPPORTED, "MP_MODEL_LGSSM_DENSE: D = 16 is compiled in (one matrix-core tile)");
    if (m->n_params != 2 + 3 * D * D || m->dim_state != D || m->dim_obs != D)
        return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_DENSE: n_params = 2 + 3 D^2, dim_state = dim_obs = D");
    const double sig0 = m->params[1];
    if (!(sig0 > 0.)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_DENSE: sig0 must be > 0");
    const double* q = m->params + 2;
    const std::vector<double> A(q, q + D * D), Q(q + D * D, q + 2 * D * D), R(q + 2 * D * D, q + 3 * D * D);
    // the per-call nalgebra work of mvnormal.rs:17-18,27-33, once: transform of Q / sig0^2 I / R, inverse and ln det of R
    std::vector<double> cov0((size_t)D * D, 0.), TQ, T0, TR, Rinv;
    for (int i = 0; i < D; ++i) cov0[i * D + i] = sig0 * sig0;
    mp_host_mvnormal_transform(Q, D, TQ);
    mp_host_mvnormal_transform(cov0, D, T0);
    mp_host_mvnormal_transform(R, D, TR);
    const double detR = mp_host_det(R, D);
    if (!mp_host_inverse(R, D, Rinv)) return mp_fail(MP_ERR_INVALID_ARG, "MP_MODEL_LGSSM_DENSE: R is not invertible (try_inverse().unwrap() panics, mvnormal.rs:18)");
    std::vector<double> mats;
    mats.insert(mats.end(), A.begin(), A.end());
    mats.insert(mats.end(), TQ.begin(), TQ.end());
    mats.insert(mats.end(), T0.begin(), T0.end());
    mats.insert(mats.end(), Rinv.begin(), Rinv.end());
    mats.insert(mats.end(), TR.begin(), TR.end());
    mp_dev<double> d_mats;
    HIPCK(mp_hipMalloc(d_mats, mats.size()));
    if (hipMemcpy(d_mats, mats.data(), sizeof(double) * mats.size(), hipMemcpyHostToDevice) != hipSuccess)
        return mp_fail(MP_ERR_HIP, "MP_MODEL_LGSSM_DENSE: copying the model matrices failed");
    mp_lgssm_dense<16> k{d_mats, mp_log(detR)};
    auto* ops = new ModelOpsT<mp_lgssm_dense<16>>(k);
    ops->owned_device_mem = std::move(d_mats);
    out.reset(ops);
    return MP_OK;
}

static const int mp_registered_builtin[] = {
    mp_register_model_factory(MP_MODEL_LGSSM1, make_lgssm1),         mp_register_model_factory(MP_MODEL_SPIRAL, make_spiral),
    mp_register_model_factory(MP_MODEL_HMM, make_hmm),               mp_register_model_factory(MP_MODEL_BEARINGS, make_bearings),
    mp_register_model_factory(MP_MODEL_LGSSM_BAND, make_lgssm_band), mp_register_model_factory(MP_MODEL_POINTED_2D, make_pointed2d),
    mp_register_model_factory(MP_MODEL_LINE, make_line),             mp_register_model_factory(MP_MODEL_LGSSM_DENSE, make_lgssm_dense),
};
