// mp_models_counts.h — Unfold models with observed counts (mp_dists.h poisson), registered like mp_models_extra.h's; a header of its
// own because the CPU checker compiles mp_models.h (and with it mp_models_extra.h) against handlers that know only the reference's
// normal / uniform / categorical sites.  Included by mp_pf.hip after mp_models.h.
#pragma once
#include "mp_models.h"

// ---------------------------------------------------------------------------------------
// Poisson state-space model, kind 101, dim_state = dim_obs = 1: a latent AR(1) log-intensity observed through counts
//   t==0: h ~ normal(mu, sig0) %= "h";   t>0: h ~ normal(mu + phi (h_prev - mu), sigma) %= "h";   poisson(exp(h)) %= "y" observed
// params = {mu, phi, sigma, sig0}.  One free normal and a one-double state: at 2^20 particles it runs through the two-tile
// k_propagate_mt, as stochastic volatility (kind 100) does.
// ---------------------------------------------------------------------------------------
struct mp_poisson_ssm {
    static constexpr int DIM_STATE = 1, DIM_OBS = 1;
    enum { H = 0, Y = 1 };
    static constexpr int obs_of(int site) { return site == Y ? 0 : -1; }
    static constexpr int MAX_NORMALS = 1;
    static constexpr int normal_index(int site) { return site == H ? 0 : -1; }
    MP_HD int n_normals(int64_t) const { return 1; }
    MP_HD uint32_t normal_site(int) const { return H; }
    double mu, phi, sigma, sig0;

    template <class G>
    MP_HD void operator()(G& g, int64_t t, const double* prev, double* next) const {
        double h;
        if (t == 0) h = g.template normal<H>(mu, sig0);
        else h = g.template normal<H>(mu + phi * (prev[0] - mu), sigma);
        g.template poisson<Y>(g.exp_(h));
        next[0] = h;
    }
};
inline bool mp_parse_poisson_ssm(const mp_model_desc& m, mp_poisson_ssm& k, std::string& err) {
    if (m.n_params != 4 || !m.params || m.dim_state != 1 || m.dim_obs != 1) {
        err = "poisson state-space model: params = {mu, phi, sigma, sig0}, dim_state = dim_obs = 1";
        return false;
    }
    k.mu = m.params[0]; k.phi = m.params[1]; k.sigma = m.params[2]; k.sig0 = m.params[3];
    if (!(k.sigma > 0.) || !(k.sig0 > 0.) || !(k.sigma < 1e300) || !(k.sig0 < 1e300)) {
        err = "poisson state-space model: standard deviations must be finite and > 0";
        return false;
    }
    if (!(k.mu - k.mu == 0.) || !(k.phi - k.phi == 0.)) {
        err = "poisson state-space model: mu and phi must be finite";
        return false;
    }
    return true;
}
MP_REGISTER_UNFOLD_MODEL(101, mp_poisson_ssm, mp_parse_poisson_ssm)
