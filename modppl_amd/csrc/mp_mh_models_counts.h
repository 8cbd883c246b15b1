// mp_mh_models_counts.h — registered generative functions over the count and positive-real distributions (mp_dists.h: poisson,
// gamma, beta, geometric, uniform_discrete), kinds 130 - 132.  Same contract as mp_mh_models.h; a header of its own because the CPU
// checker compiles mp_mh_models.h against handlers that know only the distributions of the reference's inference tests.
// Observations are constraints on ordinary sites (the counts as doubles), as in the hierarchical model.
#pragma once
#include <string>

#include "mp_genfn.h"

// ---------------------------------------------------------------------------------------
// The Poisson model at the end of the reference's test_update (modppl/tests/dyngenfn.rs:277-301), kind 130:
//   k ~ poisson(rate) %= "k";  for i in 0..k { uniform(0, 1) %= ("value", i) }
// with a static cap of 31 value sites (V0 + i); a trace whose k exceeds it is the kernels' panic (simulate, which reports no panic,
// keeps the first 31 values).  params = {} (rate 5, the test's) or {rate}.
// ---------------------------------------------------------------------------------------
struct mp_poisson_update_fn {
    static constexpr int MAX_VALUES = 31;
    static constexpr int NS = 1 + MAX_VALUES;
    enum { K = 0, V0 = 1 };
    static constexpr uint32_t sub_of(int) { return 0u; }
    static constexpr bool is_bool(int) { return false; }
    double rate;
    template <class H, int J>
    MP_HD void values(H& g, double k) const {
        if ((double)J < k) g.template uniform<V0 + J>(0., 1.);
        if constexpr (J + 1 < MAX_VALUES) values<H, J + 1>(g, k);
    }
    template <class H>
    MP_HD void operator()(H& g) const {
        const double k = g.template poisson<K>(rate);
        if (k > (double)MAX_VALUES) g.panic = true;
        values<H, 0>(g, k);
    }
};
inline bool mp_parse_poisson_update_fn(const double* params, int n_params, mp_poisson_update_fn& m, std::string& err) {
    if (n_params > 1 || (n_params == 1 && (!params || !(params[0] > 0.) || !(params[0] < 1e300)))) {
        err = "poisson update model: params = {} or {rate > 0}";
        return false;
    }
    m.rate = n_params == 1 ? params[0] : 5.;
    return true;
}
MP_REGISTER_MH_MODEL(130, mp_poisson_update_fn, mp_parse_poisson_update_fn)

// ---------------------------------------------------------------------------------------
// Poisson change point, kind 131:
//   tau ~ uniform_discrete(1, n - 1);  l1 ~ gamma(a, b);  l2 ~ gamma(a, b);  y_j ~ poisson(j < tau ? l1 : l2), j < n   (observed)
// (gamma with shape a and SCALE b, gamma.rs).  params = {n, a, b}, 2 <= n <= 29; the observations are constraints on Y0 + j.
// ---------------------------------------------------------------------------------------
struct mp_changepoint_fn {
    static constexpr int MAX_DATA = 29;
    static constexpr int NS = 3 + MAX_DATA;
    enum { TAU = 0, L1 = 1, L2 = 2, Y0 = 3 };
    static constexpr uint32_t sub_of(int) { return 0u; }
    static constexpr bool is_bool(int) { return false; }
    int n;
    double a, b;
    template <class H, int J>
    MP_HD void ys(H& g, double tau, double l1, double l2) const {
        if (J < n) g.template poisson<Y0 + J>((double)J < tau ? l1 : l2);
        if constexpr (J + 1 < MAX_DATA) ys<H, J + 1>(g, tau, l1, l2);
    }
    template <class H>
    MP_HD void operator()(H& g) const {
        const double tau = g.template uniform_discrete<TAU>(1., (double)(n - 1));
        const double l1 = g.template gamma<L1>(a, b);
        const double l2 = g.template gamma<L2>(a, b);
        ys<H, 0>(g, tau, l1, l2);
    }
};
inline bool mp_parse_changepoint_fn(const double* params, int n_params, mp_changepoint_fn& m, std::string& err) {
    if (!params || n_params != 3 || !(params[0] >= 2. && params[0] <= mp_changepoint_fn::MAX_DATA) || params[0] != (double)(int)params[0] ||
        !(params[1] > 0. && params[1] < 1e300) || !(params[2] > 0. && params[2] < 1e300)) {
        err = "poisson change point: params = {n, a, b}, 2 <= n <= 29 an integer, shape a > 0, scale b > 0";
        return false;
    }
    m.n = (int)params[0];
    m.a = params[1];
    m.b = params[2];
    return true;
}
MP_REGISTER_MH_MODEL(131, mp_changepoint_fn, mp_parse_changepoint_fn)

// ---------------------------------------------------------------------------------------
// Beta-geometric, kind 132:  p ~ beta(a, b);  k_j ~ geometric(p), j < n   (observed: constraints on K0 + j)
// params = {n, a, b}, 1 <= n <= 30.
// ---------------------------------------------------------------------------------------
struct mp_beta_geometric_fn {
    static constexpr int MAX_DATA = 30;
    static constexpr int NS = 1 + MAX_DATA;
    enum { P = 0, K0 = 1 };
    static constexpr uint32_t sub_of(int) { return 0u; }
    static constexpr bool is_bool(int) { return false; }
    int n;
    double a, b;
    template <class H, int J>
    MP_HD void ks(H& g, double p) const {
        if (J < n) g.template geometric<K0 + J>(p);
        if constexpr (J + 1 < MAX_DATA) ks<H, J + 1>(g, p);
    }
    template <class H>
    MP_HD void operator()(H& g) const {
        const double p = g.template beta<P>(a, b);
        ks<H, 0>(g, p);
    }
};
inline bool mp_parse_beta_geometric_fn(const double* params, int n_params, mp_beta_geometric_fn& m, std::string& err) {
    if (!params || n_params != 3 || !(params[0] >= 1. && params[0] <= mp_beta_geometric_fn::MAX_DATA) || params[0] != (double)(int)params[0] ||
        !(params[1] > 0. && params[1] < 1e300) || !(params[2] > 0. && params[2] < 1e300)) {
        err = "beta-geometric: params = {n, a, b}, 1 <= n <= 30 an integer, a > 0, b > 0";
        return false;
    }
    m.n = (int)params[0];
    m.a = params[1];
    m.b = params[2];
    return true;
}
MP_REGISTER_MH_MODEL(132, mp_beta_geometric_fn, mp_parse_beta_geometric_fn)
