// dists_shim.cpp — the distributions of modppl_amd/csrc/mp_dists.h (and mp_lgamma / mp_log1p of mp_math.h) on the host, for
// tests/test_dists_host.py (compiled with g++ and the CPU checker's flags: -O2 -ffp-contract=off -mfma) and as the host side of the
// bit-for-bit comparisons with the device probe mp_probe_dist (include/modppl_hip_probe.h), whose arguments it takes.
#include <stdint.h>

#include "../../modppl_amd/csrc/mp_dists.h"

extern "C" {

// dist: 0 poisson(p0), 1 gamma(p0 shape, p1 scale), 2 beta(p0, p1), 3 geometric(p0), 4 uniform_discrete(p0, p1),
//       5 mp_lgamma(x), 6 mp_log1p(x) (op 0 only); 7 mp_exp(x) (op 0, here only: the rates of a model that draws exp(h))
// op 0: out[i] = logpdf(x[i]; p0[i], p1[i]);  op 1: out[i] = a sample with parameters (p0[i], p1[i]) from the stream of Philox
// coordinates (seed, slot0 + i, step, domain, site)
int32_t mp_shim_dist(int32_t dist, int32_t op, const double* x, const double* p0, const double* p1, int64_t n, uint64_t seed,
                     uint32_t slot0, uint32_t step, uint32_t domain, uint32_t site, double* out) {
    if (op != 0 && op != 1) return -1;
    for (int64_t i = 0; i < n; ++i) {
        const double a = p0 ? p0[i] : 0., b = p1 ? p1[i] : 0.;
        if (op == 0) {
            const double v = x[i];
            switch (dist) {
            case 0: out[i] = mp_poisson_logpdf(v, a); break;
            case 1: out[i] = mp_gamma_logpdf(v, a, b); break;
            case 2: out[i] = mp_beta_logpdf(v, a, b); break;
            case 3: out[i] = mp_geometric_logpdf(v, a); break;
            case 4: out[i] = mp_uniform_discrete_logpdf(v, a, b); break;
            case 5: out[i] = mp_lgamma(v); break;
            case 6: out[i] = mp_log1p(v); break;
            case 7: out[i] = mp_exp(v); break;
            default: return -1;
            }
        } else {
            mp_stream s;
            s.k0 = (uint32_t)seed; s.k1 = (uint32_t)(seed >> 32); s.slot = slot0 + (uint32_t)i; s.step = step;
            mp_site st(s, domain, site);
            switch (dist) {
            case 0: out[i] = mp_poisson_sample(st, a); break;
            case 1: out[i] = mp_gamma_sample(st, a, b); break;
            case 2: out[i] = mp_beta_sample(st, a, b); break;
            case 3: out[i] = mp_geometric_sample(st, a); break;
            case 4: out[i] = mp_uniform_discrete_sample(st, a, b); break;
            default: return -1;
            }
        }
    }
    return 0;
}

}  // extern "C"
