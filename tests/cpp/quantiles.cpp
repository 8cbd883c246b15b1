// The quantiles through the C++ wrapper (modppl_amd/cpp/modppl.hpp): a filter that records history takes init_step, resample, step,
// then quantiles(qs) and path_quantiles(qs); hierarchical function chains take site_quantiles(qs).  Prints the values as their bits,
// one line each, which tests/test_cpp_quantiles.py compares with the Python mirror (same C ABI underneath).
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "../../modppl_amd/cpp/modppl.hpp"

static void print_bits(const char* tag, const std::vector<double>& v) {
    std::printf("%s", tag);
    for (double x : v) {
        uint64_t b;
        std::memcpy(&b, &x, sizeof b);
        std::printf(" %016llx", (unsigned long long)b);
    }
    std::printf("\n");
}

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4096;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    const std::vector<double> qs = {0.5, 0.05, 0.95};
    try {
        modppl::ParticleSystem filter(modppl::UnfoldModel::lgssm(), n, seed, MP_PF_RECORD_HISTORY);
        filter.init_step({}, {0.31});
        filter.resample();
        filter.step({-0.12});
        print_bits("cloud", filter.quantiles(qs));
        print_bits("path", filter.path_quantiles(qs));
        std::vector<double> xs(4);
        std::vector<std::pair<int32_t, double>> cons;
        for (int k = 0; k < 4; ++k) {
            xs[k] = -1.0 + 0.5 * k;
            cons.push_back({MP_SITE_Y0 + k, 0.25 * k - 0.1});
        }
        modppl::FunctionChains chains(MP_MH_MODEL_HIERARCHICAL_FN, xs, cons, n, seed);
        const modppl::FunctionChains::SiteQuantiles sq = chains.site_quantiles(qs);
        std::printf("count");
        for (uint64_t c : sq.count) std::printf(" %llu", (unsigned long long)c);
        std::printf("\n");
        print_bits("sites", sq.values);
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
