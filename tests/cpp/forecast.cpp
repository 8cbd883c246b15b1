// The forecast through the C++ wrapper (modppl_amd/cpp/modppl.hpp): init_step, resample, step, then forecast(3) and
// forecast_paths(3, 5, 2).  Prints one line that tests/test_cpp_forecast.py compares with the Python mirror (same C ABI underneath).
#include <cstdio>
#include <cstdlib>

#include "../../modppl_amd/cpp/modppl.hpp"

int main(int argc, char** argv) {
    const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 4096;
    const uint64_t seed = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 7;
    try {
        modppl::ParticleSystem filter(modppl::UnfoldModel::lgssm(), n, seed);
        filter.init_step({}, {0.31});
        filter.resample();
        filter.step({-0.12});
        const modppl::ParticleSystem::Forecast f = filter.forecast(3);
        const modppl::ParticleSystem::ForecastPaths p = filter.forecast_paths(3, 5, 2);
        const modppl::ParticleSystem::Forecast mean_only = filter.forecast(3, false, false);
        std::printf("mean2=%.17g var2=%.17g omean2=%.17g ovar2=%.17g x=%.17g y=%.17g sizes=%zu,%zu,%zu,%zu same=%d\n", f.state_mean[2], f.state_var[2],
                    f.obs_mean[2], f.obs_var[2], p.states[5], p.obs[5], p.states.size(), mean_only.state_var.size(), mean_only.obs_mean.size(),
                    mean_only.obs_var.size(), (int)(mean_only.state_mean == f.state_mean));
    } catch (const std::exception& e) {
        std::fprintf(stderr, "error: %s\n", e.what());
        return 1;
    }
    return 0;
}
