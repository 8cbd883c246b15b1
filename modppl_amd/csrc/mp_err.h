// mp_err.h — the one error idiom of the library's host code (mp_pf.hip, mp_mh.hip, mp_mh_fn.h, mp_shard_native.h, mp_probe.hip).
// Every entry point returns an int32_t status (include/modppl_hip.h) and leaves its message where mp_last_error() finds it: that
// thread-local lives in mp_pf.hip, and mp_set_error is how every translation unit writes it.  Here: HIPCK, MPCK, the degenerate-weights
// failure and check_scheme.  The `world` / `rank` checks of the sharded entry points (check_world, check_world_rank) read the handle
// and SH_MAX_WORLD, so they sit next to struct mp_pf in mp_pf.hip, the only translation unit with worlds.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/modppl_hip.h"

int32_t mp_set_error(int32_t code, const std::string& msg);   // mp_pf.hip: stores msg, returns code

// a HIP call that must succeed: MP_ERR_HIP and "<the call>: <HIP's message>" otherwise
#define HIPCK(call)                                                                                       \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess)                                                                             \
            return mp_set_error(MP_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_));           \
    } while (0)
// a status of the library's own: evaluated once, returned as it is unless MP_OK (whoever produced it has set the message)
#define MPCK(expr)                                  \
    do {                                            \
        const int32_t mpck_rc_ = (expr);            \
        if (mpck_rc_ != MP_OK) return mpck_rc_;     \
    } while (0)

static inline int32_t mp_fail_degenerate() {
    return mp_set_error(MP_ERR_DEGENERATE, "all log-weights are -inf: normalized weights are NaN (categorical.rs:23 assert in the reference)");
}
// `split`: the entry point also takes MP_RESAMPLE_MULTINOMIAL_SPLIT (the sharded count)
static inline int32_t check_scheme(int32_t scheme, bool split = false) {
    if (scheme != MP_RESAMPLE_MULTINOMIAL && scheme != MP_RESAMPLE_SYSTEMATIC && scheme != MP_RESAMPLE_STRATIFIED &&
        !(split && scheme == MP_RESAMPLE_MULTINOMIAL_SPLIT))
        return mp_set_error(MP_ERR_INVALID_ARG, "unknown resampling scheme");
    return MP_OK;
}
