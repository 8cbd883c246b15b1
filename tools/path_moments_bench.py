"""What the smoothed moments of a finished filter cost: `path_moments()` against the only route there was before, `trajectories()`
into numpy plus the reduction over particles — on the SAME handle, after `init_step; {resample; step} * (T - 1)` with history
recorded.  Times are host clocks around synchronous calls; the two routes alternate, five rounds, medians.

    python tools/path_moments_bench.py [--T 50] [--rounds 5] [--which lgssm1,band16]

Prints one JSON line per (model, round) and a summary line per model.  The device route reads about T n (4 + 8 d) bytes per pass (the
parents and the gathered rows; lineages coalesce going back, so the gathers turn cache-resident), two passes with the variance; the
host route moves 8 n T d bytes over the link and then reads them again."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"lgssm1": (1 << 20, 1), "band16": (1 << 21, 16)}


def host_route(pf):
    """-> (mean [T, d], var [T, d], seconds inside trajectories()): the reduction a caller writes over the lineages"""
    s = time.perf_counter()
    paths = pf.trajectories()
    copy_s = time.perf_counter() - s
    lw = pf.log_weights
    w = np.exp(lw - lw.max())
    w /= w.sum()
    mean = np.einsum("i,itj->tj", w, paths)
    var = np.einsum("i,itj,itj->tj", w, paths, paths) - mean * mean     # (one pass, no centred copy of n T d doubles)
    return mean, var, copy_s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--T", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--which", default="lgssm1,band16")
    a = ap.parse_args()
    import modppl_amd
    from modppl_amd import capi

    for name in a.which.split(","):
        n, d = CASES[name]
        model = modppl_amd.lgssm_model() if d == 1 else modppl_amd.lgssm_band_model(16)
        obs = np.random.default_rng(3).normal(0, 1.0, size=(a.T, d))
        pf = modppl_amd.ParticleSystem(model, n, 11, flags=capi.MP_PF_RECORD_HISTORY)
        pf.init_step(None, obs[:1])
        for t in range(1, a.T):
            pf.resample(sync=False)
            pf.step(obs[t:t + 1])
        pf.path_moments(var=True, distinct=True)     # (sizes the scratch)
        us = {"path_moments": [], "path_moments_mean_only": [], "path_moments_with_distinct": [], "host_route": [], "of_which_trajectories": []}
        for r in range(a.rounds):
            s = time.perf_counter()
            mean, var, _ = pf.path_moments()
            us["path_moments"].append((time.perf_counter() - s) * 1e6)
            s = time.perf_counter()
            pf.path_moments(var=False)
            us["path_moments_mean_only"].append((time.perf_counter() - s) * 1e6)
            s = time.perf_counter()
            _, _, k = pf.path_moments(distinct=True)
            us["path_moments_with_distinct"].append((time.perf_counter() - s) * 1e6)
            s = time.perf_counter()
            hm, hv, copy_s = host_route(pf)
            us["host_route"].append((time.perf_counter() - s) * 1e6)
            us["of_which_trajectories"].append(copy_s * 1e6)
            row = {"model": name, "n": n, "d": d, "T": a.T, "round": r}
            row.update({key + "_us": v[-1] for key, v in us.items()})
            row["max_abs_mean_diff"] = float(np.max(np.abs(mean - hm)))     # the same posterior, up to the order of the host's sums
            row["max_abs_var_diff"] = float(np.max(np.abs(var - hv)))
            row["distinct_first_last"] = [int(k[0]), int(k[-1])]
            print(json.dumps(row), flush=True)
        summ = {"model": name, "n": n, "d": d, "T": a.T, "summary": True, "rounds": a.rounds,
                "device_bytes_per_pass_upper": a.T * n * (4 + 8 * d), "host_route_bytes_over_link": 8 * n * a.T * d}
        for key, v in us.items():
            summ.update({key + "_us_median": float(np.median(v)), key + "_us_min": min(v), key + "_us_max": max(v)})
        print(json.dumps(summ), flush=True)
        pf.close()


if __name__ == "__main__":
    main()
