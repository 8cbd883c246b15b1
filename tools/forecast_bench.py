"""What a forecast costs: `forecast(var=False)`, `forecast()` and `forecast_paths()` into a pinned buffer, for H in {1, 10, 50}, against
the per-step propagate time of the SAME handle (mp_pf_get_timing(MP_K_PROPAGATE) over a `{resample; step}` loop: unchanged code).
Times are host clocks around the synchronous calls, profiler off; five rounds, medians.

    python tools/forecast_bench.py [--rounds 5] [--which lgssm1,band16] [--horizons 1,10,50] [--steps 20]

Prints one JSON line per (model, H, round) and a summary line per (model, H).  The comparison to read is the mean-only forecast against
H x the step time: the forecast moves no particle (it reads n (8 d + 8) bytes once and writes partials only, where H steps read and
write the cloud H times), but its normal deviates come from in-lane rejection loops where the step's come from the cooperative pre-draw.
forecast_paths writes count * H * (d + dobs) doubles over the link; its window is capped (--paths-doubles) so that the d = 16 case at
H = 50 stays a buffer of 1 GiB rather than 27 — the line records the count it ran."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"lgssm1": (1 << 20, 1), "band16": (1 << 21, 16)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--which", default="lgssm1,band16")
    ap.add_argument("--horizons", default="1,10,50")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--paths-doubles", type=int, default=1 << 27)
    a = ap.parse_args()
    import torch

    import modppl_amd
    from modppl_amd import capi

    for name in a.which.split(","):
        n, d = CASES[name]
        model = modppl_amd.lgssm_model() if d == 1 else modppl_amd.lgssm_band_model(16)
        obs = np.random.default_rng(3).normal(0, 1.0, size=(a.steps + 1, d))
        pf = modppl_amd.ParticleSystem(model, n, 11)
        pf.init_step(None, obs[:1])
        for t in range(1, 4):                       # (warm-up: the first launches of every kernel)
            pf.resample(sync=False)
            pf.step(obs[t:t + 1])
        pf.synchronize()
        pf.set_timing(True)
        for t in range(4, a.steps + 1):
            pf.resample(sync=False)
            pf.step(obs[t:t + 1])
        pf.synchronize()
        ms, launches = pf.get_timing(capi.MP_K_PROPAGATE)
        pf.set_timing(False)
        step_us = ms * 1e3 / launches
        form = pf.last_propagate_form()
        for H in [int(h) for h in a.horizons.split(",")]:
            count = int(min(n, max(1, a.paths_doubles // (H * 2 * d))))
            px = torch.empty((count, H, d), dtype=torch.float64, pin_memory=True).numpy()
            py = torch.empty((count, H, d), dtype=torch.float64, pin_memory=True).numpy()
            pf.forecast(H)                               # (sizes the scratch, first launches)
            pf.forecast_paths(H, 0, count, out=(px, py))
            us = {"forecast_mean_only": [], "forecast": [], "forecast_paths": []}
            for r in range(a.rounds):
                s = time.perf_counter()
                pf.forecast(H, var=False)
                us["forecast_mean_only"].append((time.perf_counter() - s) * 1e6)
                s = time.perf_counter()
                pf.forecast(H)
                us["forecast"].append((time.perf_counter() - s) * 1e6)
                s = time.perf_counter()
                pf.forecast_paths(H, 0, count, out=(px, py))
                us["forecast_paths"].append((time.perf_counter() - s) * 1e6)
                row = {"model": name, "n": n, "d": d, "H": H, "round": r, "paths_count": count}
                row.update({key + "_us": v[-1] for key, v in us.items()})
                print(json.dumps(row), flush=True)
            summ = {"model": name, "n": n, "d": d, "H": H, "summary": True, "rounds": a.rounds, "paths_count": count,
                    "paths_bytes_over_link": 8 * count * H * 2 * d, "propagate_step_us": step_us, "propagate_launches_timed": int(launches),
                    "propagate_form": form}
            for key, v in us.items():
                summ.update({key + "_us_median": float(np.median(v)), key + "_us_min": min(v), key + "_us_max": max(v)})
            summ["mean_only_over_H_steps"] = summ["forecast_mean_only_us_median"] / (H * step_us)
            print(json.dumps(summ), flush=True)
            del px, py
        pf.close()


if __name__ == "__main__":
    main()
