"""What a look at the posterior costs per step: `step; resample; moments()` against the only route there was before,
`step; resample; states(out=pinned)` plus the host-side reduction it feeds (numpy: the weights are uniform behind a resample, so the
reduction is a mean and a covariance over the rows).  The two loops alternate in one process, on one filter each with the same seed;
times are host clocks around loops whose every iteration ends in a synchronising call.

    python tools/moments_bench.py [--steps 200] [--warmup 20] [--rounds 5] [--which lgssm1,band16] [--loop-only moments]

Prints one JSON line per (model, round) and a summary line per model.  --loop-only runs one of the loops alone (for a kernel trace of
its launches).  Bytes the reduction reads: (8 d + 8) N per pass, two passes plus 8 N for the max."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"lgssm1": (1 << 20, 1), "band16": (1 << 21, 16)}


def make(name):
    import modppl_amd

    n, d = CASES[name]
    model = modppl_amd.lgssm_model() if d == 1 else modppl_amd.lgssm_band_model(16)
    return model, n, d


def pinned(n, d):
    import torch

    return torch.empty((n, d), dtype=torch.float64, pin_memory=True).numpy()


def loop_moments(pf, obs, steps, t0):
    for t in range(steps):
        pf.step(obs[(t0 + t) % len(obs)][None, :])
        pf.resample(sync=False)
        mean, cov = pf.moments()
    return mean, cov


COPY_S = [0.0]   # seconds inside states(out=pinned) (the wait for the step and the resample included) since it was last zeroed


def loop_copy(pf, obs, steps, t0, buf):
    for t in range(steps):
        pf.step(obs[(t0 + t) % len(obs)][None, :])
        pf.resample(sync=False)
        s = time.perf_counter()
        x = pf.states(out=buf)
        COPY_S[0] += time.perf_counter() - s
        mean = x.mean(axis=0)
        c = x - mean
        cov = c.T @ c / len(x)
    return mean, cov


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--which", default="lgssm1,band16")
    ap.add_argument("--loop-only", default="")
    a = ap.parse_args()
    import modppl_amd

    for name in a.which.split(","):
        model, n, d = make(name)
        obs = np.random.default_rng(3).normal(0, 1.0, size=(64, d))
        pa, pb = modppl_amd.ParticleSystem(model, n, 11), modppl_amd.ParticleSystem(model, n, 11)
        pa.init_step(None, obs[:1])
        pb.init_step(None, obs[:1])
        buf = pinned(n, d)
        if a.loop_only != "copy":
            loop_moments(pa, obs, a.warmup, 1)
        if a.loop_only != "moments":
            loop_copy(pb, obs, a.warmup, 1, buf)
        us_m, us_c = [], []
        for r in range(a.rounds):
            t0 = 1 + a.warmup + r * a.steps
            row = {"model": name, "n": n, "d": d, "round": r, "steps": a.steps}
            if a.loop_only != "copy":
                s = time.perf_counter()
                ma = loop_moments(pa, obs, a.steps, t0)
                us_m.append((time.perf_counter() - s) / a.steps * 1e6)
                row["moments_us_per_step"] = us_m[-1]
            if a.loop_only != "moments":
                COPY_S[0] = 0.0
                s = time.perf_counter()
                mb = loop_copy(pb, obs, a.steps, t0, buf)
                us_c.append((time.perf_counter() - s) / a.steps * 1e6)
                row["pinned_copy_us_per_step"] = us_c[-1]
                row["of_which_step_resample_and_copy_us"] = COPY_S[0] / a.steps * 1e6
            if not a.loop_only:   # the two filters took the same steps: the same posterior, up to the order of the host's sums
                row["max_abs_mean_diff"] = float(np.max(np.abs(ma[0] - mb[0])))
            print(json.dumps(row), flush=True)
        summ = {"model": name, "n": n, "d": d, "summary": True, "bytes_read_per_call": (8 * d + 8) * n * 2 + 8 * n}
        if us_m:
            summ.update(moments_us_median=float(np.median(us_m)), moments_us_min=min(us_m), moments_us_max=max(us_m))
        if us_c:
            summ.update(pinned_copy_us_median=float(np.median(us_c)), pinned_copy_us_min=min(us_c), pinned_copy_us_max=max(us_c))
        print(json.dumps(summ), flush=True)
        pa.close()
        pb.close()


if __name__ == "__main__":
    main()
