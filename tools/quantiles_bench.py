"""What a median and a credible interval cost per step: `step; resample; quantiles([0.05, 0.5, 0.95])` against the only route there was
before, `step; resample; states(out=pinned) + log_weights` plus the host-side sort they feed (numpy: per column an argsort, a running
sum of the weights and a search).  With --path: `path_quantiles` of a filter that recorded T steps against `trajectories()` plus the
same sort per time step.  The two routes alternate in one process, on one filter each with the same seed; times are host clocks around
loops whose every iteration ends in a synchronising call.

    python tools/quantiles_bench.py [--steps 20] [--warmup 3] [--rounds 3] [--which lgssm1,band16,hmm] [--loop-only quantiles]
    python tools/quantiles_bench.py --path [--n 262144] [--T 50] [--rounds 3] [--loop-only quantiles]

Prints one JSON line per (case, round) and a summary line per case.  --loop-only runs one of the routes alone (for a kernel trace of
its launches).  The host sort is slow (seconds per step at 2^21 x 16), so the default step counts are small."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

CASES = {"lgssm1": (1 << 20, 1), "band16": (1 << 21, 16), "hmm": (1 << 20, 1)}   # hmm: two-valued states, every key of a wave in one LDS bin
QS = [0.05, 0.5, 0.95]


def make(name):
    import modppl_amd

    n, d = CASES[name]
    if name == "hmm":
        return modppl_amd.hmm_model([0.5, 0.5], [[0.7, 0.2], [0.3, 0.8]], [[0.9, 0.3], [0.1, 0.7]]), n, d
    model = modppl_amd.lgssm_model() if d == 1 else modppl_amd.lgssm_band_model(16)
    return model, n, d


def pinned(n, d):
    import torch

    return torch.empty((n, d), dtype=torch.float64, pin_memory=True).numpy()


def host_quantiles(x, lw, qs):
    """the weighted inverted CDF per column, in floating point (what a user writes; not the library's integer definition)"""
    w = np.exp(lw - lw.max())
    out = np.empty((len(qs), x.shape[1]))
    for j in range(x.shape[1]):
        order = np.argsort(x[:, j], kind="stable")
        cum = np.cumsum(w[order])
        pos = np.minimum(np.searchsorted(cum, np.asarray(qs) * cum[-1], side="left"), len(order) - 1)
        out[:, j] = x[order[pos], j]
    return out


def loop_quantiles(pf, obs, steps, t0):
    for t in range(steps):
        pf.step(obs[(t0 + t) % len(obs)][None, :])
        pf.resample(sync=False)
        q = pf.quantiles(QS)
    return q


COPY_S = [0.0]   # seconds inside states(out=pinned) + log_weights (the wait for the step and the resample included) since it was last zeroed


def loop_copy(pf, obs, steps, t0, buf):
    for t in range(steps):
        pf.step(obs[(t0 + t) % len(obs)][None, :])
        pf.resample(sync=False)
        s = time.perf_counter()
        x = pf.states(out=buf)
        lw = pf.log_weights
        COPY_S[0] += time.perf_counter() - s
        q = host_quantiles(x, lw, QS)
    return q


def summary(row, us_q, us_c):
    if us_q:
        row.update(quantiles_us_median=float(np.median(us_q)), quantiles_us_min=min(us_q), quantiles_us_max=max(us_q))
    if us_c:
        row.update(host_route_us_median=float(np.median(us_c)), host_route_us_min=min(us_c), host_route_us_max=max(us_c))
    print(json.dumps(row), flush=True)


def bench_cloud(a):
    import modppl_amd

    for name in a.which.split(","):
        model, n, d = make(name)
        obs = np.random.default_rng(3).normal(0, 1.0, size=(64, d))
        if name == "hmm":
            obs = (obs > 0).astype(np.float64)
        pa, pb = modppl_amd.ParticleSystem(model, n, 11), modppl_amd.ParticleSystem(model, n, 11)
        pa.init_step(None, obs[:1])
        pb.init_step(None, obs[:1])
        buf = pinned(n, d)
        if a.loop_only != "copy":
            loop_quantiles(pa, obs, a.warmup, 1)
        if a.loop_only != "quantiles":
            loop_copy(pb, obs, a.warmup, 1, buf)
        us_q, us_c = [], []
        for r in range(a.rounds):
            t0 = 1 + a.warmup + r * a.steps
            row = {"model": name, "n": n, "d": d, "round": r, "steps": a.steps, "levels": QS}
            if a.loop_only != "copy":
                s = time.perf_counter()
                qa = loop_quantiles(pa, obs, a.steps, t0)
                us_q.append((time.perf_counter() - s) / a.steps * 1e6)
                row["quantiles_us_per_step"] = us_q[-1]
            if a.loop_only != "quantiles":
                COPY_S[0] = 0.0
                s = time.perf_counter()
                qb = loop_copy(pb, obs, a.steps, t0, buf)
                us_c.append((time.perf_counter() - s) / a.steps * 1e6)
                row["host_route_us_per_step"] = us_c[-1]
                row["of_which_step_resample_and_copy_us"] = COPY_S[0] / a.steps * 1e6
            if not a.loop_only:   # the two filters took the same steps: the same cloud, the same order statistics
                row["max_abs_diff"] = float(np.max(np.abs(qa - qb)))
            print(json.dumps(row), flush=True)
        summary({"model": name, "n": n, "d": d, "summary": True}, us_q, us_c)
        pa.close()
        pb.close()


def bench_path(a):
    import modppl_amd
    from modppl_amd import capi

    n, T = a.n, a.T
    obs = np.random.default_rng(3).normal(0, 1.0, size=(T, 1))
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(), n, 11, flags=capi.MP_PF_RECORD_HISTORY)
    pf.init_step(None, obs[:1])
    for t in range(1, T):
        pf.resample(sync=False)
        pf.step(obs[t:t + 1])
    us_q, us_c = [], []
    if a.loop_only != "copy":
        pf.path_quantiles(QS)
    for r in range(a.rounds):
        row = {"model": "lgssm1", "n": n, "d": 1, "T": T, "round": r, "levels": QS, "path": True}
        if a.loop_only != "copy":
            s = time.perf_counter()
            qa = pf.path_quantiles(QS)
            us_q.append((time.perf_counter() - s) * 1e6)
            row["path_quantiles_us"] = us_q[-1]
        if a.loop_only != "quantiles":
            s = time.perf_counter()
            paths, lw = pf.trajectories(), pf.log_weights
            row["of_which_trajectories_us"] = (time.perf_counter() - s) * 1e6
            qb = np.stack([host_quantiles(paths[:, t, :], lw, QS) for t in range(T)])
            us_c.append((time.perf_counter() - s) * 1e6)
            row["host_route_us"] = us_c[-1]
        if not a.loop_only:
            row["max_abs_diff"] = float(np.max(np.abs(qa - qb)))
        print(json.dumps(row), flush=True)
    summary({"model": "lgssm1", "n": n, "d": 1, "T": T, "path": True, "summary": True}, us_q, us_c)
    pf.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--which", default="lgssm1,band16")
    ap.add_argument("--loop-only", default="")
    ap.add_argument("--path", action="store_true")
    ap.add_argument("--n", type=int, default=1 << 18)
    ap.add_argument("--T", type=int, default=50)
    a = ap.parse_args()
    (bench_path if a.path else bench_cloud)(a)


if __name__ == "__main__":
    main()
