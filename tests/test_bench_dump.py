"""CPU: bench.py --dump-outputs writes what the timed path's last step left to its caller, as float64 .npy files under a 64 MB
budget (a fixed, seeded sample of the particles when the population is larger).  A stand-in filter supplies the arrays."""
import os

import numpy as np

import bench


class FakeFilter:
    def __init__(self, n, d, seed):
        r = np.random.default_rng(seed)
        self.x = r.normal(size=(n, d))
        self.p = r.integers(0, n, size=n).astype(np.uint32)
        self.w = np.zeros(n)
        self.queries = 0

    def log_marginal_likelihood_estimate(self):
        self.queries += 1
        return -12.5

    def states(self):
        return self.x.copy()

    @property
    def parents(self):
        return self.p.copy()

    @property
    def log_weights(self):
        return self.w.copy()


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def _size(d):
    return sum(os.path.getsize(os.path.join(d, f)) for f in os.listdir(d))


def test_small_population_is_dumped_whole(tmp_path):
    pf = FakeFilter(4096, 2, 1)
    bench.dump_outputs(pf, str(tmp_path), 0, 1)
    out = _load(tmp_path)
    assert sorted(out) == ["log_ml", "log_weights", "parents", "states"]
    assert all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["states"], pf.x) and np.array_equal(out["parents"], pf.p) and np.array_equal(out["log_weights"], pf.w)
    assert out["log_ml"].tolist() == [-12.5] and pf.queries == 1


def test_large_population_is_a_fixed_sample_within_the_budget(tmp_path):
    n = 3 << 20   # 3 * 2^20 particles x (1 state + parent + log-weight) x 8 B = 75 MB: over the budget
    pf = FakeFilter(n, 1, 2)
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(pf, str(a), 0, 1)
    bench.dump_outputs(pf, str(b), 0, 1)
    assert _size(a) <= bench.DUMP_BYTES
    oa, ob = _load(a), _load(b)
    assert sorted(oa) == ["log_ml", "log_weights", "parents", "sample_index", "states"]
    assert all(np.array_equal(oa[k], ob[k]) for k in oa)   # the same sample every run
    idx = oa["sample_index"].astype(np.int64)
    assert idx.size > n // 2 and np.all(np.diff(idx) > 0) and idx[-1] < n
    assert np.array_equal(oa["states"], pf.x[idx]) and np.array_equal(oa["parents"], pf.p[idx])


def test_each_rank_writes_its_shard_under_a_shared_budget(tmp_path):
    world = 4
    for r in range(world):
        bench.dump_outputs(FakeFilter(2 << 20, 1, 10 + r), str(tmp_path), r, world)
    out = _load(tmp_path)
    assert _size(tmp_path) <= bench.DUMP_BYTES
    assert "log_ml" in out and all(f"rank{r}_{k}" in out for r in range(world) for k in ("states", "parents", "log_weights", "sample_index"))
