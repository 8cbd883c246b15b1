"""GPU: the count and positive-real distributions of modppl_amd/csrc/mp_dists.h (and mp_lgamma / mp_log1p) evaluated on the device by
the probe mp_probe_dist equal the host shim (tests/host/dists_shim.cpp, the CPU checker's compiler flags) BIT FOR BIT: log-densities
over arrays, and samples drawn from the same Philox coordinates — every rejection attempt takes the same blocks on both sides."""
import ctypes as C

import numpy as np
import pytest

from tests import dists_shim as S

pytestmark = pytest.mark.gpu
N = 200_000


def probe(dist, op, x, p0, p1, n, seed=0, slot0=0, step=0, domain=0, site=0):
    from modppl_amd import capi

    L = capi.load()
    xa, a, b = S.args(op, x, p0, p1, n)
    out = np.empty(n)
    capi.check(L.mp_probe_dist(dist, op, S._ptr(xa), S._ptr(a), S._ptr(b), n, seed, slot0, step, domain, site, S._ptr(out), 0))
    return out


def same_bits(a, b):
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def _params(dist, rng, n):
    """parameter arrays spanning each sampler's regimes"""
    if dist == S.POISSON:
        return np.concatenate([rng.uniform(0., 10., n // 2), 10. * np.exp(rng.uniform(0., np.log(1e5), n - n // 2))]), None
    if dist == S.GAMMA:
        return np.exp(rng.uniform(np.log(0.05), np.log(200.), n)), np.exp(rng.uniform(-3., 3., n))
    if dist == S.BETA:
        return np.exp(rng.uniform(np.log(0.1), np.log(20.), n)), np.exp(rng.uniform(np.log(0.1), np.log(20.), n))
    if dist == S.GEOMETRIC:
        return np.exp(rng.uniform(np.log(1e-4), np.log(0.98), n)), None
    lo = np.floor(rng.uniform(-1000., 1000., n))
    return lo, lo + np.floor(rng.uniform(0., 5000., n))


def _values(dist, rng, n, a, b):
    if dist in (S.POISSON, S.GEOMETRIC):
        return np.concatenate([np.floor(rng.uniform(0., 200., n - 1000)), np.floor(np.exp(rng.uniform(0., np.log(1e6), 990))),
                               [-1., 0.5, 0., np.inf, np.nan, -0., 1e6, 2., 3., 1.]])
    if dist == S.GAMMA:
        return np.concatenate([np.exp(rng.uniform(-20., 8., n - 4)), [0., -1., np.inf, np.nan]])
    if dist == S.BETA:
        return np.concatenate([rng.uniform(0., 1., n - 6), [0., 1., 1e-300, 1. - 2. ** -53, -0.5, np.nan]])
    return np.floor(rng.uniform(-2000., 7000., n))


@pytest.mark.parametrize("dist", [S.POISSON, S.GAMMA, S.BETA, S.GEOMETRIC, S.UNIFORM_DISCRETE])
def test_logpdf_bits_device_equal_host(dist):
    rng = np.random.default_rng(100 + dist)
    a, b = _params(dist, rng, N)
    x = _values(dist, rng, N, a, b)
    dev = probe(dist, 0, x, a, b, N)
    host = S.logpdf(dist, x, a, b)
    assert same_bits(dev, host)


def test_special_functions_bits_device_equal_host():
    rng = np.random.default_rng(7)
    x = np.concatenate([np.exp(rng.uniform(np.log(1e-12), np.log(1e12), N - 8)), [1., 2., 0.5, 3., 8., 0., -1., np.inf]])
    assert same_bits(probe(S.LGAMMA, 0, x, None, None, x.size), S.lgamma(x))
    y = np.concatenate([rng.uniform(-1., 2., N // 2), np.exp(rng.uniform(-700., 700., N - N // 2 - 4)), [-1., -2., 0., np.inf]])
    assert same_bits(probe(S.LOG1P, 0, y, None, None, y.size), S.log1p(y))


@pytest.mark.parametrize("dist", [S.POISSON, S.GAMMA, S.BETA, S.GEOMETRIC, S.UNIFORM_DISCRETE])
def test_sample_bits_device_equal_host(dist):
    rng = np.random.default_rng(200 + dist)
    a, b = _params(dist, rng, N)
    seed, slot0, step, domain, site = 0x1234_5678_9abc, 17, 5, 0, 3 + dist
    dev = probe(dist, 1, None, a, b, N, seed, slot0, step, domain, site)
    host = S.sample(dist, N, a, b, seed=seed, slot0=slot0, step=step, domain=domain, site=site)
    assert same_bits(dev, host)
    assert np.isfinite(dev).all()


def test_small_shape_beta_and_gamma_sample_bits_device_equal_host():
    """shapes down to 10^-3, where both gammas of a beta underflow and the sampler takes its log form: device == host, bit for bit"""
    rng = np.random.default_rng(300)
    a = np.exp(rng.uniform(np.log(1e-3), np.log(0.1), N))
    b = np.where(rng.uniform(size=N) < 0.5, a, np.exp(rng.uniform(np.log(1e-3), np.log(20.), N)))
    dev = probe(S.BETA, 1, None, a, b, N, 99, 0, 2, 0, 7)
    host = S.sample(S.BETA, N, a, b, seed=99, step=2, site=7)
    assert same_bits(dev, host)
    assert np.isfinite(dev).all() and dev.min() >= 2. ** -1022 and dev.max() <= 1. - 2. ** -53
    assert (dev == 2. ** -1022).any() and (dev == 1. - 2. ** -53).any()   # the clamps are reached on both sides
    dev = probe(S.GAMMA, 1, None, a, 1., N, 99, 0, 3, 0, 7)
    assert same_bits(dev, S.sample(S.GAMMA, N, a, 1., seed=99, step=3, site=7))
