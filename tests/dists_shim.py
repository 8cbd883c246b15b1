"""The host side of the count and positive-real distributions: tests/host/dists_shim.cpp (modppl_amd/csrc/mp_dists.h and
mp_math.h's mp_lgamma / mp_log1p) compiled with g++ and the CPU checker's flags, loaded with ctypes.  Its one entry takes the
arguments of the device probe mp_probe_dist (include/modppl_hip_probe.h), so host and device results can be compared bit for bit."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "host", "dists_shim.cpp")
# oracle/Makefile's CXXFLAGS: the arithmetic the device code is held to
FLAGS = ["-O2", "-std=c++17", "-fPIC", "-ffp-contract=off", "-mfma", "-mavx2", "-Wall", "-Wextra", "-Wno-unused-parameter",
         "-Wno-unknown-pragmas", "-shared"]

POISSON, GAMMA, BETA, GEOMETRIC, UNIFORM_DISCRETE, LGAMMA, LOG1P = range(7)   # = enum mp_probe_dist_kind
EXP = 7   # (the shim only: mp_exp)

_lib = None


def build():
    """-> (path of the shared object, g++'s diagnostics)"""
    out = os.path.join(tempfile.mkdtemp(prefix="mp_dists_shim_"), "dists_shim.so")
    res = subprocess.run(["g++"] + FLAGS + [SRC, "-o", out], capture_output=True, text=True)
    if res.returncode != 0:
        raise RuntimeError("g++ failed on the distributions shim:\n" + res.stderr[-4000:])
    return out, res.stderr


def load():
    global _lib
    if _lib is None:
        so, _ = build()
        L = C.CDLL(so)
        dp = C.POINTER(C.c_double)
        L.mp_shim_dist.argtypes = [C.c_int32, C.c_int32, dp, dp, dp, C.c_int64, C.c_uint64, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32, dp]
        L.mp_shim_dist.restype = C.c_int32
        _lib = L
    return _lib


def _arr(a, n):
    return None if a is None else np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), (n,)))


def _ptr(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_double))


def args(op, x, p0, p1, n):
    """the arrays both entries take: x (op 0), p0, p1 broadcast to n"""
    return (_arr(x, n) if op == 0 else None), _arr(p0, n), _arr(p1, n)


def logpdf(dist, x, p0=None, p1=None):
    x = np.atleast_1d(np.asarray(x, dtype=np.float64))
    n = x.size
    xa, a, b = args(0, x, p0, p1, n)
    out = np.empty(n)
    rc = load().mp_shim_dist(dist, 0, _ptr(xa), _ptr(a), _ptr(b), n, 0, 0, 0, 0, 0, _ptr(out))
    assert rc == 0
    return out


def lgamma(x):
    return logpdf(LGAMMA, x)


def log1p(x):
    return logpdf(LOG1P, x)


def exp(x):
    return logpdf(EXP, x)


def sample(dist, n, p0=None, p1=None, seed=1, slot0=0, step=0, domain=0, site=0):
    _, a, b = args(1, None, p0, p1, n)
    out = np.empty(n)
    rc = load().mp_shim_dist(dist, 1, None, _ptr(a), _ptr(b), n, seed, slot0, step, domain, site, _ptr(out))
    assert rc == 0
    return out
