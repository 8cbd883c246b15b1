"""The quantiles through the C++ host wrapper (modppl_amd/cpp/modppl.hpp): CPU — tests/cpp/quantiles.cpp compiles and links against
libmodppl_hip.so; GPU — its quantiles(qs), path_quantiles(qs) and site_quantiles(qs) are the Python mirror's values, bit for bit (same
C ABI underneath)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "quantiles.cpp")
CSRC = os.path.join(ROOT, "modppl_amd", "csrc")


def build_exe(tmp_path):
    from modppl_amd import build as b

    b.build(force=False)
    exe = str(tmp_path / "quantiles")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", exe, "-L" + CSRC, "-lmodppl_hip", "-Wl,-rpath," + CSRC,
           "-Wl,--allow-shlib-undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "warning" not in res.stderr, res.stderr[-3000:]
    return exe


def test_cpp_quantiles_compiles_and_links(tmp_path):
    build_exe(tmp_path)


def bits(a):
    return " ".join("%016x" % b for b in np.ascontiguousarray(a, dtype=np.float64).view(np.uint64).ravel().tolist())


@pytest.mark.gpu
def test_cpp_quantiles_give_the_python_bits(tmp_path):
    import modppl_amd
    from modppl_amd import capi

    exe = build_exe(tmp_path)
    n, seed, qs = 4096, 7, [0.5, 0.05, 0.95]
    res = subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True, env=dict(os.environ), timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(0.0, 1.0, 0.9, 0.5, 1.0), n, seed, flags=capi.MP_PF_RECORD_HISTORY)
    pf.init_step(None, [0.31])
    pf.resample()
    pf.step([-0.12])
    xs = [-1.0 + 0.5 * k for k in range(4)]
    cons = {capi.MP_SITE_Y0 + k: 0.25 * k - 0.1 for k in range(4)}
    fc = modppl_amd.FunctionChains(capi.MP_MH_MODEL_HIERARCHICAL_FN, xs, cons, n, seed)
    count, sites = fc.site_quantiles(qs)
    want = ["cloud " + bits(pf.quantiles(qs)), "path " + bits(pf.path_quantiles(qs)), "count " + " ".join(str(int(c)) for c in count),
            "sites " + bits(sites)]
    assert res.stdout.strip().splitlines() == want, (res.stdout, want)
    assert 0 < count[capi.MP_SITE_C] < n and np.isfinite(sites[:, capi.MP_SITE_C]).all()
