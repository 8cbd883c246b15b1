"""The forecast through the C++ host wrapper (modppl_amd/cpp/modppl.hpp): CPU — tests/cpp/forecast.cpp compiles and links against
libmodppl_hip.so; GPU — its forecast(3) and forecast_paths(3, 5, 2) are the Python mirror's values (same C ABI underneath)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "forecast.cpp")
CSRC = os.path.join(ROOT, "modppl_amd", "csrc")


def build_exe(tmp_path):
    from modppl_amd import build as b

    b.build(force=False)
    exe = str(tmp_path / "forecast")
    cmd = ["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", SRC, "-o", exe, "-L" + CSRC, "-lmodppl_hip", "-Wl,-rpath," + CSRC,
           "-Wl,--allow-shlib-undefined"]
    res = subprocess.run(cmd, capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-3000:]
    assert "warning" not in res.stderr, res.stderr[-3000:]
    return exe


def test_cpp_forecast_compiles_and_links(tmp_path):
    build_exe(tmp_path)


@pytest.mark.gpu
def test_cpp_forecast_gives_the_python_values(tmp_path):
    import modppl_amd

    exe = build_exe(tmp_path)
    n, seed = 4096, 7
    res = subprocess.run([exe, str(n), str(seed)], capture_output=True, text=True, env=dict(os.environ), timeout=300)
    assert res.returncode == 0, res.stdout + res.stderr
    pf = modppl_amd.ParticleSystem(modppl_amd.lgssm_model(0.0, 1.0, 0.9, 0.5, 1.0), n, seed)
    pf.init_step(None, [0.31])
    pf.resample()
    pf.step([-0.12])
    sm, sv, om, ov = pf.forecast(3)
    xs, ys = pf.forecast_paths(3, 5, 2)
    want = "mean2=%.17g var2=%.17g omean2=%.17g ovar2=%.17g x=%.17g y=%.17g sizes=6,0,0,0 same=1" % (
        sm[2, 0], sv[2, 0], om[2, 0], ov[2, 0], xs.ravel()[5], ys.ravel()[5])
    lines = [l for l in res.stdout.strip().splitlines() if l.startswith("mean2=")]
    assert lines == [want], (res.stdout, want)
