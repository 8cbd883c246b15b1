"""CPU: the host side's ownership rule (csrc/mp_hip_own.h) as a source check — handles and one-shot entry
points hold holders, so nothing outside that header calls a HIP release function."""
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "modppl_amd", "csrc")
RELEASE_CALLS = ("hipFree(", "hipHostFree(", "hipEventDestroy(", "hipStreamDestroy(")


def test_only_the_holders_release_hip_resources():
    sources = sorted(f for f in os.listdir(CSRC) if f.endswith((".hip", ".h")))
    assert "mp_hip_own.h" in sources and len(sources) > 10, sources
    found = {}
    for f in sources:
        txt = open(os.path.join(CSRC, f), errors="ignore").read()
        for tok in RELEASE_CALLS:
            if tok in txt:
                found.setdefault(tok, []).append(f)
    # every one of them is there (a holder that released nothing would pass an "elsewhere" check too) and nowhere else
    assert found == {tok: ["mp_hip_own.h"] for tok in RELEASE_CALLS}, found
