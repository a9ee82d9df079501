"""The register-level butterflies of csrc/fft_radix.hpp on the host (no GPU): csrc/tests/fft_radix_selftest.cpp, the host side of a HIP compile of the same header
the kernels use, runs both families the header keeps -- fft16 / fft16_tw (the plain second step: the FFT block's kernels) and fft16_fold / fft16_tw_fold (round 8: the
internal W_16 twiddles folded into the second-step butterflies, B = 2 u - A: one more rounding of eps |A|; the fused chain) -- against a float64 DFT-16, on the same
inputs: a unit impulse in every slot, then 64 seeded noise vectors, unit-modulus twiddles of random phase.  Errors are relative to the largest output magnitude.

The bars: BEFORE holds what fft16 / fft16_tw measured on these inputs before round 8 (profiles/r08_headline_trim.txt section 4, with the folded family's figures
beside them); the project's rule for such a fold (round 7) allows three times the figure before it.  The plain family is the code of before: it reads BEFORE itself."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gnuradio4_amd", "csrc", "tests", "fft_radix_selftest.cpp")

BEFORE = {
    "fft16_impulses": 2.898351e-08, "fft16_noise": 1.378817e-07,
    "fft16_tw_impulses": 6.548626e-08, "fft16_tw_noise": 1.224589e-07,
}


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp_path_factory.mktemp("fft_radix") / "fft_radix_selftest"
    subprocess.check_call([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", SRC, "-o", str(exe)])
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout + r.stderr
    print(r.stdout)
    return {k: float(v) for k, v in (line.split() for line in r.stdout.splitlines())}


@pytest.mark.parametrize("family", ["fft16", "fft16_fold"])
@pytest.mark.parametrize("name", sorted(BEFORE))
def test_butterflies_against_float64(figures, name, family):
    got = figures[name.replace("fft16", family, 1)]
    print(f"{family} {name}: {got:.3e} (before the fold {BEFORE[name]:.3e})")
    assert got <= 3.0 * BEFORE[name]


def test_every_check_ran(figures):
    assert set(figures) == {n.replace("fft16", f, 1) for n in BEFORE for f in ("fft16", "fft16_fold")}
