"""The leaf-and-fold integration scheme of csrc/leaf_integrator.hpp on the host (no GPU): csrc/tests/leaf_integrator_selftest.cpp, the host side of a HIP compile
of the same header the spectrum integrator, the cross-spectrum correlator and the integrating beamformer use.  For leaves of 32 and of 64 frames:

  geometry   leaf_geom / leaf_range against a walk over the call's frames, exhaustive over A in {1, 2, LEAF - 1, LEAF, LEAF + 1, 2 LEAF, 2 LEAF + 3}, every
             pos < A and every n in 1 .. 2 A + LEAF + 1: nl, nq, k0, every call-leaf's first / count / complete, and that the ranges tile the call
  fold       streams cut into calls (five seeded sequences per shape, each with a call that ends on a leaf's end and one that ends on an integration's end),
             folded on the CPU with the emit kernel's own body, against the uncut definition -- bit for bit, sum and mean, the carried float64 sum and the
             running leaf after the last call included.  Rows of 6 and of 14 floats, and the Hermitian rule on S = 2 streams of N = 2 bins (P = 3 baselines,
             rows of 2 P N = 12 floats): the diagonal's imaginary parts come out as +0 and nothing else does.

The program exits non-zero at the first mismatch and prints the tuple it belongs to.  It is built a second time with the address and undefined-behaviour
sanitizers (a stand-alone program: nothing is loaded into Python) and has to pass clean there too, where the toolchain links such a build."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "gnuradio4_amd", "csrc", "tests", "leaf_integrator_selftest.cpp")
SANITIZE = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all", "-g"]


def _build(tmp, name, extra):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    exe = tmp / name
    r = subprocess.run([hipcc, "-x", "hip", "--cuda-host-only", "-std=c++17", "-O2", *extra, SRC, "-o", str(exe)], capture_output=True, text=True)
    return exe, r


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True, timeout=300)
    print(r.stdout + r.stderr)
    assert r.returncode == 0, r.stdout + r.stderr
    lines = r.stdout.splitlines()
    for leaf in (32, 64):
        assert any(l.startswith(f"geometry LEAF={leaf}:") and l.endswith("calls ok") for l in lines), r.stdout
        assert f"fold LEAF={leaf}: 150 cut streams ok" in lines, r.stdout  # 3 row shapes x 5 lengths x sum / mean x 5 sequences


def test_geometry_and_fold(tmp_path):
    exe, r = _build(tmp_path, "leaf_integrator_selftest", [])
    assert r.returncode == 0, r.stderr
    _run(exe)


def test_geometry_and_fold_sanitized(tmp_path):
    exe, r = _build(tmp_path, "leaf_integrator_selftest_san", SANITIZE)
    if r.returncode != 0:
        pytest.skip("this toolchain does not link an address / undefined-behaviour sanitizer build of a host program:\n" + r.stderr[-600:])
    _run(exe)
