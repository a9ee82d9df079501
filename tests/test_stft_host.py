"""The `stride` setting of the C++ host mirror (gr4/core.hpp Block::stride / strideCounter; OVERLAPPED_FFT.md) on the CPU path, through host/tests/test_host_stft.cpp:
VectorSource -> PowerSpectrum{fftSize 64, stride} -> VectorSink against the frames by the definition (tests/stft_oracle.py), the inactive strides against the block
without the setting, a source that delivers 1, 7 and then many samples per call, the partial frame dropped at the end of the stream, the setting through the plugin.
No GPU needed; the device half of the program runs in tests/test_gpu_stft.py."""
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as O
import pfb_oracle as PO
import stft_oracle as SO

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_stft")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")
N = 64
TOL = 1e-5  # the mirror's PowerSpectrum bar (host/tests/test_host_device.cpp): the body is a float32 window and a float64 transform


@pytest.fixture(scope="module")
def host_run(tmp_path_factory):
    assert os.path.exists(BIN) and os.path.exists(PLUGIN), "build() compiles host/tests/test_host_stft.cpp and the plugin"
    prefix = str(tmp_path_factory.mktemp("stft") / "host")
    r = subprocess.run([BIN, "host", PLUGIN, prefix], capture_output=True, text=True, timeout=120)
    print(r.stdout[-3000:], r.stderr[-2000:])
    return r, prefix


def test_host_program_holds(host_run):
    """paced == at once, inactive stride == no setting, the setting's bookkeeping and the plugin parameter are EXPECTs of the program"""
    r, _ = host_run
    assert r.returncode == 0 and "stft host: ok" in r.stdout and "FAIL" not in r.stdout


@pytest.mark.parametrize("S", [32, 67, 1, 64, 0])
def test_cpu_path_gives_the_frames_by_the_definition(host_run, S):
    _, prefix = host_run
    x = np.fromfile(prefix + ".in", np.float32).view(np.complex64)
    assert len(x) == 20 * N + 37
    eff = S or N
    t = np.abs(SO.spectrum(x, N, eff)) ** 2  # Hann
    got = np.fromfile(f"{prefix}.S{S}.mag2", np.float32).reshape(-1, N)
    assert got.shape == t.shape == (SO.n_frames_total(len(x), N, eff), N)  # the partial frame at the end of the stream is dropped
    e = PO.rel(got, t)
    print(f"stride {S}: host path |X|^2 {e:.2e}")
    assert e <= TOL
