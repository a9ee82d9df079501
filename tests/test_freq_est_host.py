"""The frequency estimators in the C++ host layer (gnuradio4_amd/host): the plugin's four registered names, the decimating forms' chunks, the loud failure of
the device blocks without a GPU, and, on a GPU, source -> fir_filter -> FrequencyEstimatorFrequencyDomainDecimating -> sink and the per-sample time-domain block
on compute_domain gpu:hip:0 against the oracle (tests/freq_est_oracle.py)."""
import os
import subprocess

import numpy as np
import pytest

import freq_est_oracle as FE
import oracle_lib as O

ROOT = O.ROOT
BIN = os.path.join(ROOT, "build", "host", "test_host_freq_est")
PLUGIN = os.path.join(ROOT, "gnuradio4_amd", "libgr4hip_blocks.so")


@pytest.fixture(scope="module")
def prog():
    subprocess.check_call(["bash", os.path.join(ROOT, "gnuradio4_amd", "host", "build.sh")], stdout=subprocess.DEVNULL)
    return BIN


def test_plugin_makes_the_four_names(prog):
    r = subprocess.run([prog, PLUGIN, "host"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed (compute_domain host)" in r.stdout


def test_device_blocks_fail_loudly_without_gpu(prog, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    sig = tmp_path / "x.f32"
    FE.tone(50.3, 1000.0, 8192).tofile(sig)
    for domain in ("gpu:hip:0", "host"):  # off-device the blocks have no host arithmetic: the graph fails, it does not produce numbers
        r = subprocess.run([prog, PLUGIN, domain, str(sig), str(tmp_path / "y")], capture_output=True, text=True, timeout=300)
        assert r.returncode == 3, (domain, r.returncode, r.stdout, r.stderr)


@pytest.mark.gpu
def test_device_graph_matches_the_oracle(prog, tmp_path):
    n = 4096 * 24
    x = FE.tone(50.37, 1000.0, n, noise=0.01, seed=4)
    sig = tmp_path / "x.f32"
    x.tofile(sig)
    r = subprocess.run([prog, PLUGIN, "gpu:hip:0", str(sig), str(tmp_path / "y")], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout + r.stderr
    fd = np.fromfile(tmp_path / "y_fd.f32", np.float32).astype(np.float64)
    td = np.fromfile(tmp_path / "y_td.f32", np.float32).astype(np.float64)
    # fir_filter {0.5, 0.5} in float64, then the decimating frequency-domain estimator (chunk N = 4096)
    xf = O.fir(np.array([0.5, 0.5]), x)[0]
    pf = FE.Params(1, f_min=45.0, f_max=55.0, min_fft_size=4096, chunk=4096)
    want_fd, _, valid, m = FE.fd_truth(pf, xf)
    assert len(fd) == n // 4096 and valid[1:].all() and m["top2"] > 1e-4
    assert np.max(FE.rel_err(fd, want_fd)) <= 1e-5
    pt = FE.Params(0, f_min=45.0, f_max=55.0, n_periods=3, chunk=1)
    want_td, _, valid, m = FE.td_truth(pt, x)
    assert len(td) == n and valid[-1]
    assert np.max(FE.rel_err(td, want_td)) <= 1e-5
