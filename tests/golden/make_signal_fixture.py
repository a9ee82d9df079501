"""Generates tests/golden/signal_generator_reference.npz from oracle/_ref/libgr4ref.so, i.e. from the REFERENCE'S OWN SignalGeneratorCore<T>
(algorithm/.../signal/{Tone,Noise,SignalGeneratorCore}.hpp and the rng headers, compiled by oracle/Makefile where the reference tree is present).
For each of float / double / int16 / complex<float> and each of the eleven signal types, 200 000 samples at the parameters of
tests/test_host_cpp.py::test_signal_generator_is_the_reference_core: the SHA-256 of the whole output and the values at `index` (the first
256 samples, the 256 around the phasor renormalisation at 65 536, 512 spread over the rest).  The fixture is data; this script is its provenance."""
import ctypes as C
import hashlib
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import oracle_lib as O  # noqa: E402

N = 200_000
CASES = {"f32": (np.float32, 1.5, 0.25), "f64": (np.float64, 1.5, 0.25), "i16": (np.int16, 30000.0, 9000.0), "c32": (np.complex64, 1.5, 0.25)}

O.build()
R = C.CDLL(os.path.join(O.ORACLE_DIR, "_ref", "libgr4ref.so"))
idx = np.unique(np.r_[np.arange(256), np.arange(65536 - 128, 65536 + 128), np.linspace(0, N - 1, 512).astype(np.int64)])
out = {"index": idx}
for tname, (dt, amp, off) in CASES.items():
    fn = getattr(R, f"gr4ref_signal_{tname}")
    fn.argtypes = [C.c_int, C.c_float, C.c_float, C.c_float, C.c_float, C.c_float, C.c_uint64, C.c_void_p, C.c_size_t]
    fn.restype = None
    for t in range(11):
        want = np.empty(N, dt)
        fn(t, 37.5, 1000.0, 0.3, amp, off, 12345, want.ctypes.data, N)
        out[f"{tname}_{t}"] = want[idx]
        out[f"{tname}_{t}_sha256"] = np.array(hashlib.sha256(want.tobytes()).hexdigest())
np.savez_compressed(os.path.join(os.path.dirname(__file__), "signal_generator_reference.npz"), **out)
print("wrote signal_generator_reference.npz")
