"""no GPU: the plans of tests/test_gpu_fir_interp_paths.py are what they say they are -- the kernel each call states is the one the dispatch rule picks, the records
they assert cover every kernel, G, R, segments per workgroup and both ways of writing the next history, the limits table states ip_upload's (KS, G), and the numpy
polyphase truth is the zero-stuffing oracle.  The test hook is exported and declared nowhere."""
import os
import re

import pytest

pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fir_interp_plans():
    import test_gpu_fir_interp_paths as T
    T.test_plans_reach_every_path_and_state_the_dispatch_rule()
    T.test_limits_table_states_the_form()
    for plan in T._all_plans():  # no span beyond about 1e5 inputs: the tests stay quick
        assert all(n <= 110_000 for n, _, _, _, _ in T._walk(plan)), plan["id"]


@pytest.mark.parametrize("L,K,n,cplx", [(2, 33, 3000, False), (7, 50, 2000, True), (16, 5, 1000, False)])
def test_fir_interp_truth_is_the_oracle(L, K, n, cplx):
    import test_gpu_fir_interp_paths as T
    T.test_polyphase_truth_is_the_zero_stuffing_oracle(L, K, n, cplx)


def test_fir_interp_hook_is_exported_and_not_declared():
    from gnuradio4_amd import capi
    import ctypes
    raw = ctypes.CDLL(capi.LIB_PATH)
    text = open(os.path.join(ROOT, "include", "gr4hip.h")).read()
    assert hasattr(raw, "gr4hip_internal_fir_interp_last_path") and not re.search(r"\bgr4hip_internal_fir_interp_last_path\b", text)
    assert "gr4hip_internal_fir_interp_last_path" not in capi.SIGNATURES
