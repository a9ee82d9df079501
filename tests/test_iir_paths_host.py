"""no GPU: the filters of tests/test_gpu_iir_paths.py's routing table are what the table says they are -- warm-up lengths by the create-time criterion restated in
numpy, every kernel instantiation and warm-up choice named, and the reference's float32 cascade within 3e-6 of float64 wherever a case is held to 1e-5"""
import pytest

pytest.importorskip("torch")


def test_iir_routing_table_filters():
    import test_gpu_iir_paths as T
    T.check_table()
