"""wv_last_sbd_stats: present in the ABI, refuses a null index, takes null outputs (no GPU needed)."""
import ctypes as C

import weaviate_amd as W


def test_stats_function_exists():
    assert hasattr(W.lib(), "wv_last_sbd_stats")
    assert hasattr(W.GPUVectorIndex, "last_sbd_stats")


def test_stats_need_an_index():
    a, b, c = C.c_uint64(7), C.c_uint64(7), C.c_uint64(7)
    assert W.lib().wv_last_sbd_stats(None, C.byref(a), C.byref(b), C.byref(c)) == 1
    assert "wv_last_sbd_stats" in W.lib().wv_last_error().decode()
    assert (a.value, b.value, c.value) == (7, 7, 7)


def test_null_outputs_with_a_null_index():
    assert W.lib().wv_last_sbd_stats(None, None, None, None) == 1
    assert "null index" in W.lib().wv_last_error().decode()
