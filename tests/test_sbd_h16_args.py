"""wv_index_set_sbd_key_pass / wv_last_sbd_key_pass_stats: present in the ABI and the binding, refuse a null index (no GPU needed)."""
import ctypes as C

import pytest

import weaviate_amd as W


def test_symbols_exist():
    for name in ("wv_index_set_sbd_key_pass", "wv_last_sbd_key_pass_stats"):
        assert hasattr(W.lib(), name) and name in W.header_symbols()
    assert hasattr(W.GPUVectorIndex, "set_sbd_key_pass") and hasattr(W.GPUVectorIndex, "last_sbd_key_pass_stats")


@pytest.mark.parametrize("on", [0, 1])
def test_switch_needs_an_index(on):
    assert W.lib().wv_index_set_sbd_key_pass(None, on) == 1
    assert "wv_index_set_sbd_key_pass" in W.lib().wv_last_error().decode()


def test_stats_need_an_index():
    a = C.c_uint64()
    assert W.lib().wv_last_sbd_key_pass_stats(None, C.byref(a), None, None) == 1
    assert "wv_last_sbd_key_pass_stats" in W.lib().wv_last_error().decode()
