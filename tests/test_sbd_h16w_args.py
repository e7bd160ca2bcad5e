"""wv_index_set_sbd_wide_key_pass: present in the ABI and the binding, refuses a null index (no GPU needed)."""
import pytest

import weaviate_amd as W
from weaviate_amd import _lib


def test_symbol_exists():
    name = "wv_index_set_sbd_wide_key_pass"
    assert name in _lib.SIGNATURES and hasattr(W.lib(), name) and name in W.header_symbols()
    assert hasattr(W.GPUVectorIndex, "set_sbd_wide_key_pass")


@pytest.mark.parametrize("on", [0, 1])
def test_switch_needs_an_index(on):
    assert W.lib().wv_index_set_sbd_wide_key_pass(None, on) == 1   # WV_EINVAL
    assert "wv_index_set_sbd_wide_key_pass" in W.lib().wv_last_error().decode()
