"""wv_index_set_large_k and wv_last_large_k_stats: present in the ABI and the binding, refuse a null index (no GPU needed)."""
import pytest

import weaviate_amd as W

SYMBOLS = {"wv_index_set_large_k": "set_large_k", "wv_last_large_k_stats": "last_large_k_stats"}


@pytest.mark.parametrize("sym", sorted(SYMBOLS))
def test_symbols_exist(sym):
    assert hasattr(W.lib(), sym)
    assert hasattr(W.GPUVectorIndex, SYMBOLS[sym])
    assert sym in W.header_symbols()


@pytest.mark.parametrize("sym", sorted(SYMBOLS))
def test_calls_need_an_index(sym):
    args = (None, 1) if sym == "wv_index_set_large_k" else (None, None, None)
    assert getattr(W.lib(), sym)(*args) == 1
    assert sym in W.lib().wv_last_error().decode()
