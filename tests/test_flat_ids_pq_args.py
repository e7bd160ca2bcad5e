"""wv_index_set_pq_list_search: present in the ABI and the binding, refuses a null index (no GPU needed)."""
import weaviate_amd as W


def test_setter_exists():
    assert hasattr(W.lib(), "wv_index_set_pq_list_search")
    assert hasattr(W.GPUVectorIndex, "set_pq_list_search")
    assert "wv_index_set_pq_list_search" in W.header_symbols()


def test_setter_needs_an_index():
    for on in (0, 1):
        assert W.lib().wv_index_set_pq_list_search(None, on) == 1
        assert "wv_index_set_pq_list_search" in W.lib().wv_last_error().decode()
