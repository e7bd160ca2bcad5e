"""wv_index_cleanup_tombstones refuses bad arguments before it touches a device (no GPU needed)."""
import ctypes as C

import pytest

import weaviate_amd as W

EF_MAX = 512   # HNSW_EF_MAX, as include/wvgpu.h states it for this call


def _call(ix=None, efc=32, div=8, outputs=True):
    r, d, k = C.c_uint64(7), C.c_uint64(8), C.c_uint64(9)
    out = [C.byref(r), C.byref(d), C.byref(k)] if outputs else [None, None, None]
    rc = W.lib().wv_index_cleanup_tombstones(ix, efc, div, *out)
    return rc, W.lib().wv_last_error().decode(), (r.value, d.value, k.value)


def test_symbol_is_declared_and_bound():
    assert "wv_index_cleanup_tombstones" in W.header_symbols()
    assert hasattr(W.GPUVectorIndex, "cleanup_tombstones")


def test_null_index_is_refused_and_the_counts_are_zeroed():
    rc, msg, counts = _call()
    assert rc == 1 and "null index" in msg and counts == (0, 0, 0)


@pytest.mark.parametrize("efc", [0, -1, EF_MAX + 1])
def test_ef_construction_out_of_range_is_refused(efc):
    rc, msg, _ = _call(efc=efc)
    assert rc == 1 and "ef_construction" in msg


def test_largest_ef_construction_passes_the_range_check():
    rc, msg, _ = _call(efc=EF_MAX)
    assert rc == 1 and "null index" in msg


@pytest.mark.parametrize("div", [0, -5])
def test_batch_div_below_one_is_refused(div):
    rc, msg, _ = _call(div=div)
    assert rc == 1 and "batch_div" in msg


def test_null_outputs_are_accepted_by_the_prototype():
    rc, msg, _ = _call(outputs=False)
    assert rc == 1 and "null index" in msg   # (refused for the index, not for the null counters)
