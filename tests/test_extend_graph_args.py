"""wv_index_extend_graph refuses bad arguments before it touches a device (no GPU needed)."""
import ctypes as C
import os
import re

import weaviate_amd as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _ef_max():
    src = open(os.path.join(ROOT, "weaviate_amd", "csrc", "wv_params.h")).read()
    return int(re.search(r"constexpr int HNSW_EF_MAX = (\d+);", src).group(1))


def _call(ix=None, efc=32, seed=1, div=32, inserted=True):
    k = C.c_uint64(77)
    rc = W.lib().wv_index_extend_graph(ix, efc, seed, div, C.byref(k) if inserted else None)
    return rc, W.lib().wv_last_error().decode(), k.value


def test_symbol_is_declared_and_bound():
    assert "wv_index_extend_graph" in W.header_symbols()
    assert hasattr(W.GPUVectorIndex, "extend_graph")


def test_null_index_is_refused():
    rc, msg, k = _call()
    assert rc == 1 and "null index" in msg and k == 0


def test_ef_construction_out_of_range_is_refused():
    for efc in (0, -1, _ef_max() + 1):
        rc, msg, _ = _call(efc=efc)
        assert rc == 1 and "ef_construction" in msg
    rc, msg, _ = _call(efc=_ef_max())   # the largest legal value passes this check
    assert rc == 1 and "null index" in msg


def test_batch_div_below_one_is_refused():
    for div in (0, -5):
        rc, msg, _ = _call(div=div)
        assert rc == 1 and "batch_div" in msg


def test_null_inserted_is_accepted_by_the_prototype():
    rc, msg, _ = _call(inserted=False)
    assert rc == 1 and "null index" in msg   # (refused for the index, not for the null counter)
