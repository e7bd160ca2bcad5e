"""wv_search_batch_ids refuses bad arguments before it touches a device (no GPU needed)."""
import ctypes as C

import numpy as np

import weaviate_amd as W


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _call(ix=None, nq=1, k=5, off=True):
    q = np.zeros((1, 4), np.float32)
    ids = np.array([1, 2], np.uint64)
    offs = np.array([0, 2], np.uint64)
    oi, od, on = np.zeros(8, np.uint64), np.zeros(8, np.float32), np.zeros(1, np.int32)
    rc = W.lib().wv_search_batch_ids(ix, _vp(q), nq, k, 0, _vp(ids), _vp(offs) if off else None, 0, _vp(oi), _vp(od),
                                     _vp(on))
    return rc, W.lib().wv_last_error().decode()


def test_null_index_is_refused():
    rc, msg = _call()
    assert rc == 1 and "null index" in msg


def test_null_offsets_are_refused():
    rc, msg = _call(off=False)
    assert rc == 1 and "allow_offsets" in msg


def test_negative_batch_is_refused():
    rc, msg = _call(nq=-1)
    assert rc == 1 and "nq" in msg


def test_nonpositive_k_is_refused():
    for k in (0, -3):
        rc, msg = _call(k=k)
        assert rc == 1 and "k <= 0" in msg


def test_stats_need_an_index():
    a = C.c_uint64()
    assert W.lib().wv_last_sparse_stats(None, C.byref(a), None, None) == 1
