"""wv_search_by_vector_distance_batch_ids refuses bad arguments before it touches a device (no GPU needed)."""
import ctypes as C

import numpy as np

import weaviate_amd as W


def _vp(a):
    return C.c_void_p(a.ctypes.data)


def _call(ix=None, nq=1, out_cap=8, off=True):
    q = np.zeros((1, 4), np.float32)
    t = np.zeros(1, np.float32)
    ids = np.array([1, 2], np.uint64)
    offs = np.array([0, 2], np.uint64)
    oi, od, on = np.zeros(8, np.uint64), np.zeros(8, np.float32), np.zeros(1, np.int64)
    rc = W.lib().wv_search_by_vector_distance_batch_ids(ix, _vp(q), nq, _vp(t), -1, _vp(ids),
                                                        _vp(offs) if off else None, _vp(oi), _vp(od), out_cap,
                                                        _vp(on))
    return rc, W.lib().wv_last_error().decode()


def test_null_index_is_refused():
    rc, msg = _call()
    assert rc == 1 and "wv_search_by_vector_distance_batch_ids" in msg and "null index" in msg


def test_null_offsets_are_refused():
    rc, msg = _call(off=False)
    assert rc == 1 and "allow_offsets" in msg


def test_negative_batch_is_refused():
    rc, msg = _call(nq=-1)
    assert rc == 1 and "nq < 0" in msg


def test_negative_output_capacity_is_refused():
    rc, msg = _call(out_cap=-1)
    assert rc == 1 and "out_cap < 0" in msg


def test_stats_need_an_index():
    a = C.c_uint64()
    assert W.lib().wv_last_sbd_ids_stats(None, C.byref(a), None, None, None) == 1
    assert "wv_last_sbd_ids_stats" in W.lib().wv_last_error().decode()
