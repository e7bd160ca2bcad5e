"""wv_launch_l1_ids and wv_launch_l1_sbd_ids refuse bad arguments before any launch (no GPU needed).

The structures restate FlatIdsParams and SbdIdsParams of csrc/wv_params.h; every case changes one field of
a set the launchers accept, and none reaches a launch."""
import ctypes as C

import pytest

import weaviate_amd as W

P, U64, I = C.c_void_p, C.c_uint64, C.c_int
INVALID = 1   # hipErrorInvalidValue
PTR = 0x1000  # never read: the checks come first


class FlatIdsParams(C.Structure):
    _fields_ = [("X", P), ("Q", P), ("excl", P), ("excl_nbits", U64), ("ids", P), ("off", P), ("sel", P),
                ("n_rows", U64), ("id_base", U64), ("chunk_len", U64), ("part", P), ("ns", I), ("n_chunks", I),
                ("D", I), ("dpad", I), ("ldx", I), ("metric", I), ("k", I), ("out_ids", P), ("out_d", P), ("out_n", P)]


class SbdIdsParams(C.Structure):
    _fields_ = [("X", P), ("Q", P), ("target", P), ("excl", P), ("excl_nbits", U64), ("ids", P), ("off", P),
                ("seg_beg", P), ("seg_cap", P), ("n_rows", U64), ("chunk_len", U64), ("q0", I), ("nq", I),
                ("n_chunks", I), ("D", I), ("dpad", I), ("ldx", I), ("metric", I), ("keys", P), ("cnt", P),
                ("cand_cnt", P), ("n_elig", P), ("cand_cap", I), ("key_cap", I), ("n_elig_stride", I)]


COMMON = dict(X=PTR, Q=PTR, excl=PTR, excl_nbits=64, ids=PTR, off=PTR, n_rows=64, chunk_len=256, n_chunks=1, D=8,
              dpad=8, ldx=8, metric=3)
KNN = dict(COMMON, sel=PTR, ns=1, k=10, out_ids=PTR, out_d=PTR, out_n=PTR)
SBD = dict(COMMON, target=PTR, seg_beg=PTR, seg_cap=PTR, nq=1, keys=PTR, cnt=PTR)
BAD = [("metric", 0), ("metric", 2), ("metric", 5), ("n_chunks", 0), ("n_chunks", 65536), ("chunk_len", 0),
       ("chunk_len", 100), ("dpad", 8196), ("ldx", 6), ("ldx", 4), ("X", 0), ("ids", 0)]


@pytest.mark.parametrize("field,value", BAD + [("k", 0), ("k", 257), ("n_chunks", 2), ("sel", 0), ("out_n", 0)])
def test_knn_launcher_refuses(field, value):
    p = FlatIdsParams(**dict(KNN, **{field: value}))
    assert W.lib().wv_launch_l1_ids(C.byref(p), None) == INVALID


@pytest.mark.parametrize("field,value", BAD + [("cand_cnt", PTR), ("target", 0), ("seg_cap", 0), ("cnt", 0)])
def test_threshold_launcher_refuses(field, value):
    p = SbdIdsParams(**dict(SBD, **{field: value}))
    assert W.lib().wv_launch_l1_sbd_ids(C.byref(p), None) == INVALID


def test_an_empty_batch_launches_nothing():
    assert W.lib().wv_launch_l1_ids(C.byref(FlatIdsParams(**dict(KNN, ns=0, metric=0))), None) == 0
    assert W.lib().wv_launch_l1_sbd_ids(C.byref(SbdIdsParams(**dict(SBD, nq=0, metric=0))), None) == 0
