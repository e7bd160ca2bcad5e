"""Exact search past every key pass on the batched large-k route (-m gpu).

set_large_k(True) answers k > 256 (k > 32 with per-query bitmaps) by a sampled
bound per query, the distance search's threshold pass, a segmented sort and an
emit kernel (wv_bigk.hip) instead of a scan and sort per query.  The answers
must equal the CPU restatement's flatSearch -- distances bit for bit, ids up to
the reference's heap order among equal distances -- and last_large_k_stats()
must show which route answered.
"""
import functools

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from helpers import same_tie_aware

pytestmark = pytest.mark.gpu

NAMES = {O.L2: "l2-squared", O.DOT: "dot", O.COSINE: "cosine-dot"}
N, D, NQ, KMAX = 20_000, 20, 24, 4096


@functools.lru_cache(maxsize=None)
def _case(metric):
    """(index with 2 % tombstones and the route on, queries, allow lists by
    name, the restatement's KMAX nearest per list); one draw for all metrics."""
    rng = np.random.default_rng(7)
    base = rng.standard_normal((N, D)).astype(np.float32)
    qs = rng.standard_normal((NQ, D)).astype(np.float32)
    dead = rng.choice(N, N // 50, replace=False)
    masks = {"none": np.ones(N, bool), "shared": rng.random(N) < 0.3, "per_query": rng.random((NQ, N)) < 0.5,
             "few": np.arange(N) % 40 == 0}
    ix = W.GPUVectorIndex(D, NAMES[metric], capacity=N)
    ix.upload_vectors(base)
    ix.add_tombstones(dead)
    ix.set_large_k(True)
    b, q = (O.normalize_rows(base), O.normalize_rows(qs)) if metric == O.COSINE else (base, qs)
    alive = np.ones(N, bool)
    alive[dead] = False
    allow, ref = {}, {}
    for name, m in masks.items():
        rows = m if m.ndim == 2 else [m]
        allow[name] = [W.AllowList.from_ids(np.nonzero(r)[0], N) for r in rows]
        parts = [O.flat_scan(metric, b, q[i:i + 1] if m.ndim == 2 else q, KMAX,
                             allow_bits=O.bits_from_ids(np.nonzero(r & alive)[0], N)) for i, r in enumerate(rows)]
        ref[name] = tuple(np.concatenate(x) for x in zip(*parts))
        if m.ndim == 1:
            allow[name] = None if name == "none" else allow[name][0]
    return ix, qs, allow, ref


def _check(metric, k, name, stats, nq=NQ):
    ix, qs, allow, ref = _case(metric)
    ids, ds, n = ix.search_batch(qs[:nq], k, mode="exact", allow=allow[name])
    assert ix.last_large_k_stats() == stats
    oi, od, on = ref[name]
    assert n.tolist() == np.minimum(on[:nq], k).tolist()
    for i in range(nq):
        same_tie_aware(ids[i, :n[i]], ds[i, :n[i]], oi[i, :n[i]], od[i, :n[i]])


@pytest.mark.parametrize("name", ["none", "shared", "per_query"])
@pytest.mark.parametrize("k", [257, 1000, 4096])
@pytest.mark.parametrize("metric", [O.L2, O.DOT, O.COSINE])
def test_large_k_equals_restatement(metric, k, name):
    _check(metric, k, name, (NQ, 0))


def test_per_query_bitmaps_take_the_route_from_k_33():
    _check(O.L2, 40, "per_query", (NQ, 0))


@pytest.mark.parametrize("nq,k,taken", [(1, 600, True), (1, 601, False), (3, 2000, True), (3, 2001, False), (4, 4096, True)])
def test_smallest_batches_take_the_route_only_where_it_is_faster(nq, k, taken):
    _check(O.L2, k, "none", (nq, 0) if taken else (0, 0), nq)


def test_short_allow_list_lists_every_eligible_row():
    """500 allowed rows, k = 1000: the sample holds under 36 of them, tau is
    +inf and out_n is the eligible count."""
    _check(O.DOT, 1000, "few", (NQ, 0))


@pytest.mark.parametrize("name", ["none", "per_query"])
def test_f16_filter_as_the_threshold_pass(name):
    ix = _case(O.L2)[0]
    ix.set_sbd_key_pass(True)
    try:
        _check(O.L2, 1000, name, (NQ, 0))
    finally:
        ix.set_sbd_key_pass(False)


def test_overflowing_lists_fall_back(monkeypatch):
    monkeypatch.setenv("WV_SBD_CAP", "128")
    _check(O.L2, 257, "none", (0, NQ))


def test_three_chunks(monkeypatch):
    monkeypatch.setenv("WV_BIGK_MAX_ENTRIES", str(8 * 16384))
    _check(O.COSINE, 1000, "shared", (NQ, 0))


def test_switch_off_is_the_per_query_route():
    ix = _case(O.L2)[0]
    ix.set_large_k(False)
    try:
        _check(O.L2, 257, "none", (0, 0))
    finally:
        ix.set_large_k(True)


def test_fewer_rows_than_k():
    base = np.random.default_rng(1).standard_normal((300, D)).astype(np.float32)
    ix = W.GPUVectorIndex(D, "l2-squared", capacity=300)
    ix.upload_vectors(base)
    ix.set_large_k(True)
    ids, ds, n = ix.search_batch(base[:5], 1000, mode="exact")
    assert ix.last_large_k_stats() == (5, 0) and n.tolist() == [300] * 5
    oi, od, on = O.flat_scan(O.L2, base, base[:5], 1000)
    for i in range(5):
        same_tie_aware(ids[i, :300], ds[i, :300], oi[i, :300], od[i, :300])
    ix.close()


def test_ties_are_cut_and_ordered_by_id():
    """Integer rows: every fp32 sum is exact and hundreds of rows tie at the
    k-th distance; the reference is the float64 ranking by (dist, id)."""
    rng = np.random.default_rng(3)
    n, d, k = 5000, 8, 300
    base = rng.integers(-2, 3, (n, d)).astype(np.float32)
    qs = rng.integers(-2, 3, (16, d)).astype(np.float32)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    ix.set_large_k(True)
    ids, ds, cnt = ix.search_batch(qs, k, mode="exact")
    assert ix.last_large_k_stats() == (16, 0) and cnt.tolist() == [k] * 16
    for i in range(16):
        full = ((base.astype(np.float64) - qs[i].astype(np.float64)) ** 2).sum(1)
        order = np.lexsort((np.arange(n), full))[:k]
        assert ids[i].tolist() == order.tolist()
        assert np.array_equal(ds[i].view(np.uint32), full[order].astype(np.float32).view(np.uint32))
    ix.close()
