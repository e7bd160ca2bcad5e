"""The batched large-k route on manhattan, hamming and PQ-compressed indexes
(wv_bigk_kinds.hip; -m gpu).

The yardstick is never the new code.  Manhattan and hamming: the numpy float32
chain in dimension order, float64 as a bound, ranked by (dist, id)
(test_gpu_l1).  Compressed: the CPU restatement's PQ distance of every live
allowed row in (dist, id) order (test_gpu_flat_ids_pq).  Bar: ids, distance
bits and counts identical, and last_large_k_stats() shows the route answered.

Every (nq, 0) here is a property of the data: from the reference distances
alone, each query's tau (the 36th smallest over the eligible rows
j max(1, k // 16)) leaves at least k and at most 10,971 (manhattan), 13,735
(hamming: integer distances tie at tau, hence values 0..7 x 64 columns) and
2,903 (compressed) eligible rows within it, against lists of 16,384.

Code layouts: d32-m8-ks256's table (8 KiB) is built in LDS; d32-m32-ks1024's
(128 KiB) is past the 64 KiB limit, which forces direct evaluation -- no
environment switch is used.
"""
import functools

import numpy as np
import pytest

import weaviate_amd as W
from test_gpu_flat_ids_pq import _queries, _restated, _same
from test_gpu_l1 import _check_knn, _reference
from test_pq import _compressed_pair

pytestmark = pytest.mark.gpu

N, NP, NQ = 20_000, 6000, 24
L1_D = {"manhattan": 33, "hamming": 64}
LAYOUTS = {"table": (32, 8, 256), "direct": (32, 32, 1024)}
METRICS_PQ = ["l2-squared", "dot", "cosine-dot"]


def _masks(rng, n):
    """[1 or NQ][n] bool per filter; `few`: 2.5 % of the rows, none of them a
    multiple of an even step, so the sample holds no eligible row"""
    return {"none": np.ones((1, n), bool), "shared": (rng.random(n) < 0.3)[None], "perq": rng.random((NQ, n)) < 0.5,
            "few": (np.arange(n) % 40 == 1)[None]}


def _allow(mask, n):
    if mask.all():
        return None
    rows = [W.AllowList.from_ids(np.flatnonzero(r), n) for r in mask]
    return rows if len(rows) > 1 else rows[0]


def l1_data(metric, n=N, d=None):
    """rows, queries, eligible [NQ][n] per filter, allow masks, the reference's chains and float64 sums"""
    d = d or L1_D[metric]
    rng = np.random.default_rng(11)
    if metric == "hamming":
        draw = lambda m: rng.integers(0, 8, (m, d)).astype(np.float32)
    else:
        draw = lambda m: rng.random((m, d), dtype=np.float32) * 2 - 1
    base, qs = draw(n), draw(NQ)
    dead = rng.choice(n, n // 50, replace=False)
    masks = _masks(rng, n)
    alive = np.ones(n, bool)
    alive[dead] = False
    ok = {name: np.broadcast_to(m & alive, (NQ, n)) for name, m in masks.items()}
    return (base, qs, dead, masks, ok) + _reference(metric, base, qs)


@functools.lru_cache(maxsize=None)
def _l1_case(metric, n=N, d=None):
    data = l1_data(metric, n, d)
    ix = W.GPUVectorIndex(data[0].shape[1], metric, capacity=n)
    ix.upload_vectors(data[0])
    ix.add_tombstones(data[2])
    ix.set_large_k(True)
    return (ix,) + data


def _check_l1(metric, k, name, stats, n=N, d=None):
    ix, base, qs, _, masks, ok, s, d64 = _l1_case(metric, n, d)
    got = ix.search_batch(qs, k, mode="exact", allow=_allow(masks[name], n))
    assert ix.last_large_k_stats() == stats
    _check_knn(got, s, d64, ok[name], k, base.shape[1])


@pytest.mark.parametrize("name", ["none", "shared", "perq"])
@pytest.mark.parametrize("k", [129, 257, 1000, 4096])   # 129: the first k past the tiled kernel
@pytest.mark.parametrize("metric", list(L1_D))
def test_l1_equals_the_serial_chain(metric, k, name):
    _check_l1(metric, k, name, (NQ, 0))


def test_l1_query_row_past_1024_columns():
    _check_l1("manhattan", 129, "perq", (NQ, 0), n=3000, d=1030)


def pq_data(metric, layout):
    """the restatement, the index, queries, allow masks and per filter each query's (ids, dists) in (dist, id) order"""
    d, m, ks = LAYOUTS[layout]
    ref, ix, _, _, _ = _compressed_pair(NP, d, m, ks, metric)
    rng = np.random.default_rng(21)
    dead = rng.choice(NP, NP // 50, replace=False)
    for t in dead:
        ref.add_tombstone(int(t))
    ix.add_tombstones(dead)
    qs = _queries(rng, NQ, d, metric)
    masks = {name: m for name, m in _masks(rng, NP).items() if name != "shared"}
    full = {name: _restated(ref, NP, qs, [np.flatnonzero(m[i % len(m)]).astype(np.uint64) for i in range(NQ)])
            for name, m in masks.items()}
    return ref, ix, qs, masks, full


@functools.lru_cache(maxsize=None)
def _pq_case(metric, layout):
    _, ix, qs, masks, full = pq_data(metric, layout)
    ix.set_large_k(True)
    return ix, qs, masks, full


def _check_pq(metric, layout, k, name, stats, fused=False):
    ix, qs, masks, full = _pq_case(metric, layout)
    ix.set_pq_scan(fused)
    ids, ds, n = ix.search_batch(qs, k, mode="exact", allow=_allow(masks[name], NP))
    assert ix.last_large_k_stats() == stats
    if stats[0]:
        assert ix.last_pq_scan_stats() == {"fused_queries": 0, "sorted_queries": stats[1]}
    for i, (wi, wd) in enumerate(full[name]):
        assert n[i] == min(k, len(wi)), i
        _same(ids[i, :n[i]], ds[i, :n[i]], wi[:k], wd[:k])


@pytest.mark.parametrize("fused", [False, True])
@pytest.mark.parametrize("name", ["none", "perq"])
@pytest.mark.parametrize("k", [257, 1000])
@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("metric", METRICS_PQ)
def test_compressed_equals_the_restatement(metric, layout, k, name, fused):
    _check_pq(metric, layout, k, name, (NQ, 0), fused)


@pytest.mark.parametrize("fused,k,stats", [(True, 256, (0, 0)), (True, 257, (NQ, 0)), (False, 32, (0, 0)), (False, 33, (NQ, 0))])
def test_compressed_lower_edge(fused, k, stats):
    """With the fused scan on it keeps k <= 256; with it off the route takes every k past 32."""
    _check_pq("l2-squared", "table", k, "perq", stats, fused)
    if not stats[0]:
        assert _pq_case("l2-squared", "table")[0].last_pq_scan_stats() == {
            "fused_queries": NQ if fused else 0, "sorted_queries": 0 if fused else NQ}


@pytest.mark.parametrize("kind", ["manhattan", "hamming", "dot"])
def test_overflowing_lists_fall_back(monkeypatch, kind):
    monkeypatch.setenv("WV_SBD_CAP", "128")
    _check_pq(kind, "table", 257, "none", (0, NQ)) if kind == "dot" else _check_l1(kind, 257, "none", (0, NQ))


@pytest.mark.parametrize("kind", ["manhattan", "hamming", "cosine-dot"])
def test_short_allow_list_lists_every_eligible_row(kind):
    """k = 1000, step 62: no allowed row is sampled, tau is +inf and out_n is the eligible count (under 500)."""
    _check_pq(kind, "direct", 1000, "few", (NQ, 0)) if kind == "cosine-dot" else _check_l1(kind, 1000, "few", (NQ, 0))


@pytest.mark.parametrize("kind", ["hamming", "l2-squared"])
def test_switch_off_is_the_old_route(kind):
    ix = _pq_case(kind, "table")[0] if kind == "l2-squared" else _l1_case(kind, N, None)[0]   # (the cache's key as _check_l1 spells it)
    ix.set_large_k(False)
    try:
        _check_pq(kind, "table", 257, "none", (0, 0)) if kind == "l2-squared" else _check_l1(kind, 257, "shared", (0, 0))
    finally:
        ix.set_large_k(True)
