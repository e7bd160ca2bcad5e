"""Flat k-NN on a PQ-compressed index by the fused scan (wv_index_set_pq_scan,
wv_pq_scan.hip) against the CPU restatement, and with the setting on against
off.

The yardstick is never the new code.  The restatement is asked, per query, for
the PQ distance of every live row (test_gpu_flat_ids_pq's _restated over the
list of all rows); those a filter allows, in (dist, id) order and cut to k, are
the expected rows.  Bar: ids, distance bits and counts identical, and the stats
say the fused kernel answered every query.  Runs on an MI355X (-m gpu).
"""
import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from test_gpu_flat_ids_pq import LAYOUTS, _queries, _restated, _same, _same_batch
from test_pq import _centroids, _compressed_pair

pytestmark = pytest.mark.gpu

N, NQ = 6000, 9   # whole groups of four or two queries and a group of one
KS_ALL = (1, 10, 64, 65, 256)
LAYOUT_ID = lambda c: "d%d-m%d-ks%d-%s" % (c[0], c[1], c[2], "bits" if c[3] else "bytes")   # noqa: E731


def _filters(rng, n, k):
    """No filter, a shared bitmap of 10 %, per-query bitmaps whose cardinalities
    cross k, a wave step and the 256 keys a wave holds -- as (allow argument,
    per-query membership masks)."""
    shared = rng.random(n) < 0.1
    cards = [0, k - 1, k, k + 1, 63, 64, 65, 257, n // 2]
    each = np.zeros((NQ, n), bool)
    for i, c in enumerate(cards):
        each[i, rng.choice(n, c, replace=False)] = True
    return [("none", None, np.ones((NQ, n), bool)),
            ("shared", W.AllowList.from_ids(np.nonzero(shared)[0], n), np.tile(shared, (NQ, 1))),
            ("each", [W.AllowList.from_ids(np.nonzero(m)[0], n) for m in each], each)]


def _check(ix, n, qs, full, ks=KS_ALL, seed=3):
    """Every k and filter: the batch equals the restatement's rows, all fused."""
    rng = np.random.default_rng(seed)
    for k in ks:
        for name, allow, member in _filters(rng, n, k):
            ids, ds, cnt = ix.search_batch(qs, k, allow=allow, mode="exact")
            assert ix.last_pq_scan_stats() == {"fused_queries": NQ, "sorted_queries": 0}, (k, name)
            for i in range(NQ):
                keep = member[i][full[i][0].astype(np.int64)]
                wi, wd = full[i][0][keep][:k], full[i][1][keep][:k]
                assert cnt[i] == len(wi), (k, name, i)
                _same(ids[i, : cnt[i]], ds[i, : cnt[i]], wi, wd)


@pytest.fixture(scope="module")
def pairs():
    """Per (metric, layout), built once when first asked for: 6,000
    standard-normal rows, 5 % tombstoned, the setting on, nine queries and the
    restatement's ordering of every live row for each."""
    made = {}

    def get(metric, layout):
        if (metric, layout) not in made:
            d, m, ks, use_bits = layout
            ref, ix, _, _, _ = _compressed_pair(N, d, m, ks, metric, use_bits=use_bits)
            rng = np.random.default_rng(200 + m + ks)
            dead = rng.choice(N, N // 20, replace=False)
            for t in dead:
                ref.add_tombstone(int(t))
            ix.add_tombstones(dead)
            ix.set_pq_scan(True)
            qs = _queries(rng, NQ, d, metric)
            full = _restated(ref, N, qs, [np.arange(N, dtype=np.uint64)] * NQ)
            ref.close()
            made[(metric, layout)] = (ix, qs, full)
        return made[(metric, layout)]

    yield get
    for ix, _, _ in made.values():
        ix.close()


@pytest.mark.parametrize("layout", LAYOUTS, ids=LAYOUT_ID)
@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
def test_parity_against_the_restatement(pairs, monkeypatch, metric, layout):
    """Three metrics, five code layouts (groups of 2 and 1 queries and direct
    evaluation by the launcher's rule), k on both sides of a wave step
    and at the kernel's limit, the three kinds of filter."""
    monkeypatch.delenv("WV_PQ_SCAN_ROWS", raising=False)
    monkeypatch.delenv("WV_PQ_SCAN_GROUP", raising=False)
    ix, qs, full = pairs(metric, layout)
    _check(ix, N, qs, full)


@pytest.mark.parametrize("knob", [("WV_PQ_SCAN_ROWS", "256"), ("WV_PQ_SCAN_GROUP", "1"), ("WV_PQ_SCAN_GROUP", "2"),
                                  ("WV_PQ_SCAN_GROUP", "4")],
                         ids=lambda c: "%s-%s" % c)
@pytest.mark.parametrize("metric,li", [("l2-squared", 0), ("dot", 1), ("cosine-dot", 4)])
def test_knobs_do_not_change_the_answers(pairs, monkeypatch, metric, li, knob):
    """Slabs of 256 rows (24 of them, the last of 112 rows: the slab merge
    runs) and every group size -- four queries is never the launcher's own
    choice, and with 64 KiB tables it does not fit: the launcher's choice
    runs -- give the same rows."""
    monkeypatch.delenv("WV_PQ_SCAN_ROWS", raising=False)
    monkeypatch.delenv("WV_PQ_SCAN_GROUP", raising=False)
    monkeypatch.setenv(*knob)
    ix, qs, full = pairs(metric, LAYOUTS[li])
    _check(ix, N, qs, full, ks=(10, 256))


def test_ties_come_back_by_id():
    """A corpus whose second half repeats its first (equal codes, equal
    distances), k = 5 cuts a pair: equal distances come back in id order."""
    rng = np.random.default_rng(7)
    half, d, m, ks, k = 512, 16, 4, 256, 5
    base = np.tile(rng.standard_normal((half, d)).astype(np.float32), (2, 1))
    n = 2 * half
    cent = _centroids(base, m, ks, 7)
    enc = O.pq_encode_kmeans(base, cent)
    ref = O.Index(d, "l2-squared", 16, 64, capacity=n, seed=7)
    ref.add_batch(base, threads=8)
    ref.compress(cent, enc)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    ix.set_pq(cent)
    ix.upload_pq_codes(enc)
    ix.set_compressed(True)
    ix.set_pq_scan(True)
    qs = _queries(rng, NQ, d, "l2-squared")
    full = _restated(ref, n, qs, [np.arange(n, dtype=np.uint64)] * NQ)
    ref.close()
    _check(ix, n, qs, full, ks=(k,))
    ids, ds, _ = ix.search_batch(qs, k, mode="exact")
    ix.close()
    for i in range(NQ):
        assert ds[i, 0] == ds[i, 1] and ids[i, 1] == ids[i, 0] + half   # a row and its copy
        assert ds[i, 4] != ds[i, 3]                                      # the cut pair's first


def test_on_against_off(pairs):
    """One index, the same batches with the setting off, then on: identical
    results.  k = 257 stays on the sort route and the stats say so."""
    ix, qs, _ = pairs("l2-squared", LAYOUTS[0])
    rng = np.random.default_rng(15)
    runs = [(name, 10, qs, allow) for name, allow, _ in _filters(rng, N, 10)]
    runs += [("nq1", 10, qs[:1], None), ("k257", 257, qs, None)]
    got = {}
    for on in (False, True):
        ix.set_pq_scan(on)
        for name, k, q, allow in runs:
            got[(name, on)] = ix.search_batch(q, k, allow=allow, mode="exact")
            fused = len(q) if on and k <= 256 else 0
            assert ix.last_pq_scan_stats() == {"fused_queries": fused, "sorted_queries": len(q) - fused}, (name, on)
    for name, _, _, _ in runs:
        _same_batch(got[(name, False)], got[(name, True)])


def test_delta_rows_beside_the_graph():
    """HNSW mode on a compressed index with rows added after the graph: the
    exact pass over the delta rows takes the fused scan; on equals off."""
    n0, n1, d, m, ks, k = 3000, 3100, 32, 8, 256, 10
    rng = np.random.default_rng(31)
    base = rng.standard_normal((n1, d)).astype(np.float32)
    cent = _centroids(base, m, ks, 31)
    ref = O.Index(d, "l2-squared", 16, 64, capacity=n0, seed=31)
    ref.add_batch(base[:n0], threads=8)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n1, max_connections=16)
    ix.upload_vectors(base[:n0])
    ix.upload_graph(ref.export_graph())
    ref.close()
    ix.set_pq(cent)
    ix.upload_pq_codes(O.pq_encode_kmeans(base[:n0], cent))
    ix.set_compressed(True)
    ix.add(np.arange(n0, n1), base[n0:])
    qs = np.concatenate([_queries(rng, NQ - 3, d, "l2-squared"), base[n0 : n0 + 3]])   # three sit on added rows
    each = [W.AllowList.from_ids(np.sort(rng.choice(n1, n1 // 3, replace=False)), n1) for _ in range(NQ)]
    got = {}
    for on in (False, True):
        ix.set_pq_scan(on)
        for name, allow in (("none", None), ("each", each)):
            got[(name, on)] = ix.search_batch(qs, k, ef=64, allow=allow, mode="hnsw")
            st = ix.last_pq_scan_stats()
            assert (st["fused_queries"] >= NQ, st["sorted_queries"] == 0) == (on, on), (name, on, st)
    ix.close()
    for name in ("none", "each"):
        _same_batch(got[(name, False)], got[(name, True)])
    assert (got[("none", True)][0][NQ - 3 :] >= n0).any()   # added rows are found
