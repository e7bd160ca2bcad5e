"""Manhattan and hamming indexes: exact search and distance search (wv_l1.hip).

The reference is the distancers' own order in numpy: one float32 sum per
(query, row), dimension by dimension; the expected rows are the eligible ones
in (dist, id) order.  The GPU must return the same ids and distance bits, and
every distance stays within D 2^-23 relative of the float64 sum (D + 1
roundings per chain).

Constants the cases are sized for: 128-row tiles, 64-query (wide) and 8-query
(narrow, nq <= 128) blocks, 16-float k chunks, L1_KMAX = 128.
  37x1     one partial tile, narrow block, D = 1
  777x100  129 queries: wide blocks, the third with one query; partial last
           tile; one tile per segment (7 segments merged); shared allow list
           + tombstones
  1303x33  two narrow blocks, D no multiple of 4 or 16; per-query allow lists
  5000x130 130 queries (wide); k = L1_KMAX with WV_L1_SEGS=3: 14-tile segments, every pool pruned
           more than once, partial last k chunk, per-query allow lists
Runs on an MI355X (-m gpu).
"""
import numpy as np
import pytest

import weaviate_amd as W

pytestmark = pytest.mark.gpu

KMAX = 128
METRICS = ["manhattan", "hamming"]


def _data(metric, kind, n, nq, d, seed):
    rng = np.random.default_rng(seed)
    if metric == "hamming":
        draw = lambda m: rng.integers(0, 3, (m, d)).astype(np.float32)
    elif kind == "ints":
        draw = lambda m: rng.integers(-2, 3, (m, d)).astype(np.float32)
    else:
        draw = lambda m: (rng.random((m, d), dtype=np.float32) * 2 - 1).astype(np.float32)
    return draw(n), draw(nq), rng


def _reference(metric, base, qs):
    """[nq][n] float32 chains in dimension order, and the float64 sums."""
    s = np.zeros((qs.shape[0], base.shape[0]), np.float32)
    d64 = np.zeros(s.shape, np.float64)
    for i in range(base.shape[1]):
        a, b = qs[:, i:i + 1], base[None, :, i]
        s += np.abs(a - b) if metric == "manhattan" else (a != b).astype(np.float32)
        d64 += np.abs(a.astype(np.float64) - b) if metric == "manhattan" else (a != b)
    return s, d64


def _filters(rng, kind, n, nq, tombs):
    """eligible [nq][n] bool, the allow argument, the tombstoned ids"""
    dead = rng.choice(n, n // 10, replace=False) if tombs else np.zeros(0, np.int64)
    ok = np.ones((nq, n), bool)
    allow = None
    if kind == "shared":
        ids = np.flatnonzero(rng.random(n) < 0.6)
        ok[:, :] = np.isin(np.arange(n), ids)[None]
        allow = W.AllowList.from_ids(ids.tolist(), n)
    elif kind == "perq":
        m = rng.random((nq, n)) < 0.7
        ok &= m
        allow = [W.AllowList.from_ids(np.flatnonzero(r).tolist(), n) for r in m]
    ok[:, dead] = False
    return ok, allow, dead


def _index(metric, base, dead):
    ix = W.GPUVectorIndex(base.shape[1], metric, capacity=base.shape[0])
    ix.upload_vectors(base)
    if len(dead):
        ix.set_tombstones(dead.tolist())
    return ix


def _check_knn(got, s, d64, ok, k, d):
    ids, ds, cnt = got
    for q in range(s.shape[0]):
        rows = np.flatnonzero(ok[q])
        want = rows[np.lexsort((rows, s[q, rows]))][:k]
        assert cnt[q] == len(want), q
        assert ids[q, :cnt[q]].tolist() == want.tolist(), q
        assert np.array_equal(ds[q, :cnt[q]].view(np.uint32), s[q, want].view(np.uint32)), q
        assert (np.abs(ds[q, :cnt[q]] - d64[q, want]) <= d * 2.0 ** -23 * d64[q, want]).all(), q


CASES = [
    pytest.param(37, 1, 1, 10, None, False, None, "uniform", id="37x1-q1-k10"),
    pytest.param(777, 100, 129, 10, "shared", True, None, "uniform", id="777x100-q129-k10-shared-tombs"),
    pytest.param(777, 100, 129, 10, "shared", True, None, "ints", id="777x100-q129-k10-ties"),
    pytest.param(1303, 33, 9, 1, "perq", False, None, "uniform", id="1303x33-q9-k1-perq"),
    pytest.param(5000, 130, 130, KMAX, "perq", False, "3", "uniform", id="5000x130-q130-kmax-perq-3seg"),
    pytest.param(777, 100, 129, KMAX + 1, "shared", True, None, "uniform", id="777x100-q129-scan-route"),
]


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,nq,k,allow_kind,tombs,segs,kind", CASES)
def test_knn_ids_and_bits_match_the_serial_chain(monkeypatch, metric, n, d, nq, k, allow_kind, tombs, segs, kind):
    if segs:
        monkeypatch.setenv("WV_L1_SEGS", segs)
    base, qs, rng = _data(metric, kind, n, nq, d, 7)
    ok, allow, dead = _filters(rng, allow_kind, n, nq, tombs)
    s, d64 = _reference(metric, base, qs)
    ix = _index(metric, base, dead)
    got = ix.search_batch(qs, k, allow=allow, mode="exact" if k <= KMAX else "auto")
    ix.close()
    _check_knn(got, s, d64, ok, k, d)


@pytest.mark.parametrize("metric", METRICS)
def test_short_allow_list_returns_its_rows(metric):
    base, qs, _ = _data(metric, "uniform", 777, 3, 100, 8)
    keep = [5, 130, 131, 640, 776]
    ok = np.zeros((3, 777), bool)
    ok[:, keep] = True
    s, d64 = _reference(metric, base, qs)
    ix = _index(metric, base, [])
    got = ix.search_batch(qs, 10, allow=W.AllowList.from_ids(keep, 777))
    ix.close()
    assert got[2].tolist() == [5, 5, 5]
    _check_knn(got, s, d64, ok, 10, 100)


def _check_sets(res, counts, s, ok, targets):
    for q in range(s.shape[0]):
        rows = np.flatnonzero(ok[q] & (s[q].astype(np.float64) - np.float64(targets[q]) <= 1e-6))
        want = rows[np.lexsort((rows, s[q, rows]))]
        assert counts[q] == len(want), q
        assert res[q][0].tolist() == want.tolist(), q
        assert np.array_equal(res[q][1].view(np.uint32), s[q, want].view(np.uint32)), q


@pytest.mark.parametrize("metric", METRICS)
@pytest.mark.parametrize("n,d,nq,allow_kind,tombs", [
    pytest.param(777, 100, 129, "shared", True, id="777x100-q129-shared-tombs"),
    pytest.param(1303, 33, 9, "perq", False, id="1303x33-q9-perq"),
])
def test_distance_search_sets_match(metric, n, d, nq, allow_kind, tombs):
    """Targets: each query's 30th-smallest reference distance (hamming: an integer with ties on it)."""
    base, qs, rng = _data(metric, "uniform", n, nq, d, 9)
    ok, allow, dead = _filters(rng, allow_kind, n, nq, tombs)
    s, _ = _reference(metric, base, qs)
    targets = np.array([np.sort(s[q, ok[q]])[29] for q in range(nq)], np.float32)
    ix = _index(metric, base, dead)
    res, counts = ix.search_by_vector_distance_batch(qs, targets, -1, allow=allow, cap=n)
    st = ix.last_sbd_stats()
    ix.close()
    assert st == {"pass_queries": nq, "hnsw_round1_queries": 0, "legacy_queries": 0}
    _check_sets(res, counts, s, ok, targets)


@pytest.mark.parametrize("metric", METRICS)
def test_distance_search_past_the_list_cap(monkeypatch, metric):
    """WV_SBD_CAP=128 and ~700 rows within two queries' targets: those take the per-query path."""
    monkeypatch.setenv("WV_SBD_CAP", "128")
    base, qs, _ = _data(metric, "uniform", 777, 3, 100, 10)
    s, _ = _reference(metric, base, qs)
    ok = np.ones((3, 777), bool)
    targets = np.array([np.sort(s[0])[29], np.sort(s[1])[699], np.sort(s[2])[699]], np.float32)
    ix = _index(metric, base, [])
    res, counts = ix.search_by_vector_distance_batch(qs, targets, -1, cap=777)
    st = ix.last_sbd_stats()
    ix.close()
    assert st["legacy_queries"] == 2 and st["pass_queries"] == 1, st
    _check_sets(res, counts, s, ok, targets)


@pytest.mark.parametrize("metric", METRICS)
def test_empty_index_answers_nothing(metric):
    ix = W.GPUVectorIndex(8, metric, capacity=64)
    qs = np.ones((3, 8), np.float32)
    assert ix.search_batch(qs, 5)[2].tolist() == [0, 0, 0]
    res, counts = ix.search_by_vector_distance_batch(qs, 1e9, -1, cap=4)
    ix.close()
    assert counts.tolist() == [0, 0, 0] and all(len(r[0]) == 0 for r in res)


@pytest.mark.parametrize("metric", METRICS)
def test_graph_and_quantizer_are_refused(metric):
    base, qs, _ = _data(metric, "uniform", 64, 2, 8, 11)
    ix = _index(metric, base, [])
    for call in (lambda: ix.search_batch(qs, 5, mode="hnsw"), lambda: ix.build_graph(),
                 lambda: ix.set_pq(np.zeros((2, 4, 4), np.float32))):
        with pytest.raises(W.WvError) as e:
            call()
        assert e.value.code == 4 and metric in str(e.value)   # WV_ESTATE
    ix.close()
