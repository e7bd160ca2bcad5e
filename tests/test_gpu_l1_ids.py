"""Manhattan and hamming indexes over per-query allow lists given as ids
(wv_l1_ids.hip): search_batch_ids, search_by_vector_distance_batch_ids and the
batcher's calls.

The reference is tests/test_gpu_l1.py's: one float32 sum per (query, row),
dimension by dimension, in numpy; the expected rows are the list's eligible
ids (below n_rows, not tombstoned) in (dist, id) order.  The GPU must return
the same ids and distance bits, and every distance stays within D 2^-23
relative of the float64 sum (D + 1 roundings per chain).

6,000 rows, 16 queries, one list length per query: empty, one id, around k,
around a wave step (64), a stage (256), a long list's chunks (1,024, 2,049)
and nearly every row.  Every list that is long enough holds ids past the rows
and tombstoned ids.  Runs on an MI355X (-m gpu).
"""
import functools
import threading

import numpy as np
import pytest

import weaviate_amd as W

pytestmark = pytest.mark.gpu

N, NQ = 6000, 16
DATA = [("manhattan", "uniform"), ("manhattan", "ints"), ("hamming", "ints")]
RANKS = [40, 100, 101, 1100, 1101, 2500]


def _lengths(k):
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5999]


def _reference(metric, base, qs):
    """[nq][n] float32 chains in dimension order, and the float64 sums."""
    s = np.zeros((qs.shape[0], base.shape[0]), np.float32)
    d64 = np.zeros(s.shape, np.float64)
    for i in range(base.shape[1]):
        a, b = qs[:, i:i + 1], base[None, :, i]
        s += np.abs(a - b) if metric == "manhattan" else (a != b).astype(np.float32)
        d64 += np.abs(a.astype(np.float64) - b) if metric == "manhattan" else (a != b)
    return s, d64


@functools.lru_cache(maxsize=None)
def _setup(metric, kind, d):
    """data, reference and index of one (metric, data, D): built once, never changed"""
    rng = np.random.default_rng(17 + d)
    if kind == "ints":
        draw = lambda m: rng.integers(-2, 3, (m, d)).astype(np.float32)
    else:
        draw = lambda m: (rng.random((m, d), dtype=np.float32) * 2 - 1).astype(np.float32)
    base, qs = draw(N), draw(NQ)
    dead = np.sort(rng.choice(N, N // 10, replace=False))
    s, d64 = _reference(metric, base, qs)
    ix = W.GPUVectorIndex(d, metric, capacity=N)
    ix.upload_vectors(base)
    ix.set_tombstones(dead.tolist())
    _OPEN.append(ix)
    return base, qs, dead, s, d64, ix


_OPEN = []


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    while _OPEN:
        _OPEN.pop().close()
    _setup.cache_clear()


def _lists(dead, lengths, seed=3):
    """ascending lists; where long enough: ids past the rows (two the device drops, one the host does) and dead ids"""
    rng = np.random.default_rng(seed)
    out = []
    for L in lengths:
        past = [N + 5, N + 1000, 2 ** 31 + 7][:L // 4]
        forced = rng.choice(dead, min(2, (L - len(past)) // 2), replace=False)
        rest = rng.choice(np.setdiff1d(np.arange(N), forced), L - len(past) - len(forced), replace=False)
        out.append(np.concatenate([np.sort(np.concatenate([forced, rest])), past]).astype(np.uint64))
    return out


def _eligible(lists, dead):
    ok = np.zeros((len(lists), N), bool)
    for q, ls in enumerate(lists):
        ok[q, ls[ls < N].astype(np.int64)] = True
    ok[:, dead] = False
    return ok


def _check_knn(got, s, d64, ok, k, d):
    ids, ds, cnt = got
    for q in range(s.shape[0]):
        rows = np.flatnonzero(ok[q])
        want = rows[np.lexsort((rows, s[q, rows]))][:k]
        assert cnt[q] == len(want), q
        assert ids[q, :cnt[q]].tolist() == want.tolist(), q
        assert np.array_equal(ds[q, :cnt[q]].view(np.uint32), s[q, want].view(np.uint32)), q
        assert (np.abs(ds[q, :cnt[q]] - d64[q, want]) <= d * 2.0 ** -23 * d64[q, want]).all(), q


@pytest.mark.parametrize("k", [1, 10, 128, 129, 256])
@pytest.mark.parametrize("d", [1, 33, 130])
@pytest.mark.parametrize("metric,kind", DATA)
def test_knn_over_lists_matches_the_serial_chain(metric, kind, d, k):
    base, qs, dead, s, d64, ix = _setup(metric, kind, d)
    lists = _lists(dead, _lengths(k))
    got = ix.search_batch_ids(qs, k, lists)
    assert ix.last_sparse_stats() == {"sparse_queries": NQ, "sparse_ids": sum(len(x) for x in lists),
                                      "bitmap_queries": 0}
    _check_knn(got, s, d64, _eligible(lists, dead), k, d)


@pytest.mark.parametrize("d", [33, 130])
@pytest.mark.parametrize("metric,kind", DATA)
def test_one_long_list_is_cut_into_chunks(metric, kind, d):
    """One query: its 5,999 ids go to chunks of 256-512 ids, merged by flat_ids_merge_kernel."""
    base, qs, dead, s, d64, ix = _setup(metric, kind, d)
    lists = _lists(dead, [5999])
    got = ix.search_batch_ids(qs[:1], 256, lists)
    assert ix.last_sparse_stats()["sparse_queries"] == 1
    _check_knn(got, s[:1], d64[:1], _eligible(lists, dead), 256, d)


def _targets(s, ok):
    """query q: its list's own distance at one of RANKS, as far as the list is long enough for"""
    t = np.zeros(ok.shape[0], np.float32)
    for q in range(ok.shape[0]):
        ds = np.sort(s[q, ok[q]])
        fit = [r for r in RANKS if r < len(ds)] or [len(ds) - 1]
        t[q] = ds[fit[q % len(fit)]] if len(ds) else 1.0
    return t


@pytest.mark.parametrize("d", [1, 33, 130])
@pytest.mark.parametrize("metric,kind", DATA)
def test_distance_search_over_lists_matches_numpy(metric, kind, d):
    base, qs, dead, s, d64, ix = _setup(metric, kind, d)
    lists = _lists(dead, _lengths(10))
    ok = _eligible(lists, dead)
    targets = _targets(s, ok)
    res, counts = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=N)
    assert ix.last_sbd_ids_stats() == {"list_queries": NQ, "list_ids": sum(len(x) for x in lists),
                                       "hnsw_round1_queries": 0, "legacy_queries": 0}
    for q in range(NQ):
        rows = np.flatnonzero(ok[q] & (s[q].astype(np.float64) - np.float64(targets[q]) <= 1e-6))
        want = rows[np.lexsort((rows, s[q, rows]))]
        assert counts[q] == len(want), q
        assert res[q][0].tolist() == want.tolist(), q
        assert np.array_equal(res[q][1].view(np.uint32), s[q, want].view(np.uint32)), q
        assert (np.abs(res[q][1] - d64[q, want]) <= d * 2.0 ** -23 * d64[q, want]).all(), q


@pytest.mark.parametrize("max_limit,cap", [(-1, 4096), (150, 4096), (1100, 120)])
@pytest.mark.parametrize("metric,kind", DATA)
def test_distance_search_deepens_as_the_bitmap_route(metric, kind, max_limit, cap):
    base, qs, dead, s, d64, ix = _setup(metric, kind, 33)
    lists = _lists(dead, _lengths(10))
    targets = _targets(s, _eligible(lists, dead))
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, max_limit, cap=cap)
    allow = [W.AllowList.from_ids(ls[ls < N].tolist(), N) for ls in lists]
    want, want_n = ix.search_by_vector_distance_batch(qs, targets, max_limit, allow=allow, cap=cap)
    assert got_n.tolist() == want_n.tolist()
    for q in range(NQ):
        assert got[q][0].tolist() == want[q][0].tolist(), q
        assert np.array_equal(got[q][1].view(np.uint32), want[q][1].view(np.uint32)), q


def test_batcher_calls_return_the_direct_answers():
    base, qs, dead, s, d64, ix = _setup("manhattan", "uniform", 33)
    nt = 8
    lists = _lists(dead, [300 + 40 * t for t in range(nt)])
    targets = _targets(s, _eligible(lists, dead))
    want_k = ix.search_batch_ids(qs[:nt], 10, lists)
    want_d, _ = ix.search_by_vector_distance_batch_ids(qs[:nt], targets, lists, -1, cap=4096)
    b = W.Batcher(ix, max_batch=nt, max_wait_us=5_000_000)
    calls = [lambda t: b.search_ids(qs[t], 10, lists[t]),
             lambda t: b.search_distance_ids(qs[t], float(targets[t]), -1, lists[t])]
    got = [[None] * nt for _ in calls]
    for r, call in enumerate(calls):
        th = [threading.Thread(target=lambda t=t: got[r].__setitem__(t, call(t))) for t in range(nt)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
    b.close()
    for t in range(nt):
        (ki, kd), (di, dd) = got[0][t], got[1][t]
        assert ki.tolist() == want_k[0][t, :want_k[2][t]].tolist(), t
        assert np.array_equal(kd.view(np.uint32), want_k[1][t, :want_k[2][t]].view(np.uint32)), t
        assert di.tolist() == want_d[t][0].tolist(), t
        assert np.array_equal(dd.view(np.uint32), want_d[t][1].view(np.uint32)), t
