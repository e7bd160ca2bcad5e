"""Flat search over per-query allow lists given as ids (wv_search_batch_ids):
the sparse kernel against the CPU restatement, and the whole entry point
against the bitmap route of wv_search_batch.

Bar: ids, distance bits and counts identical -- every distance is computed in
the reference's summation order and (dist, id) orders the results.  Runs on an
MI355X (-m gpu).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W

pytestmark = pytest.mark.gpu

METRICS = {"l2-squared": O.L2, "dot": O.DOT, "cosine-dot": O.COSINE}
N, NQ = 20000, 48


def _same(a_ids, a_d, b_ids, b_d):
    assert a_ids.tolist() == b_ids.tolist()
    assert np.array_equal(a_d.view(np.uint32), b_d.view(np.uint32))


def _same_batch(a, b):
    assert a[2].tolist() == b[2].tolist()
    for i in range(len(a[2])):
        _same(a[0][i, : a[2][i]], a[1][i, : a[2][i]], b[0][i, : b[2][i]], b[1][i, : b[2][i]])


def _lists(rng, n, lengths):
    return [np.sort(rng.choice(n, int(L), replace=False)).astype(np.uint64) for L in lengths]


def _allow(lists, n):
    return [W.AllowList.from_ids(a[a < n], n) for a in lists]


def _oracle(metric, base, qs, k, lists, tomb=None):
    """flat_scan per query over its own list (ids past the rows name nothing),
    in (dist, id) order with no tie exemption.  The restatement's own top k
    orders equal distances by heap layout, and fp32 distances do
    tie at these sizes (20,000 x 768 uniform rows: two of the 2049 listed rows
    of one query), so it is asked for every listed row -- its distances, bit
    for bit -- and the first k by (dist, id) are the expected result."""
    n = base.shape[0]
    out = []
    for i, a in enumerate(lists):
        a = a[a < n]
        bits = O.bits_from_ids(a, n)
        oi, od, on = O.flat_scan(metric, base, qs[i:i + 1], max(k, len(a)), allow_bits=bits, tomb_bits=tomb,
                                 threads=1)
        order = np.lexsort((oi[0, : on[0]], od[0, : on[0]]))[:k]
        out.append((oi[0, : on[0]][order], od[0, : on[0]][order]))
    return out


@pytest.mark.parametrize("dim", [5, 100, 128, 768])
@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
def test_sparse_flat_parity_against_oracle(metric, dim):
    """Mode exact, every k and list length that crosses a boundary of the
    kernel (a wave step, the staging size, a chunk), ids past the rows and
    tombstones: ids, distance bits and counts equal the restatement, and the
    stats show that only the listed rows were handed to the sparse kernel."""
    rng = np.random.default_rng(1000 + dim)
    base = rng.random((N, dim), dtype=np.float32)
    qs = rng.random((NQ, dim), dtype=np.float32)
    if metric != "l2-squared":
        base -= 0.5
        qs -= 0.5
    dead = rng.choice(N, N // 20, replace=False)
    tomb = O.bits_from_ids(dead, N)
    ix = W.GPUVectorIndex(dim, metric, capacity=N)
    ix.upload_vectors(base)
    ix.set_tombstones(dead)
    ob = O.normalize_rows(base) if metric == "cosine-dot" else base
    oq = O.normalize_rows(qs) if metric == "cosine-dot" else qs
    for k in (1, 10, 32, 33, 256):
        pool = [0, 1, k - 1, k, k + 1, 31, 32, 33, 63, 64, 65, 255, 256, 257, 2049]
        lengths = [pool[(i + k) % len(pool)] for i in range(NQ)]
        lists = _lists(rng, N, lengths)
        # ids past the rows (and past 2^31) are skipped, not refused
        for i in range(0, NQ, 5):
            lists[i] = np.concatenate([lists[i], np.array([N, N + 77, (1 << 31) + 5, 1 << 40], np.uint64)])
        ids, ds, n = ix.search_batch_ids(qs, k, lists, mode="exact")
        st = ix.last_sparse_stats()
        want = _oracle(METRICS[metric], ob, oq, k, lists, tomb)
        for i in range(NQ):
            assert n[i] == len(want[i][0]), (k, i, lengths[i])
            _same(ids[i, : n[i]], ds[i, : n[i]], want[i][0], want[i][1])
        assert st == {"sparse_queries": NQ, "sparse_ids": sum(a.size for a in lists), "bitmap_queries": 0}, (k, st)
    ix.close()


def test_ties_come_back_by_id():
    """64 distinct vectors, each stored 8 times; lists of whole duplicate
    groups, k = 10 (a group and a quarter).  Equal distances come back in
    ascending id order, and the result is the restatement's: its distances of
    every listed row, ordered by (dist, id).  (The restatement's own top-k
    keeps and orders equal distances by heap layout, SURVEY 8c, so it is asked
    for the whole list and the order among equal distances is made the id's.)"""
    rng = np.random.default_rng(7)
    groups, rep, dim, k = 64, 8, 16, 10
    base = np.repeat(rng.random((groups, dim), dtype=np.float32), rep, axis=0)
    n = groups * rep
    qs = rng.random((NQ, dim), dtype=np.float32)
    lists = []
    for i in range(NQ):
        g = np.sort(rng.choice(groups, 2 + i % 6, replace=False))   # 8 L < n: the sparse route in mode exact
        lists.append((g[:, None] * rep + np.arange(rep)[None, :]).reshape(-1).astype(np.uint64))
    ix = W.GPUVectorIndex(dim, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    ids, ds, cnt = ix.search_batch_ids(qs, k, lists, mode="exact")
    assert ix.last_sparse_stats()["sparse_queries"] == NQ
    ix.close()
    for i, a in enumerate(lists):
        oi, od, on = O.flat_scan(O.L2, base, qs[i:i + 1], len(a), allow_bits=O.bits_from_ids(a, n), threads=1)
        assert on[0] == len(a)
        order = np.lexsort((oi[0], od[0]))[:k]
        assert cnt[i] == k
        _same(ids[i], ds[i], oi[0][order], od[0][order])
        for v in np.unique(ds[i]):
            same = ids[i][ds[i] == v]
            assert (np.diff(same.astype(np.int64)) > 0).all()
        assert len(np.unique(ds[i])) < k   # the case does hold equal distances


@pytest.fixture(scope="module")
def graph3000():
    n, d = 3000, 32
    rng = np.random.default_rng(21)
    base = rng.random((n, d), dtype=np.float32)
    qs = rng.random((NQ, d), dtype=np.float32)
    ref = O.Index(d, "l2-squared", 16, 64, capacity=n)
    ref.add_batch(base, threads=8)
    return base, qs, ref.export_graph()


def _graph_index(graph3000, capacity=3000, **kw):
    base, _, g = graph3000
    ix = W.GPUVectorIndex(base.shape[1], "l2-squared", capacity=capacity, max_connections=16, **kw)
    ix.upload_vectors(base)
    ix.upload_graph(g)
    return ix


def test_equal_to_bitmap_route_exact():
    """k = 257 and lists of half the rows go down the bitmap route, short
    lists on an index with an id base down the sparse one: all bit-identical
    to wv_search_batch over per-query bitmaps."""
    rng = np.random.default_rng(3)
    d = 64
    base = rng.random((N, d), dtype=np.float32)
    qs = rng.random((NQ, d), dtype=np.float32)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=N)
    ix.upload_vectors(base)
    lists = _lists(rng, N, [300 + i for i in range(NQ)])
    _same_batch(ix.search_batch_ids(qs, 257, lists, mode="exact"),
                ix.search_batch(qs, 257, allow=_allow(lists, N), mode="exact"))
    assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": NQ}
    half = _lists(rng, N, [N // 2] * 8)
    _same_batch(ix.search_batch_ids(qs[:8], 10, half, mode="exact"),
                ix.search_batch(qs[:8], 10, allow=_allow(half, N), mode="exact"))
    assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": 8}
    # a mixed batch: each query's row comes from its own route
    mixed = [half[i % 8] if i % 3 == 0 else lists[i] for i in range(NQ)]
    _same_batch(ix.search_batch_ids(qs, 10, mixed, mode="exact"),
                ix.search_batch(qs, 10, allow=_allow(mixed, N), mode="exact"))
    st = ix.last_sparse_stats()
    assert (st["sparse_queries"], st["bitmap_queries"]) == (NQ - NQ // 3, NQ // 3)
    ix.close()
    sh = W.GPUVectorIndex(d, "l2-squared", capacity=N, id_base=64000)
    sh.upload_vectors(base)
    got = sh.search_batch_ids(qs, 10, lists, mode="exact")
    _same_batch(got, sh.search_batch(qs, 10, allow=_allow(lists, N), mode="exact"))
    assert sh.last_sparse_stats()["sparse_queries"] == NQ
    assert (got[0] >= 64000).all()
    sh.close()


def test_large_batch_of_long_lists():
    """More than 512 K ids in a batch: the host checks and narrows the lists
    in threads, and a list runs as many chunks.  Lists of 33,000 ids out of
    [0, 40000) over 20,000 rows (mode auto, no graph: flat below the cutoff)
    equal the bitmap route; a list out of order in any thread's share is
    refused."""
    rng = np.random.default_rng(17)
    d, nq, k = 32, 16, 33
    base = rng.random((N, d), dtype=np.float32)
    qs = rng.random((nq, d), dtype=np.float32)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=N)
    ix.upload_vectors(base)
    lists = _lists(rng, 2 * N, [33000] * nq)
    got = ix.search_batch_ids(qs, k, lists, mode="auto")
    assert ix.last_sparse_stats() == {"sparse_queries": nq, "sparse_ids": 33000 * nq, "bitmap_queries": 0}
    _same_batch(got, ix.search_batch(qs, k, allow=_allow(lists, N), mode="auto"))
    for bad_q in (0, nq // 2, nq - 1):
        bad = [a.copy() for a in lists]
        bad[bad_q][[20000, 20001]] = bad[bad_q][[20001, 20000]]
        with pytest.raises(W.WvError) as e:
            ix.search_batch_ids(qs, k, bad, mode="auto")
        assert e.value.code == 1 and "ascending" in str(e.value)
    ix.close()


def test_equal_to_bitmap_route_compressed():
    """A PQ-compressed index ranks by the PQ distance: every query goes down
    the bitmap route, in every mode."""
    from test_pq import _compressed_pair
    n, d = 6000, 32
    ref, ix, base, _, _ = _compressed_pair(n, d, 8, 256)
    rng = np.random.default_rng(8)
    qs = rng.standard_normal((NQ, d)).astype(np.float32)
    lists = _lists(rng, n, [10 + 20 * i for i in range(NQ)])
    for mode in ("exact", "auto"):
        _same_batch(ix.search_batch_ids(qs, 10, lists, mode=mode),
                    ix.search_batch(qs, 10, allow=_allow(lists, n), mode=mode))
        assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": NQ}
    ix.close()
    ref.close()


def test_equal_to_bitmap_route_hnsw(graph3000):
    base, qs, _ = graph3000
    n = base.shape[0]
    ix = _graph_index(graph3000)
    rng = np.random.default_rng(9)
    lists = _lists(rng, n, [30 + 50 * i for i in range(NQ)])
    _same_batch(ix.search_batch_ids(qs, 10, lists, ef=64, mode="hnsw"),
                ix.search_batch(qs, 10, ef=64, allow=_allow(lists, n), mode="hnsw"))
    assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": NQ}
    ix.close()


def test_auto_dispatch_by_list_length(graph3000):
    """search.go:64-79 from the list's length: below the cutoff flat (the
    sparse kernel, equal to the restatement), at or above it HNSW (equal to
    the engine's own answer over bitmaps: the same kernels); forbid_flat sends
    every query to HNSW."""
    base, qs, _ = graph3000
    n = base.shape[0]
    ix = _graph_index(graph3000, flat_search_cutoff=50)
    rng = np.random.default_rng(10)
    lengths = [(0, 49, 50, 400)[i % 4] for i in range(NQ)]
    lists = _lists(rng, n, lengths)
    k = 10
    got = ix.search_batch_ids(qs, k, lists, mode="auto")
    st = ix.last_sparse_stats()
    assert st == {"sparse_queries": NQ // 2, "sparse_ids": (NQ // 4) * 49, "bitmap_queries": NQ // 2}
    bm = ix.search_batch(qs, k, allow=_allow(lists, n), mode="auto")
    want = _oracle(O.L2, base, qs, k, lists)
    for i in range(NQ):
        g = (got[0][i, : got[2][i]], got[1][i, : got[2][i]])
        if lengths[i] < 50:
            assert got[2][i] == min(k, lengths[i])
            _same(g[0], g[1], want[i][0], want[i][1])
        else:
            assert got[2][i] == bm[2][i]
            _same(g[0], g[1], bm[0][i, : bm[2][i]], bm[1][i, : bm[2][i]])
    ix.update_user_config(forbid_flat=1)
    _same_batch(ix.search_batch_ids(qs, k, lists, mode="auto"),
                ix.search_batch(qs, k, allow=_allow(lists, n), mode="hnsw"))
    assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": NQ}
    ix.close()


def test_delta_rows_are_listed_rows(graph3000):
    """Rows added after the graph snapshot are live: a list that names three
    of them gets them back, as the restatement's scan over the listed rows."""
    base, qs, _ = graph3000
    n = base.shape[0]
    ix = _graph_index(graph3000, capacity=n + 100, flat_search_cutoff=50)
    rng = np.random.default_rng(11)
    new = rng.random((10, base.shape[1]), dtype=np.float32)
    ix.add(np.arange(n, n + 10, dtype=np.uint64), new)
    allb = np.vstack([base, new])
    lists = []
    for i in range(NQ):
        a = np.concatenate([rng.choice(n, 17, replace=False), n + rng.choice(10, 3, replace=False)])
        lists.append(np.sort(a).astype(np.uint64))
    # the query is one of the added rows' neighbours: they must rank
    qs = qs.copy()
    qs[:10] = new + np.float32(1e-3)
    got = ix.search_batch_ids(qs, 20, lists, mode="auto")
    assert ix.last_sparse_stats()["sparse_queries"] == NQ
    want = _oracle(O.L2, allb, qs, 20, lists)
    for i in range(NQ):
        assert got[2][i] == 20
        _same(got[0][i], got[1][i], want[i][0], want[i][1])
        assert (got[0][i] >= n).sum() == 3
    ix.close()


@pytest.mark.parametrize("send_ids", [None, "0"])
def test_batcher_sends_id_lists(graph3000, monkeypatch, send_ids):
    """32 threads with lists of their own around the cutoff, k 10 and 40: every
    answer equals a direct search over the same list as a bitmap, and the
    batches went out as ids (WV_BATCHER_IDS=0: as bitmap rows, same answers)."""
    if send_ids is None:
        monkeypatch.delenv("WV_BATCHER_IDS", raising=False)
    else:
        monkeypatch.setenv("WV_BATCHER_IDS", send_ids)
    base, qs, _ = graph3000
    n = base.shape[0]
    ix = _graph_index(graph3000, flat_search_cutoff=50)
    rng = np.random.default_rng(12)
    nt = 32
    # rounds of one request per thread (the batcher waits for all 32): k 10 and
    # 40 over lengths around the cutoff, then short lists only
    rounds = [(10, [(10, 48, 49, 50, 51, 400)[t % 6] for t in range(nt)]),
              (40, [(49, 50, 39, 41, 300, 40)[t % 6] for t in range(nt)]),
              (10, [20 + t for t in range(nt)])]
    lists = [[_lists(rng, n, [L])[0] for L in lens] for _, lens in rounds]
    want = [[ix.search_by_vector(qs[t], k, allow=W.AllowList.from_ids(lists[r][t], n)) for t in range(nt)]
            for r, (k, _) in enumerate(rounds)]
    b = W.Batcher(ix, max_batch=nt, max_wait_us=5_000_000)
    got = [[None] * nt for _ in rounds]

    def worker(t):
        for r, (k, _) in enumerate(rounds):
            got[r][t] = b.search_ids(qs[t], k, lists[r][t])

    th = [threading.Thread(target=worker, args=(t,)) for t in range(nt)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    b.close()
    st = ix.last_sparse_stats()
    ix.close()
    for r in range(len(rounds)):
        for t in range(nt):
            _same(got[r][t][0], got[r][t][1], want[r][t][0], want[r][t][1])
    if send_ids is None:
        assert st["sparse_queries"] > 0, st
    else:
        assert st == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": 0}


def test_bad_lists_are_refused(graph3000):
    """Offsets that do not start at 0 or decrease, and ids that do not ascend
    within a query, return WV_EINVAL."""
    base, qs, _ = graph3000
    ix = W.GPUVectorIndex(base.shape[1], "l2-squared", capacity=base.shape[0])
    ix.upload_vectors(base)
    q = np.ascontiguousarray(qs[:2])
    out_i, out_d, out_n = np.zeros((2, 5), np.uint64), np.zeros((2, 5), np.float32), np.zeros(2, np.int32)

    def call(ids, off):
        ids, off = np.asarray(ids, np.uint64), np.asarray(off, np.uint64)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        return W.lib().wv_search_batch_ids(ix._h, vp(q), 2, 5, 0, vp(ids), vp(off), 1, vp(out_i), vp(out_d), vp(out_n))

    assert call([1, 2, 3, 4], [0, 2, 4]) == 0
    assert call([1, 2, 3, 4], [1, 2, 4]) == 1
    assert b"allow_offsets[0]" in W.lib().wv_last_error()
    assert call([1, 2, 3, 4], [0, 3, 2]) == 1
    assert b"decrease" in W.lib().wv_last_error()
    assert call([2, 1, 3, 4], [0, 2, 4]) == 1
    assert b"ascending" in W.lib().wv_last_error()
    assert call([1, 1, 3, 4], [0, 2, 4]) == 1
    # ascending is per query: the second list may start below the first's end
    assert call([5, 9, 3, 4], [0, 2, 4]) == 0
    with pytest.raises(W.WvError):
        ix.search_batch_ids(qs[:2], 5, [np.array([1, 2], np.uint64)])
    ix.close()
