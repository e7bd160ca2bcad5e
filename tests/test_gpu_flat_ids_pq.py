"""Flat search over per-query id lists on a PQ-compressed index
(wv_index_set_pq_list_search + wv_search_batch_ids): the list kernel over the
codes (flat_ids_pq_kernel: lookup table and direct evaluation) against the CPU
restatement, and the whole entry point with the setting on against off.

The yardstick is never the new code.  The restatement is asked, per query, for
the PQ distance of every listed live row (a flat search over the list as a
bitmap with k = the list's length); those ordered by (dist, id) and cut to k
are the expected rows -- the restatement's own top k orders equal distances by
heap layout.  Bar: ids, distance bits and counts identical.  Runs
on an MI355X (-m gpu).
"""
import threading

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from test_pq import _centroids, _compressed_pair

pytestmark = pytest.mark.gpu

N, NQ = 6000, 32
KS_ALL = (1, 10, 64, 65, 256)
# (d, m, ks, use_bits): narrow codes; wide codes with a table of exactly
# 64 KiB; a table that does not fit (direct evaluation); bit-packed upload; m
# that does not fill the row's last load
LAYOUTS = [(32, 8, 256, False), (32, 16, 1024, False), (32, 32, 1024, False), (32, 8, 64, True), (30, 6, 256, False)]
BEYOND = [N, N + 77, (1 << 31) + 5, 1 << 40]


def _queries(rng, nq, d, metric):
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    return O.normalize_rows(qs) if metric == "cosine-dot" else qs


def _lists(rng, n, lengths):
    return [np.sort(rng.choice(n, int(L), replace=False)).astype(np.uint64) for L in lengths]


def _allow(lists, n):
    return [W.AllowList.from_ids(a[a < n], n) for a in lists]


def _same(a_ids, a_d, b_ids, b_d):
    assert a_ids.tolist() == b_ids.tolist()
    assert np.array_equal(a_d.view(np.uint32), b_d.view(np.uint32))


def _same_batch(a, b):
    assert a[2].tolist() == b[2].tolist()
    for i in range(len(a[2])):
        _same(a[0][i, : a[2][i]], a[1][i, : a[2][i]], b[0][i, : b[2][i]], b[1][i, : b[2][i]])


def _restated(ref, n, qs, lists):
    """Per query, every listed live row's (id, PQ distance) in (dist, id) order."""
    out = []
    for q, a in zip(qs, lists):
        a = a[a < n]
        oi, od, on, _ = ref.search_batch(q[None, :], max(len(a), 1), 0, allow=O.bits_from_ids(a, n), mode=1)
        order = np.lexsort((oi[0, : on[0]], od[0, : on[0]]))
        out.append((oi[0, : on[0]][order], od[0, : on[0]][order]))
    return out


def _pool(k):
    # lengths that cross k, a wave step, the stage, ks (64, 256, 1024) and a chunk
    return [0, 1, k - 1, k, k + 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025, 2049, 5999]


def _case1(ref, ix, d, metric, seed):
    """5 % of the rows tombstoned; per k one batch of NQ lists, every fifth
    with ids past the rows, and the restatement's rows of every list."""
    rng = np.random.default_rng(seed)
    dead = rng.choice(N, N // 20, replace=False)
    for t in dead:
        ref.add_tombstone(int(t))
    ix.add_tombstones(dead)
    ix.update_user_config(flat_search_cutoff=1 << 30)   # mode auto: every list is searched flat
    ix.set_pq_list_search(True)
    batches = {}
    for k in KS_ALL:
        pool = _pool(k)
        qs = _queries(rng, NQ, d, metric)
        lists = _lists(rng, N, [pool[(i + k) % len(pool)] for i in range(NQ)])
        full = _restated(ref, N, qs, lists)
        for i in range(0, NQ, 5):
            lists[i] = np.concatenate([lists[i], np.array(BEYOND, np.uint64)])
        batches[k] = (qs, lists, full)
    return dict(ref=ref, ix=ix, d=d, metric=metric, batches=batches)


@pytest.fixture(scope="module")
def pairs():
    """Per (metric, layout), built once when first asked for: 6,000
    standard-normal rows, an M 16 graph, the quantizer, case 1's batches."""
    made = {}

    def get(metric, layout):
        if (metric, layout) not in made:
            d, m, ks, use_bits = layout
            ref, ix, _, _, _ = _compressed_pair(N, d, m, ks, metric, use_bits=use_bits)
            made[(metric, layout)] = _case1(ref, ix, d, metric, 100 + m + ks)
        return made[(metric, layout)]

    yield get
    for fx in made.values():
        fx["ix"].close()
        fx["ref"].close()


def _check_case1(fx):
    """Every batch, split by the route's own rule: mode exact where 8 L < N,
    mode auto for the longer lists.  Ids, distance bits and counts equal the
    restatement; every query and every handed id is counted as sparse."""
    ix = fx["ix"]
    for k, (qs, lists, full) in fx["batches"].items():
        short = [i for i in range(NQ) if 8 * len(lists[i]) < N]
        long_ = [i for i in range(NQ) if 8 * len(lists[i]) >= N]
        assert short and long_
        for mode, sel in (("exact", short), ("auto", long_)):
            ids, ds, n = ix.search_batch_ids(qs[sel], k, [lists[i] for i in sel], mode=mode)
            st = ix.last_sparse_stats()
            for j, i in enumerate(sel):
                wi, wd = full[i][0][:k], full[i][1][:k]
                assert n[j] == len(wi), (k, i, len(lists[i]))
                _same(ids[j, : n[j]], ds[j, : n[j]], wi, wd)
            assert st == {"sparse_queries": len(sel), "sparse_ids": sum(lists[i].size for i in sel),
                          "bitmap_queries": 0}, (k, mode, st)


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda c: "d%d-m%d-ks%d-%s" % (c[0], c[1], c[2], "bits" if c[3] else "bytes"))
@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
def test_parity_against_the_restatement(pairs, monkeypatch, metric, layout):
    """Case 1: three metrics, five code layouts, k on both sides of a wave
    step and at the kernel's limit, list lengths across every boundary."""
    monkeypatch.delenv("WV_FLAT_IDS_PQ_LUT", raising=False)
    _check_case1(pairs(metric, layout))


@pytest.mark.parametrize("layout", LAYOUTS, ids=lambda c: "d%d-m%d-ks%d-%s" % (c[0], c[1], c[2], "bits" if c[3] else "bytes"))
def test_table_and_direct_evaluation_agree(pairs, monkeypatch, layout):
    """Case 2: the l2 batches with every workgroup evaluating directly, from
    the table wherever it fits, and by the default rule: all three equal the
    restatement."""
    fx = pairs("l2-squared", layout)
    for lut in ("0", "1", None):
        if lut is None:
            monkeypatch.delenv("WV_FLAT_IDS_PQ_LUT", raising=False)
        else:
            monkeypatch.setenv("WV_FLAT_IDS_PQ_LUT", lut)
        _check_case1(fx)


def test_ties_come_back_by_id():
    """Case 3: 64 distinct vectors, each stored 8 times (identical codes);
    lists of whole duplicate groups, k = 10.  Equal distances come back in
    ascending id order, as the restatement's rows ordered by (dist, id)."""
    rng = np.random.default_rng(7)
    groups, rep, d, m, ks, k = 64, 8, 16, 4, 16, 10
    base = np.repeat(rng.standard_normal((groups, d)).astype(np.float32), rep, axis=0)
    n = groups * rep
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
    ix.set_pq_list_search(True)
    qs = _queries(rng, NQ, d, "l2-squared")
    lists = []
    for i in range(NQ):
        g = np.sort(rng.choice(groups, 2 + i % 6, replace=False))   # 8 L < n: the list kernel in mode exact
        lists.append((g[:, None] * rep + np.arange(rep)[None, :]).reshape(-1).astype(np.uint64))
    ids, ds, cnt = ix.search_batch_ids(qs, k, lists, mode="exact")
    assert ix.last_sparse_stats()["sparse_queries"] == NQ
    ix.close()
    want = _restated(ref, n, qs, lists)
    ref.close()
    for i in range(NQ):
        assert cnt[i] == k and len(want[i][0]) == len(lists[i])
        _same(ids[i], ds[i], want[i][0][:k], want[i][1][:k])
        for v in np.unique(ds[i]):
            assert (np.diff(ids[i][ds[i] == v].astype(np.int64)) > 0).all()
        assert len(np.unique(ds[i])) < k   # the case does hold equal distances


def test_zero_distance_under_dot(pairs):
    """Case 4: an all-zero query in a dot batch: every distance is -0, as the
    restatement returns it."""
    fx = pairs("dot", LAYOUTS[0])
    ref, ix, d = fx["ref"], fx["ix"], fx["d"]
    rng = np.random.default_rng(4)
    qs = _queries(rng, 4, d, "dot")
    qs[2] = 0
    lists = _lists(rng, N, [300, 40, 500, 700])
    ids, ds, n = ix.search_batch_ids(qs, 10, lists, mode="exact")
    assert ix.last_sparse_stats()["sparse_queries"] == 4
    want = _restated(ref, N, qs, lists)
    for i in range(4):
        assert n[i] == 10
        _same(ids[i], ds[i], want[i][0][:10], want[i][1][:10])
    assert (ds[2].view(np.uint32) == 0x80000000).all()
    assert (want[2][1].view(np.uint32) == 0x80000000).all()


def test_on_against_off():
    """Case 5: one index, the same batches with the setting off, then on:
    identical results, and the stats show which queries changed route -- short
    lists do; lists of half the rows in mode exact, lists at or above the
    cutoff in mode auto (HNSW) and k = 257 do not.  The same on an index with
    an id base: ids come back offset."""
    n, d, nq = N, 32, 24
    ref, ix, base, cent, enc = _compressed_pair(n, d, 8, 256)
    ref.close()
    ix.update_user_config(flat_search_cutoff=50)
    rng = np.random.default_rng(15)
    qs = _queries(rng, nq, d, "l2-squared")
    short = _lists(rng, n, [1 + 29 * i for i in range(nq)])                        # 8 L < n
    half = _lists(rng, n, [n // 2] * nq)
    mixed = [half[i] if i % 3 == 0 else short[i] for i in range(nq)]
    cut = _lists(rng, n, [(0, 49, 50, 400)[i % 4] for i in range(nq)])
    runs = [("short", 10, short, "exact", nq), ("half", 10, half, "exact", 0), ("mixed", 10, mixed, "exact", nq - nq // 3),
            ("cutoff", 10, cut, "auto", nq // 2), ("k257", 257, short, "exact", 0)]
    got = {}
    for on in (False, True):
        ix.set_pq_list_search(on)
        for name, k, lists, mode, n_sparse in runs:
            got[(name, on)] = ix.search_batch_ids(qs, k, lists, mode=mode)
            st = ix.last_sparse_stats()
            want_sparse = n_sparse if on else 0
            assert (st["sparse_queries"], st["bitmap_queries"]) == (want_sparse, nq - want_sparse), (name, on, st)
    for name, k, lists, mode, _ in runs:
        _same_batch(got[(name, False)], got[(name, True)])
        _same_batch(got[(name, True)], ix.search_batch(qs, k, allow=_allow(lists, n), mode=mode))
    ix.close()
    sh = W.GPUVectorIndex(d, "l2-squared", capacity=n, id_base=64000)
    sh.upload_vectors(base)
    sh.set_pq(cent)
    sh.upload_pq_codes(enc)
    sh.set_compressed(True)
    off = sh.search_batch_ids(qs, 10, short, mode="exact")
    assert sh.last_sparse_stats()["sparse_queries"] == 0
    sh.set_pq_list_search(True)
    on = sh.search_batch_ids(qs, 10, short, mode="exact")
    assert sh.last_sparse_stats() == {"sparse_queries": nq, "sparse_ids": sum(a.size for a in short), "bitmap_queries": 0}
    sh.close()
    _same_batch(off, on)
    _same_batch(on, (got[("short", True)][0] + np.uint64(64000), got[("short", True)][1], got[("short", True)][2]))
    assert (on[0][:, 0] >= 64000).all()


def test_added_rows_are_listed_rows():
    """Case 6: rows added after compression are encoded on the device (KMeans
    encoder): a list that names three of them gets them back, equal to the
    restatement over the grown base."""
    n0, n1, d, m, ks, k = 3000, 3010, 16, 4, 256, 20
    rng = np.random.default_rng(21)
    base = rng.standard_normal((n1, d)).astype(np.float32)
    cent = _centroids(base, m, ks, 21)
    enc = O.pq_encode_kmeans(base, cent)
    ref = O.Index(d, "l2-squared", 16, 64, capacity=n1, seed=21)
    ref.add_batch(base, threads=8)
    ref.compress(cent, enc)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n1)
    ix.upload_vectors(base[:n0])
    ix.set_pq(cent, encoder="kmeans")
    ix.upload_pq_codes(enc[:n0])
    ix.set_compressed(True)
    ix.set_pq_list_search(True)
    ix.add(np.arange(n0, n1), base[n0:])
    lists = []
    for i in range(NQ):
        a = np.concatenate([rng.choice(n0, 17, replace=False), n0 + rng.choice(n1 - n0, 3, replace=False)])
        lists.append(np.sort(a).astype(np.uint64))
    qs = _queries(rng, NQ, d, "l2-squared")
    got = ix.search_batch_ids(qs, k, lists, mode="auto")
    assert ix.last_sparse_stats()["sparse_queries"] == NQ
    ix.close()
    want = _restated(ref, n1, qs, lists)
    ref.close()
    for i in range(NQ):
        assert got[2][i] == k
        _same(got[0][i], got[1][i], want[i][0], want[i][1])
        assert (got[0][i] >= n0).sum() == 3


def test_batcher_sends_id_lists(monkeypatch):
    """Case 7: 32 threads with lists of their own through Batcher.search_ids
    on the compressed index with the setting on: every answer equals
    search_by_vector over the same list as a bitmap, and the list kernel ran."""
    monkeypatch.delenv("WV_BATCHER_IDS", raising=False)
    n, d, nt, k = N, 32, 32, 10
    ref, ix, _, _, _ = _compressed_pair(n, d, 8, 256)
    ref.close()
    rng = np.random.default_rng(12)
    qs = _queries(rng, nt, d, "l2-squared")
    lists = _lists(rng, n, [20 + 37 * t for t in range(nt)])
    want = [ix.search_by_vector(qs[t], k, allow=W.AllowList.from_ids(lists[t], n)) for t in range(nt)]
    ix.set_pq_list_search(True)
    b = W.Batcher(ix, max_batch=nt, max_wait_us=5_000_000)
    got = [None] * nt

    def worker(t):
        got[t] = b.search_ids(qs[t], k, lists[t])

    th = [threading.Thread(target=worker, args=(t,)) for t in range(nt)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    b.close()
    st = ix.last_sparse_stats()
    ix.close()
    for t in range(nt):
        _same(got[t][0], got[t][1], want[t][0], want[t][1])
    assert st["sparse_queries"] > 0, st


def test_default_is_the_bitmap_route():
    """Case 8: without the setter call a compressed index sends every query
    down the bitmap route."""
    n, d = 3000, 32
    ref, ix, _, _, _ = _compressed_pair(n, d, 8, 256)
    ref.close()
    rng = np.random.default_rng(8)
    qs = _queries(rng, 8, d, "l2-squared")
    lists = _lists(rng, n, [10 + 20 * i for i in range(8)])
    ix.search_batch_ids(qs, 10, lists, mode="exact")
    assert ix.last_sparse_stats() == {"sparse_queries": 0, "sparse_ids": 0, "bitmap_queries": 8}
    ix.close()
