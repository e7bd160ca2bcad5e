"""SearchByVectorDistance over per-query allow lists given as ids
(wv_search_by_vector_distance_batch_ids): the threshold pass that walks the
lists, its variable segments and query chunks, HNSW round 1 over bitmap rows
scattered on the device, the overflow to the per-query path and the batcher's
route.

The yardstick is never the new code: the bitmap batch call over AllowLists of
the same ids, the single-query call, or the CPU restatement.  Bar: ids,
distance bits and the counts n identical (up to the order among equal
distances against the restatement).  Runs on an MI355X (-m gpu).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from helpers import same_tie_aware

pytestmark = pytest.mark.gpu

METRICS = {"l2-squared": O.L2, "dot": O.DOT, "cosine-dot": O.COSINE}
NIL = np.uint32(0xFFFFFFFF)


def _data(rng, n, nq, d, metric):
    base = rng.random((n, d), dtype=np.float32)
    qs = rng.random((nq, d), dtype=np.float32)
    if metric != "l2-squared":
        base -= 0.5
        qs -= 0.5
    return base, qs


def _lists(rng, n, lengths):
    return [np.sort(rng.choice(n, int(L), replace=False)).astype(np.uint64) for L in lengths]


def _allow(lists, nbits):
    return [W.AllowList.from_ids(a[a < nbits], nbits) for a in lists]


def _dist_table(metric, base, qs):
    """dist[q][row] of every row, the restatement's bits."""
    b = O.normalize_rows(base) if metric == "cosine-dot" else base
    q = O.normalize_rows(qs) if metric == "cosine-dot" else qs
    n = base.shape[0]
    oi, od, on = O.flat_scan(METRICS[metric], b, q, n)
    assert (on == n).all()
    table = np.empty((len(qs), n), np.float32)
    for i in range(len(qs)):
        table[i, oi[i].astype(np.int64)] = od[i]
    return table


def _targets(table, lists, ranks, live=None):
    """Query i's target: the distance of its own listed (live) row at rank
    ranks[i] (clamped to its last row; None: below its nearest row)."""
    out = np.zeros(len(lists), np.float32)
    for i, a in enumerate(lists):
        a = a[a < table.shape[1]].astype(np.int64)
        if live is not None:
            a = a[live[a]]
        if a.size == 0:
            out[i] = 1.0
            continue
        d = np.sort(table[i, a])
        out[i] = d[0] - np.float32(1.0) if ranks[i] is None else d[min(ranks[i], a.size - 1)]
    return out


def _assert_same(got, got_n, want, want_n):
    assert np.asarray(got_n).tolist() == np.asarray(want_n).tolist()
    for i, ((gi, gd), (wi, wd)) in enumerate(zip(got, want)):
        assert gi.tolist() == wi.tolist(), i
        assert np.array_equal(gd.view(np.uint32), wd.view(np.uint32)), i


def _flat_restatement(base, metric="l2-squared"):
    """The restatement over a flat index: every row a level-0 node without
    links (flatSearch skips nil nodes, flat_search.go:35-39)."""
    n, d = base.shape
    ref = O.Index(d, metric, 16, 64, capacity=n)
    ref.import_graph(base, dict(n=n, entrypoint=0, max_level=0, levels=np.zeros(n, np.int8),
                                layer0=np.full((n, 1), NIL, np.uint32), upper_row=np.full(n, NIL, np.uint32),
                                upper=np.zeros((1, 1, 1), np.uint32)))
    ref.set_search_config(flat_search_cutoff=10**9)
    return ref


LENGTHS = [0, 1, 63, 64, 65, 255, 256, 257, 513, 1025, 4000]
RANKS = [0, 20, 99, 100, 150, 1099, 1500, None]


@pytest.mark.parametrize("dim", [1, 30, 32])
@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
def test_flat_index_list_length_edges(metric, dim):
    """One batch of 88 queries: every list length that crosses a wave step, a
    workgroup step or a chunk, with every target rank (a rank past a list's
    end is its last row).  Equal to the bitmap batch route: ids, distance bits
    and counts; every query a list query."""
    n = 4000
    rng = np.random.default_rng(500 + dim)
    nq = len(LENGTHS) * len(RANKS)
    base, qs = _data(rng, n, nq, dim, metric)
    lists = _lists(rng, n, [LENGTHS[i // len(RANKS)] for i in range(nq)])
    targets = _targets(_dist_table(metric, base, qs), lists, [RANKS[i % len(RANKS)] for i in range(nq)])
    ix = W.GPUVectorIndex(dim, metric, capacity=n)
    ix.upload_vectors(base)
    allow = _allow(lists, n)
    for max_limit in (-1, 150, 1100):
        for cap in (4096, 120):
            want, want_n = ix.search_by_vector_distance_batch(qs, targets, max_limit, allow=allow, cap=cap)
            got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, max_limit, cap=cap)
            _assert_same(got, got_n, want, want_n)
            st = ix.last_sbd_ids_stats()
            assert st == {"list_queries": nq, "list_ids": sum(a.size for a in lists), "hnsw_round1_queries": 0,
                          "legacy_queries": 0}, st
    assert got_n.max() > 120 and got_n.min() == 0   # (the shapes do reach past the caller's cap, and an empty answer)
    ix.close()


def test_skipped_and_excluded_ids():
    """Ids past the rows, past the capacity and past 2^31 are skipped;
    tombstoned rows and rows never uploaded (a hole below n_rows, and the
    capacity past the rows) are excluded: none comes back and n equals the
    bitmap route's, on an index with an id base."""
    cap_rows, d, id_base = 6000, 20, 10000
    rng = np.random.default_rng(61)
    base, qs = _data(rng, 5000, 24, d, "l2-squared")
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=cap_rows, id_base=id_base)
    ix.upload_vectors(base[:4000])
    ix.upload_vectors(base[4500:], first_id=4500)   # rows 4000..4499 have no vector; n_rows = 5000
    dead = rng.choice(4000, 400, replace=False)
    ix.add_tombstones(dead)
    live = np.zeros(5000, bool)
    live[:4000] = True
    live[4500:] = True
    live[dead] = False
    lists = _lists(rng, cap_rows, [40 + 90 * i for i in range(24)])
    for i in range(24):
        extra = [cap_rows, cap_rows + 77, (1 << 31) - 1, 1 << 31, (1 << 31) + 5, 1 << 40][: 1 + i % 6]
        lists[i] = np.concatenate([lists[i], np.array(extra, np.uint64)])
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [(5, 99, 150, 1200)[i % 4] for i in range(24)], live)
    want, want_n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=_allow(lists, cap_rows), cap=4096)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=4096)
    _assert_same(got, got_n, want, want_n)
    assert ix.last_sbd_ids_stats()["legacy_queries"] == 0
    for i, (gi, _) in enumerate(got):
        loc = gi.astype(np.int64) - id_base
        assert got_n[i] > 0 and (loc >= 0).all() and (loc < 5000).all()
        assert live[loc].all()
        assert np.isin(loc, lists[i][lists[i] < 5000].astype(np.int64)).all()
    ix.close()


@pytest.fixture(scope="module")
def graph6000():
    n, d = 6000, 24
    rng = np.random.default_rng(33)
    base, qs = _data(rng, n, 24, d, "l2-squared")
    ref = O.Index(d, "l2-squared", 16, 64, capacity=n, seed=3)
    ref.add_batch(base, threads=8)
    g = ref.export_graph()
    ref.close()
    return base, qs, g, _dist_table("l2-squared", base, qs)


def test_hnsw_round_one(graph6000):
    """Lists of about 300 ids (below the cutoff: flat) and about 3000 ids
    (HNSW round 1 over a bitmap row scattered on the device) alternate in one
    batch; targets stop in round 1, 2 and 3.  Bit-identical to the bitmap
    batch route; the stats report the HNSW queries; then all HNSW with
    forbid_flat."""
    base, qs, g, table = graph6000
    n, nq = base.shape[0], len(qs)
    ix = W.GPUVectorIndex(base.shape[1], "l2-squared", capacity=n, max_connections=16, flat_search_cutoff=1000)
    ix.upload_vectors(base)
    ix.upload_graph(g)
    rng = np.random.default_rng(34)
    lists = _lists(rng, n, [(2990 + i) if i % 2 else (290 + i) for i in range(nq)])
    # rounds: 100, 1100, 11100 entries (a 300-id list ends in round 2)
    targets = _targets(table, lists, [(20, 20, 150, 150, 250, 1500)[i % 6] for i in range(nq)])
    allow = _allow(lists, n)
    for forbid_flat, n_hnsw in ((0, nq // 2), (1, nq)):
        ix.update_user_config(forbid_flat=forbid_flat)
        for max_limit in (-1, 1100):
            want, want_n = ix.search_by_vector_distance_batch(qs, targets, max_limit, allow=allow, cap=4096)
            got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, max_limit, cap=4096)
            _assert_same(got, got_n, want, want_n)
            st = ix.last_sbd_ids_stats()
            assert (st["list_queries"], st["hnsw_round1_queries"], st["legacy_queries"]) == (nq, n_hnsw, 0), st
            # (unlimited: a third round did run; maxLimit 1100: it did not)
            assert got_n.max() == (1501 if max_limit < 0 else 1100)
    ix.close()


def test_overflow_goes_to_the_per_query_path(monkeypatch):
    """WV_SBD_CAP=128: a query with about 400 rows within its target outgrows
    its segment and is answered by the single-query path; its neighbour in the
    batch with 100 rows within stays on the list route."""
    monkeypatch.setenv("WV_SBD_CAP", "128")
    n, d = 4000, 16
    rng = np.random.default_rng(71)
    base, qs = _data(rng, n, 2, d, "l2-squared")
    lists = _lists(rng, n, [1000, 1000])
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [399, 99])
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=4096)
    st = ix.last_sbd_ids_stats()
    assert (st["list_queries"], st["legacy_queries"]) == (1, 1), st
    assert got_n.tolist() == [400, 100]
    for i in range(2):
        wi, wd = ix.search_by_vector_distance(qs[i], float(targets[i]), -1, allow=W.AllowList.from_ids(lists[i], n),
                                              cap=4096)
        assert got[i][0].tolist() == wi.tolist()
        assert np.array_equal(got[i][1].view(np.uint32), wd.view(np.uint32))
    ix.close()


def test_query_chunks(monkeypatch):
    """WV_SBD_IDS_MAX_ENTRIES=2048: 12 queries with 500-id segments run as
    three chunks of queries; the answers are the unchunked call's and the
    bitmap route's."""
    n, d, nq = 4000, 32, 12
    rng = np.random.default_rng(81)
    base, qs = _data(rng, n, nq, d, "l2-squared")
    lists = _lists(rng, n, [500] * nq)
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [(20, 150, 450, 99)[i % 4] for i in range(nq)])
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    monkeypatch.delenv("WV_SBD_IDS_MAX_ENTRIES", raising=False)
    whole, whole_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=1024)
    bitmap, bitmap_n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=_allow(lists, n), cap=1024)
    monkeypatch.setenv("WV_SBD_IDS_MAX_ENTRIES", "2048")
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=1024)
    assert ix.last_sbd_ids_stats()["list_queries"] == nq
    _assert_same(got, got_n, whole, whole_n)
    _assert_same(got, got_n, bitmap, bitmap_n)
    assert sorted(set(got_n.tolist())) == [21, 100, 151, 451]
    ix.close()


def test_long_segments():
    """66 lists of 17,000 ids: every segment is WV_SBD_CAP (16384) keys long
    and together they pass the 8 MiB that one copy fetches, so each kept
    prefix is fetched on its own.  Equal to the bitmap route."""
    n, d, nq = 20000, 8, 66
    rng = np.random.default_rng(85)
    base, qs = _data(rng, n, nq, d, "l2-squared")
    lists = _lists(rng, n, [17000] * nq)
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [(20, 150, 1500)[i % 3] for i in range(nq)])
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    want, want_n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=_allow(lists, n), cap=2048)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=2048)
    _assert_same(got, got_n, want, want_n)
    assert ix.last_sbd_ids_stats()["list_queries"] == nq
    assert got_n.min() >= 21 and got_n.max() >= 1501   # (rounds 1 to 3)
    ix.close()


def test_wide_rows():
    """D = 1500, past the bitmap scan's 1024-float query buffer: the list
    route (the query row in dynamic LDS) against the single-query call and
    the restatement."""
    n, d, nq = 2000, 1500, 4
    rng = np.random.default_rng(91)
    base, qs = _data(rng, n, nq, d, "l2-squared")
    lists = _lists(rng, n, [700] * nq)
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [5, 99, 150, 650])
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, flat_search_cutoff=10**9)
    ix.upload_vectors(base)
    ref = _flat_restatement(base)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=1024)
    assert ix.last_sbd_ids_stats()["legacy_queries"] == 0
    for i in range(nq):
        si, sd = ix.search_by_vector_distance(qs[i], float(targets[i]), -1, allow=W.AllowList.from_ids(lists[i], n),
                                              cap=1024)
        oi, od = ref.search_by_vector_distance(qs[i], float(targets[i]), -1, allow=O.bits_from_ids(lists[i], n))
        same_tie_aware(got[i][0], got[i][1], si, sd)
        same_tie_aware(got[i][0], got[i][1], oi, od)
        assert got_n[i] == len(si) == len(oi)
    assert got_n.tolist() == [6, 100, 151, 651]
    ix.close()
    ref.close()


def test_equal_to_the_restatement():
    """Flat index, 20,000 x 64 uniform rows, lists of a random 30 % of the
    ids: the restatement's SearchByVectorDistance on each query, up to the
    order among equal distances, with equal counts."""
    n, d, nq = 20000, 64, 6
    rng = np.random.default_rng(101)
    base, qs = _data(rng, n, nq, d, "l2-squared")
    lists = [np.nonzero(rng.random(n) < 0.3)[0].astype(np.uint64) for _ in range(nq)]
    targets = _targets(_dist_table("l2-squared", base, qs), lists, [(5, 99, 150, 1200)[i % 4] for i in range(nq)])
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, flat_search_cutoff=10**9)
    ix.upload_vectors(base)
    ref = _flat_restatement(base)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=8192)
    for i in range(nq):
        oi, od = ref.search_by_vector_distance(qs[i], float(targets[i]), -1, allow=O.bits_from_ids(lists[i], n))
        same_tie_aware(got[i][0], got[i][1], oi, od)
        assert got_n[i] == len(oi)
    ix.close()
    ref.close()


@pytest.mark.parametrize("send_ids", [None, "0"])
def test_batcher_sends_distance_groups_as_ids(monkeypatch, send_ids):
    """16 threads through Batcher.search_distance_ids: first all with one
    list (one shared bitmap: the list route is not taken), then each with a
    list of its own (the list route; WV_BATCHER_IDS=0: bitmap rows, stats
    untouched).  Every thread gets the answer of its own single-query call."""
    if send_ids is None:
        monkeypatch.delenv("WV_BATCHER_IDS", raising=False)
    else:
        monkeypatch.setenv("WV_BATCHER_IDS", send_ids)
    n, d, nt = 4000, 32, 16
    rng = np.random.default_rng(111)
    base, qs = _data(rng, n, nt, d, "l2-squared")
    own = _lists(rng, n, [300 + 40 * t for t in range(nt)])
    rounds = [[own[0]] * nt, own]
    table = _dist_table("l2-squared", base, qs)
    targets = [_targets(table, ls, [(5, 99, 150, 250)[t % 4] for t in range(nt)]) for ls in rounds]
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    want = [[ix.search_by_vector_distance(qs[t], float(targets[r][t]), -1, allow=W.AllowList.from_ids(ls[t], n),
                                          cap=4096) for t in range(nt)] for r, ls in enumerate(rounds)]
    zero = {"list_queries": 0, "list_ids": 0, "hnsw_round1_queries": 0, "legacy_queries": 0}
    b = W.Batcher(ix, max_batch=nt, max_wait_us=5_000_000)
    stats = []
    for r, ls in enumerate(rounds):
        got = [None] * nt

        def worker(t):
            got[t] = b.search_distance_ids(qs[t], float(targets[r][t]), -1, ls[t], cap=4096)

        th = [threading.Thread(target=worker, args=(t,)) for t in range(nt)]
        for t in th:
            t.start()
        for t in th:
            t.join(120)
        stats.append(ix.last_sbd_ids_stats())
        for t in range(nt):
            assert got[t][0].tolist() == want[r][t][0].tolist(), (r, t)
            assert np.array_equal(got[t][1].view(np.uint32), want[r][t][1].view(np.uint32)), (r, t)
    b.close()
    ix.close()
    assert stats[0] == zero, stats
    if send_ids is None:
        assert stats[1]["list_queries"] > 0 and stats[1]["legacy_queries"] == 0, stats
    else:
        assert stats[1] == zero, stats


def test_bad_lists_on_a_live_index():
    """Ids that do not ascend, offsets that decrease or do not start at 0:
    WV_EINVAL with their messages, and the index answers the next call."""
    n, d = 1000, 8
    rng = np.random.default_rng(121)
    base, qs = _data(rng, n, 2, d, "l2-squared")
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    q = np.ascontiguousarray(qs)
    t = np.full(2, 100.0, np.float32)
    out_i, out_d, out_n = np.zeros((2, 8), np.uint64), np.zeros((2, 8), np.float32), np.zeros(2, np.int64)

    def call(ids, off):
        ids, off = np.asarray(ids, np.uint64), np.asarray(off, np.uint64)
        vp = lambda a: C.c_void_p(a.ctypes.data)   # noqa: E731
        return W.lib().wv_search_by_vector_distance_batch_ids(ix._h, vp(q), 2, vp(t), -1, vp(ids), vp(off), vp(out_i),
                                                              vp(out_d), 8, vp(out_n))

    assert call([1, 2, 3, 4], [0, 2, 4]) == 0
    assert out_n.tolist() == [2, 2] and sorted(out_i[0, :2].tolist()) == [1, 2]
    assert call([1, 2, 3, 4], [1, 2, 4]) == 1
    assert b"allow_offsets[0]" in W.lib().wv_last_error()
    assert call([1, 2, 3, 4], [0, 3, 2]) == 1
    assert b"decrease" in W.lib().wv_last_error()
    assert call([2, 1, 3, 4], [0, 2, 4]) == 1
    assert b"ascending" in W.lib().wv_last_error()
    assert call([1, 1, 3, 4], [0, 2, 4]) == 1
    assert b"ascending" in W.lib().wv_last_error()
    # ascending is per query, an empty range allows nothing, and the index is still usable
    assert call([5, 9, 3, 4], [0, 2, 4]) == 0
    assert call([5, 9], [0, 2, 2]) == 0
    assert out_n.tolist() == [2, 0]
    with pytest.raises(W.WvError):
        ix.search_by_vector_distance_batch_ids(qs, t, [np.array([1, 2], np.uint64)])
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, t, [np.array([7], np.uint64), np.array([8, 9], np.uint64)])
    assert got_n.tolist() == [1, 2] and got[1][0].tolist() in ([8, 9], [9, 8])
    ix.close()
