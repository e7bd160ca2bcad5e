"""SearchByVectorDistance on a PQ-compressed index, batched on the device: the
threshold passes over the codes (wv_sbd_pq.hip: scan and list pass, the lookup
table and the direct evaluation), their routing in both batch entry points,
the overflow to the per-query path, query chunks, added rows and the batcher.

The yardstick is never the new code: the CPU restatement's
SearchByVectorDistance, or the per-query call on the same index (whose rounds
are single searches).  Bar: ids, distance bits and counts identical.  Runs on
an MI355X (-m gpu).
"""
import ctypes as C
import threading

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from test_pq import _centroids, _compressed_pair

pytestmark = pytest.mark.gpu

N, D, M, KS = 6000, 32, 8, 256
# list lengths that cross a wave step, a workgroup step, ks (the table is
# built from ks ids a chunk) and a chunk; with each the ranks of its target
# that the list is long enough for: both sides of the 100 and 1100 round limits
LENGTHS = {0: [None], 1: [1], 63: [40], 64: [40], 65: [40], 255: [40, 100, 101], 256: [40, 100, 101],
           257: [40, 100, 101], 2049: [40, 100, 101, 1100, 1101], 5999: [40, 100, 101, 1100, 1101, 2500]}
BEYOND = [N, N + 77, (1 << 31) - 1, 1 << 31, (1 << 31) + 5, 1 << 40]


def _queries(rng, nq, d, metric):
    qs = rng.standard_normal((nq, d)).astype(np.float32)
    return O.normalize_rows(qs) if metric == "cosine-dot" else qs


def _lists(rng, n, lengths):
    return [np.sort(rng.choice(n, int(L), replace=False)).astype(np.uint64) for L in lengths]


def _allow(lists, n):
    return [W.AllowList.from_ids(a[a < n], n) for a in lists]


def _sorted_dists(ref, q, words, k):
    """The restatement's PQ distances of the allowed live rows, ascending (flat search)."""
    _, od, on, _ = ref.search_batch(q[None, :], k, 0, allow=words, mode=1)
    return np.sort(od[0, : on[0]])


def _restated(ref, ix, n, d, metric, seed, lengths=LENGTHS):
    """Case 1's batch on a compressed pair, 5 % of its rows tombstoned: one
    query per (list length, target rank), ids past the rows in every third
    list, and the restatement's answer per query in (dist, id) order."""
    rng = np.random.default_rng(seed)
    dead = rng.choice(n, n // 20, replace=False)
    for t in dead:
        ref.add_tombstone(int(t))
    ix.add_tombstones(dead)
    pairs = [(L, r) for L, ranks in lengths.items() for r in ranks]
    assert len(pairs) <= 48
    nq = len(pairs)
    qs = _queries(rng, nq, d, metric)
    lists = _lists(rng, n, [min(L, n) for L, _ in pairs])
    targets = np.ones(nq, np.float32)
    want, within = [], []
    for i, (L, rank) in enumerate(pairs):
        words = O.bits_from_ids(lists[i], n)
        ds = _sorted_dists(ref, qs[i], words, max(L, 1)) if rank is not None else []
        within.append(min(rank, len(ds)) if len(ds) else None)
        if len(ds):
            targets[i] = ds[within[i] - 1]
        oi, od = ref.search_by_vector_distance(qs[i], float(targets[i]), -1, allow=words, cap=max(L, 1))
        order = np.lexsort((oi, od))
        want.append((oi[order], od[order]))
        if i % 3 == 0:
            lists[i] = np.concatenate([lists[i], np.array(BEYOND[: 1 + i % 6], np.uint64)])
    return dict(ref=ref, ix=ix, n=n, d=d, metric=metric, qs=qs, lists=lists, targets=targets, want=want, pairs=pairs,
                within=within)


@pytest.fixture(scope="module")
def pairs():
    """Per metric, built once when first asked for: 6,000 x 32 standard-normal
    rows, an M 16 graph, 8 segments of 256 centroids -- two scan row blocks
    (the second partial), lists on both sides of ks, within-target sets on
    both sides of the 100 and 1100 round limits -- with case 1's batch."""
    made = {}

    def get(metric):
        if metric not in made:
            ref, ix, _, _, _ = _compressed_pair(N, D, M, KS, metric)
            made[metric] = _restated(ref, ix, N, D, metric, 40)
        return made[metric]

    yield get
    for fx in made.values():
        fx["ix"].close()
        fx["ref"].close()


@pytest.fixture
def l2pair(pairs):
    return pairs("l2-squared")


def _assert_same(got, got_n, want, want_n=None):
    if want_n is None:
        want_n = [len(w[0]) for w in want]
    assert np.asarray(got_n).tolist() == np.asarray(want_n).tolist()
    for i, ((gi, gd), (wi, wd)) in enumerate(zip(got, want)):
        assert gi.tolist() == wi[: len(gi)].tolist(), i
        assert np.array_equal(gd.view(np.uint32), wd[: len(gd)].view(np.uint32)), i


def _both_routes(fx, cap=8192):
    """Case 1 through both entry points against the restatement, with the stats."""
    ix, n, nq = fx["ix"], fx["n"], len(fx["qs"])
    got, got_n = ix.search_by_vector_distance_batch(fx["qs"], fx["targets"], -1, allow=_allow(fx["lists"], n), cap=cap)
    _assert_same(got, got_n, fx["want"])
    st = ix.last_sbd_stats()
    assert st == {"pass_queries": nq, "hnsw_round1_queries": 0, "legacy_queries": 0}, st
    got, got_n = ix.search_by_vector_distance_batch_ids(fx["qs"], fx["targets"], fx["lists"], -1, cap=cap)
    _assert_same(got, got_n, fx["want"])
    st = ix.last_sbd_ids_stats()
    assert (st["list_queries"], st["hnsw_round1_queries"], st["legacy_queries"]) == (nq, 0, 0), st
    return got, got_n


@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
def test_flat_queries_against_the_restatement(pairs, monkeypatch, metric):
    """Case 1, three metrics: every list is below the flat-search cutoff, so
    all rounds are exact.  The restatement returns exactly the listed live
    rows within the target; the GPU's ids, distance bits and counts equal it
    on the bitmap route and on the id-list route, no query on the per-query
    path."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    pair = pairs(metric)
    for w, within in zip(pair["want"], pair["within"]):
        # the restatement returns the rows within the target: as many as the rank (one more on a tie)
        assert len(w[0]) in ((0,) if within is None else (within, within + 1)), (len(w[0]), within)
    _, got_n = _both_routes(pair)
    assert got_n.min() == 0 and got_n.max() >= 2500


def test_stats_accept_null_outputs(l2pair):
    ix = l2pair["ix"]
    assert W.lib().wv_last_sbd_stats(ix._h, None, None, None) == 0
    a = C.c_uint64(99)
    assert W.lib().wv_last_sbd_stats(ix._h, None, None, C.byref(a)) == 0 and a.value != 99


def _per_query(ix, qs, targets, max_limit, allows, cap):
    out, n = [], []
    for i in range(len(qs)):
        a = allows if allows is None or isinstance(allows, W.AllowList) else allows[i]
        big = ix.search_by_vector_distance(qs[i], float(targets[i]), max_limit, allow=a, cap=1 << 15)
        n.append(len(big[0]))
        out.append((big[0][:cap], big[1][:cap]))
    return out, n


RANKS2 = [40, 100, 101, 1100, 1101, 2500]


def _targets_over(fx, qs, allows):
    """Targets at RANKS2 of each query's PQ distances over its allowed rows (the rank clamped to their number)."""
    t = np.zeros(len(qs), np.float32)
    for i in range(len(qs)):
        a = allows if allows is None or isinstance(allows, W.AllowList) else allows[i]
        ds = _sorted_dists(fx["ref"], qs[i], None if a is None else a.words, fx["n"])
        t[i] = ds[min(RANKS2[i % 6], len(ds)) - 1]
    return t


@pytest.mark.parametrize("case", ["no filter", "shared bitmap", "per-query bitmaps", "forbid_flat"])
def test_equal_to_the_per_query_path(l2pair, monkeypatch, case):
    """Case 2 on the bitmap entry point: round 1 from the HNSW search (no
    filter; long lists; forbid_flat) or flat, every maxLimit that ends the
    deepening in a different round, the caller's cap below the count.  The
    expectation is the single-query call per query; the batch with
    WV_SBD_PQ=0 (the per-query route of before) must give the same."""
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    fx, ix, n = l2pair, l2pair["ix"], l2pair["n"]
    rng = np.random.default_rng(52)
    nq = 12
    qs = _queries(rng, nq, fx["d"], fx["metric"])
    cutoff, forbid = 40000, 0
    if case == "no filter":
        allows, n_hnsw = None, nq
    elif case == "shared bitmap":
        allows, n_hnsw, cutoff = W.AllowList.from_ids(np.nonzero(rng.random(n) < 0.6)[0], n), nq, 1000
    elif case == "per-query bitmaps":
        # lists of about 600 (flat) and 3600 ids (HNSW round 1) alternate
        allows = [W.AllowList.from_ids(np.nonzero(rng.random(n) < (0.6 if i % 2 else 0.1))[0], n) for i in range(nq)]
        n_hnsw, cutoff = nq // 2, 1000
    else:
        allows = [W.AllowList.from_ids(np.nonzero(rng.random(n) < 0.5)[0], n) for i in range(nq)]
        n_hnsw, forbid = nq, 1
    targets = _targets_over(fx, qs, allows)
    ix.update_user_config(flat_search_cutoff=cutoff, forbid_flat=forbid)
    try:
        for max_limit in (-1, 100, 1100, 1200):
            for cap in (4096, 50):
                monkeypatch.delenv("WV_SBD_PQ", raising=False)
                want, want_n = _per_query(ix, qs, targets, max_limit, allows, cap)
                got, got_n = ix.search_by_vector_distance_batch(qs, targets, max_limit, allow=allows, cap=cap)
                _assert_same(got, got_n, want, want_n)
                st = ix.last_sbd_stats()
                assert st == {"pass_queries": nq, "hnsw_round1_queries": n_hnsw, "legacy_queries": 0}, st
                monkeypatch.setenv("WV_SBD_PQ", "0")
                old, old_n = ix.search_by_vector_distance_batch(qs, targets, max_limit, allow=allows, cap=cap)
                _assert_same(old, old_n, want, want_n)
                assert ix.last_sbd_stats()["legacy_queries"] == nq
            if max_limit == -1:
                assert max(want_n) > 1100 and min(want_n) <= 100   # (rounds 1 to 3 did run)
    finally:
        ix.update_user_config(flat_search_cutoff=40000, forbid_flat=0)


def test_single_query_batches(l2pair, monkeypatch):
    """A batch of one unfiltered query runs its HNSW round 1 first and the
    pass only when round 1 lets the deepening go on: targets that end it in
    round 1 (40 rows within; maxLimit 100) and that reach rounds 2 and 3,
    each equal to the per-query call."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    fx, ix = l2pair, l2pair["ix"]
    qs = _queries(np.random.default_rng(54), 6, fx["d"], fx["metric"])
    targets = _targets_over(fx, qs, None)
    counts = []
    for i in range(len(qs)):
        for max_limit in (-1, 100):
            want, want_n = _per_query(ix, qs[i:i + 1], targets[i:i + 1], max_limit, None, 4096)
            got, got_n = ix.search_by_vector_distance_batch(qs[i:i + 1], targets[i:i + 1], max_limit, cap=4096)
            _assert_same(got, got_n, want, want_n)
            assert ix.last_sbd_stats() == {"pass_queries": 1, "hnsw_round1_queries": 1, "legacy_queries": 0}
            counts.append(int(got_n[0]))
    assert min(counts) <= 100 and max(counts) > 1100, counts


def test_id_lists_around_the_cutoff(l2pair, monkeypatch):
    """Case 2 on the id-list entry point with flat_search_cutoff 50: lists of
    30 to 70 ids (flat below 50, HNSW round 1 from 50) and lists of 3000 ids
    with deep targets in one batch, equal to the per-query call."""
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    fx, ix, n = l2pair, l2pair["ix"], l2pair["n"]
    rng = np.random.default_rng(53)
    lengths = [30, 49, 50, 51, 70, 3000, 48, 52, 3000, 3000, 3000, 3000]
    nq = len(lengths)
    qs = _queries(rng, nq, fx["d"], fx["metric"])
    lists = _lists(rng, n, lengths)
    allows = _allow(lists, n)
    targets = _targets_over(fx, qs, allows)
    ix.update_user_config(flat_search_cutoff=50)
    try:
        for max_limit in (-1, 100, 1100, 1200):
            for cap in (4096, 50):
                monkeypatch.delenv("WV_SBD_PQ", raising=False)
                want, want_n = _per_query(ix, qs, targets, max_limit, allows, cap)
                got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, max_limit, cap=cap)
                _assert_same(got, got_n, want, want_n)
                st = ix.last_sbd_ids_stats()
                assert (st["list_queries"], st["hnsw_round1_queries"], st["legacy_queries"]) == (nq, 9, 0), st
                monkeypatch.setenv("WV_SBD_PQ", "0")
                old, old_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, max_limit, cap=cap)
                _assert_same(old, old_n, want, want_n)
                assert ix.last_sbd_ids_stats()["legacy_queries"] == nq
    finally:
        ix.update_user_config(flat_search_cutoff=40000)


@pytest.mark.parametrize("lut", ["0", "1"])
def test_table_and_direct_variants_agree(l2pair, monkeypatch, lut):
    """Case 3: case 1's l2 batch with every workgroup evaluating directly
    (WV_SBD_PQ_LUT=0) and with every workgroup building the table (=1, also
    for chunks shorter than ks): the restatement's answer both times."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.setenv("WV_SBD_PQ_LUT", lut)
    _both_routes(l2pair)


@pytest.mark.parametrize("d,m,ks,use_bits", [(32, 4, 1024, True), (30, 6, 256, False), (64, 32, 1024, False),
                                             (64, 64, 256, False)])
def test_quantizers_that_change_the_code_path(monkeypatch, d, m, ks, use_bits):
    """Case 3: u16 codes from a bit-packed upload (m 4, ks 1024); m no
    multiple of 4 with a row stride of 8 bytes (d 30, m 6); a table of 128
    KiB that does not fit, so the direct variant runs whatever the switch says
    (d 64, m 32, ks 1024); a table of exactly 64 KiB, the largest that is
    used, with 16-byte code loads (d 64, m 64).  Each against the restatement as case 1, with the
    switch unset, 0 and 1."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    ref, ix, _, _, _ = _compressed_pair(N, d, m, ks, "l2-squared", seed=6, use_bits=use_bits)
    lengths = {0: [None], 65: [40], 257: [40, 101], 1023: [100], 1024: [101], 1025: [1100], 2049: [40, 1101],
               5999: [100, 1100, 2500]}
    fx = _restated(ref, ix, N, d, "l2-squared", 60 + m, lengths)
    try:
        for lut in (None, "0", "1"):
            if lut is None:
                monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
            else:
                monkeypatch.setenv("WV_SBD_PQ_LUT", lut)
            _both_routes(fx)
    finally:
        ix.close()
        ref.close()


def test_overflow_goes_to_the_per_query_path(l2pair, monkeypatch):
    """Case 4, WV_SBD_CAP=128: the query with 400 rows within its target
    outgrows its segment and takes the per-query path, its neighbour with 100
    stays on the pass; on both entry points."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    fx, ix, n = l2pair, l2pair["ix"], l2pair["n"]
    rng = np.random.default_rng(71)
    qs = _queries(rng, 2, fx["d"], fx["metric"])
    lists = _lists(rng, n, [1000, 1000])
    allows = _allow(lists, n)
    targets = np.array([_sorted_dists(fx["ref"], qs[i], allows[i].words, 1000)[r - 1] for i, r in enumerate((400, 100))],
                       np.float32)
    want, want_n = _per_query(ix, qs, targets, -1, allows, 4096)
    assert want_n == [400, 100]
    monkeypatch.setenv("WV_SBD_CAP", "128")
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=4096)
    st = ix.last_sbd_ids_stats()
    assert (st["list_queries"], st["legacy_queries"]) == (1, 1), st
    _assert_same(got, got_n, want, want_n)
    got, got_n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=allows, cap=4096)
    st = ix.last_sbd_stats()
    assert (st["pass_queries"], st["legacy_queries"]) == (1, 1), st
    _assert_same(got, got_n, want, want_n)


def test_query_chunks(l2pair, monkeypatch):
    """Case 4, WV_SBD_IDS_MAX_ENTRIES=2048: 12 queries with 500-id segments
    run as three chunks of queries; the answers are the unchunked call's and
    the per-query call's."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    fx, ix, n = l2pair, l2pair["ix"], l2pair["n"]
    rng = np.random.default_rng(81)
    nq = 12
    qs = _queries(rng, nq, fx["d"], fx["metric"])
    lists = _lists(rng, n, [500] * nq)
    allows = _allow(lists, n)
    targets = np.array([_sorted_dists(fx["ref"], qs[i], allows[i].words, 500)[(21, 151, 451, 100)[i % 4] - 1]
                        for i in range(nq)], np.float32)
    want, want_n = _per_query(ix, qs, targets, -1, allows, 1024)
    monkeypatch.delenv("WV_SBD_IDS_MAX_ENTRIES", raising=False)
    whole, whole_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=1024)
    monkeypatch.setenv("WV_SBD_IDS_MAX_ENTRIES", "2048")
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=1024)
    st = ix.last_sbd_ids_stats()
    assert (st["list_queries"], st["legacy_queries"]) == (nq, 0), st
    _assert_same(got, got_n, whole, whole_n)
    _assert_same(got, got_n, want, want_n)
    assert sorted(set(got_n.tolist())) == [21, 100, 151, 451]


def test_added_rows():
    """Case 5: rows added to a compressed KMeans index after its codes were
    uploaded are encoded on the device; a list naming three of them gets them
    back, and the batch equals the per-query call."""
    n0, n1, d, m, ks = 3000, 3300, 16, 4, 256
    rng = np.random.default_rng(21)
    base = rng.standard_normal((n1, d)).astype(np.float32)
    cent = _centroids(base, m, ks, 21)
    enc = O.pq_encode_kmeans(base, cent)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n1)
    ix.upload_vectors(base[:n0])
    ix.set_pq(cent, encoder="kmeans")
    ix.upload_pq_codes(enc[:n0])
    ix.set_compressed(True)
    ix.add(np.arange(n0, n1), base[n0:])
    added = np.array([n0, n0 + 150, n1 - 1], np.uint64)
    nq = 4
    qs = base[added[[0, 1, 2, 0]].astype(np.int64)] + np.float32(0.01)
    lists = [np.sort(np.concatenate([rng.choice(n0, 300 + 100 * i, replace=False).astype(np.uint64), added]))
             for i in range(nq)]
    allows = _allow(lists, n1)
    targets = np.full(nq, 1e30, np.float32)   # every listed row is within
    want, want_n = _per_query(ix, qs, targets, -1, allows, 4096)
    got, got_n = ix.search_by_vector_distance_batch_ids(qs, targets, lists, -1, cap=4096)
    assert ix.last_sbd_ids_stats()["legacy_queries"] == 0
    _assert_same(got, got_n, want, want_n)
    for i in range(nq):
        assert got_n[i] == len(lists[i]) and np.isin(added, got[i][0]).all()
        dist = np.array([O.pq_distance(O.L2, qs[i], enc[int(r)].tobytes(), cent, ks) for r in got[i][0]], np.float32)
        assert np.array_equal(dist.view(np.uint32), got[i][1].view(np.uint32))
    got, got_n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=allows, cap=4096)
    assert ix.last_sbd_stats()["legacy_queries"] == 0
    _assert_same(got, got_n, want, want_n)
    ix.close()


def test_through_the_batcher(l2pair, monkeypatch):
    """Case 6: 16 threads call Batcher.search_distance_ids on the compressed
    index, each with a list of its own; every answer is the direct per-query
    call's, and the group went down the list route."""
    monkeypatch.delenv("WV_SBD_PQ", raising=False)
    monkeypatch.delenv("WV_SBD_PQ_LUT", raising=False)
    monkeypatch.delenv("WV_BATCHER_IDS", raising=False)
    fx, ix, n = l2pair, l2pair["ix"], l2pair["n"]
    nt = 16
    rng = np.random.default_rng(111)
    qs = _queries(rng, nt, fx["d"], fx["metric"])
    lists = _lists(rng, n, [300 + 40 * t for t in range(nt)])
    allows = _allow(lists, n)
    targets = np.array([_sorted_dists(fx["ref"], qs[t], allows[t].words, 1000)[(5, 100, 151, 250)[t % 4] - 1]
                        for t in range(nt)], np.float32)
    want, _ = _per_query(ix, qs, targets, -1, allows, 4096)
    b = W.Batcher(ix, max_batch=nt, max_wait_us=5_000_000)
    got = [None] * nt

    def worker(t):
        got[t] = b.search_distance_ids(qs[t], float(targets[t]), -1, lists[t], cap=4096)

    th = [threading.Thread(target=worker, args=(t,)) for t in range(nt)]
    for t in th:
        t.start()
    for t in th:
        t.join(120)
    st = ix.last_sbd_ids_stats()
    b.close()
    for t in range(nt):
        assert got[t] is not None, t
        assert got[t][0].tolist() == want[t][0].tolist(), t
        assert np.array_equal(got[t][1].view(np.uint32), want[t][1].view(np.uint32)), t
        assert len(got[t][0]) == (5, 100, 151, 250)[t % 4]
    assert st["list_queries"] > 0 and st["legacy_queries"] == 0, st
