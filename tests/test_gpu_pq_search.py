"""k-NN search on a PQ-compressed index against the restatement (-m gpu):
search_batch / search_by_vector after compress(), over the code layouts, the
metrics, ef (every result-list variant of the compressed HNSW kernel), allow
lists, tombstones, rows added after the graph, the flat route and the
flat / graph dispatch.

Compressed HNSW: wv_hnsw_kernel<METRIC, PQ=true, NR> (wv_hnsw.hip) with
pq_dist_row (wv_device.h); under a list or tombstones the LDS side-set kernel,
its 2048-entry second pass and the per-query flat fallback (run_hnsw,
wv_search_hnsw.hip).  Flat: run_pq_flat (wv_search_exact.hip: scan, segmented
radix sort, wv_pq_topk_kernel).  Reference: search.go:171-199, index.go:493-511,
flat_search.go:19-74 as restated in oracle/.

A GPU answer that differs from the restatement's beyond tie order is accepted
only where the restatement itself took a decision between equal distances
(ties > 0: the reference orders those by heap layout) -- and the
share of such waived queries is capped (helpers.PQ_CAP_*; tests/test_pq.py
bounds the restatement's own tie share for these inputs on the CPU) -- or,
under a filter, where the device reported a fallback and the answer is
flatSearch's.
"""
import contextlib

import numpy as np
import pytest

import helpers as H
import pyoracle as O
import weaviate_amd as W
from helpers import merge_lists, same, same_tie_aware, tie_aware_equal, unexplained, unexplained_filtered

pytestmark = pytest.mark.gpu

THREADS = 8
N, NQ, K = H.PQ_N, H.PQ_NQ, H.PQ_K
LAYOUT_IDS = range(len(H.PQ_LAYOUTS))


@pytest.fixture(scope="module")
def pairs():
    """(layout, metric) -> the case's inputs, restatement and GPU index, built once."""
    cache = {}

    def get(li, metric):
        if (li, metric) not in cache:
            c = H.pq_case_inputs(li, metric)
            c["ix"] = H.upload_compressed(c["ref"], c["base"], c["cent"], c["enc"], metric, c["layout"][3])
            c["shared_al"] = W.AllowList.from_ids(c["shared"], N)
            c["selective_al"] = W.AllowList.from_ids(c["selective"], N)
            cache[(li, metric)] = c
        return cache[(li, metric)]

    yield get
    for c in cache.values():
        c["ix"].close()


def _per_lists(c):
    if "per_al" not in c:
        c["per_al"] = [W.AllowList.from_ids(p, N) for p in c["per"]]
    return c["per_al"]


@contextlib.contextmanager
def _tombstoned(c):
    dead = [int(t) for t in c["dead"]]
    for t in dead:
        c["ref"].add_tombstone(t)
    c["ix"].add_tombstones(dead)
    try:
        yield set(dead)
    finally:
        for t in dead:
            c["ref"].remove_tombstone(t)
        c["ix"].remove_tombstones(dead)


def _ref_batch(ref, qs, k, ef, words, mode=0):
    """ref.search_batch with None, one shared bitmap or one bitmap per query."""
    if not isinstance(words, list):
        return ref.search_batch(qs, k, ef, allow=words, mode=mode, threads=THREADS)[:3]
    oi = np.zeros((len(qs), k), np.uint64)
    od = np.zeros((len(qs), k), np.float32)
    on = np.zeros(len(qs), np.int32)
    for i in range(len(qs)):
        a, b, c, _ = ref.search_batch(qs[i:i + 1], k, ef, allow=words[i], mode=mode)
        oi[i], od[i], on[i] = a[0], b[0], c[0]
    return oi, od, on


def _returned(gi, gn):
    return {int(x) for i in range(len(gn)) for x in gi[i, : gn[i]]}


# ---------------------------------------------------------------- (a) unfiltered HNSW
# ef 10 / 100 / 200 / 300 -> 64 / 128 / 256 results in registers (NR 1, 2, 4) and
# the LDS-results kernel; 203 queries leave a short last block at 4 waves a block
@pytest.mark.parametrize("ef,nq", [(10, NQ), (100, NQ), (200, NQ), (300, NQ), (100, NQ + 3)])
@pytest.mark.parametrize("metric", H.PQ_METRICS)
@pytest.mark.parametrize("li", LAYOUT_IDS)
def test_unfiltered_hnsw_equals_restatement(pairs, li, metric, ef, nq):
    c = pairs(li, metric)
    ref, ix, qs = c["ref"], c["ix"], c["qs"][:nq]
    gi, gd, gn = ix.search_batch(qs, K, ef=ef, mode="hnsw")
    oi, od, on, _ = ref.search_batch(qs, K, ef, threads=THREADS)
    assert gn.tolist() == on.tolist()
    bad, waived = unexplained(ref, qs, K, ef, gi, gd, oi, od, with_waived=True)
    print(f"layout {c['layout']} {metric} ef {ef} nq {nq}: tie-waived {len(waived)}")
    assert not bad, bad[:10]
    assert len(waived) <= H.PQ_CAP_UNFILTERED * nq, waived


# ---------------------------------------------------------------- (b), (c) filtered HNSW
def _filtered_case(c, ef, gpu_allow, words, cap, dead=frozenset()):
    ref, ix, qs = c["ref"], c["ix"], c["qs"][:NQ]
    gi, gd, gn = ix.search_batch(qs, K, ef=ef, allow=gpu_allow, mode="hnsw")
    fb = ix.last_batch_stats()["fallbacks"]
    oi, od, on = _ref_batch(ref, qs, K, ef, words)
    bad, flat, waived = unexplained_filtered(ref, qs, K, ef, words, gi, gd, gn, oi, od, on, with_waived=True)
    assert not bad, bad[:10]
    assert len(flat) <= fb, (len(flat), fb)
    assert not _returned(gi, gn) & dead
    assert len(waived) <= cap * NQ, waived
    return fb, len(flat), len(waived)


@pytest.mark.parametrize("kind", ["shared", "per-query", "tombstones", "shared+tombstones"])
@pytest.mark.parametrize("ef", H.PQ_EF_FILTERED)
@pytest.mark.parametrize("li,metric", H.pq_filtered_pairs())
def test_filtered_hnsw_equals_restatement(pairs, li, metric, ef, kind):
    """A compressed index under a list or tombstones: the LDS side-set kernel,
    the 2048-entry second pass, the per-query flat fallback."""
    c = pairs(li, metric)
    if kind == "per-query":
        gpu_allow = _per_lists(c)
        words = [a.words for a in gpu_allow]
    elif kind == "tombstones":
        gpu_allow = words = None
    else:
        gpu_allow, words = c["shared_al"], c["shared_al"].words
    with _tombstoned(c) if "tombstones" in kind else contextlib.nullcontext(frozenset()) as dead:
        fb, n_flat, n_waived = _filtered_case(c, ef, gpu_allow, words, H.PQ_CAP_FILTERED, dead)
    print(f"layout {c['layout']} {metric} ef {ef} {kind}: fallbacks {fb}, answered as flatSearch {n_flat}, "
          f"tie-waived {n_waived}")


@pytest.mark.parametrize("li", sorted(H.PQ_CAP_SELECTIVE))
def test_selective_list_second_pass_and_fallback(pairs, li):
    """A shared 5 % list at ef 64 (a 2 % list leaves the restatement itself
    tie-dependent for most queries, helpers.PQ_CAP_SELECTIVE): the side set
    outgrows its 256 entries, so the queries re-run with 2048 and, where that
    overflows, fall back to the flat scan.  The fallback count is printed, not
    asserted."""
    c = pairs(li, "l2-squared")
    al = c["selective_al"]
    fb, n_flat, n_waived = _filtered_case(c, 64, al, al.words, H.PQ_CAP_SELECTIVE[li])
    print(f"layout {c['layout']} shared list of {len(c['selective'])} rows, ef 64: fallbacks {fb} of {NQ}, answered as "
          f"flatSearch {n_flat}, tie-waived {n_waived}")


@pytest.mark.parametrize("li", sorted(H.PQ_CAP_SELECTIVE))
def test_list_shorter_than_ef(pairs, li):
    """A shared list of 40 rows at ef 64: the result set never fills, so every
    node the traversal reaches stays a candidate (search.go:282-298) and the
    side set grows with the graph -- the case for the second pass and the
    per-query flat fallback.  The restatement's long traversal meets equal
    distances for 131 and 143 of the 200 queries (ties > 0, measured on the
    CPU), so the waiver cannot be capped usefully here; instead every answer,
    waived or not, must hold what no tie decides: ids from the list, no id
    twice, each distance the PQ distance of its id, ascending (dist, id)
    order.  The fallback count is printed."""
    c = pairs(li, "l2-squared")
    rows = c["shared"][:H.PQ_TINY_LIST]
    al = W.AllowList.from_ids(rows, N)
    fb, n_flat, n_waived = _filtered_case(c, 64, al, al.words, 1.0)
    print(f"layout {c['layout']} shared list of {H.PQ_TINY_LIST} rows, ef 64: fallbacks {fb} of {NQ}, answered as "
          f"flatSearch {n_flat}, tie-waived {n_waived}")
    m, ks, use_bits = c["layout"][1:]
    gi, gd, gn = c["ix"].search_batch(c["qs"][:NQ], K, ef=64, allow=al, mode="hnsw")
    for i in range(NQ):
        ids, ds = gi[i, : gn[i]].astype(np.int64), gd[i, : gn[i]]
        assert set(ids.tolist()) <= set(rows.tolist()) and len(set(ids.tolist())) == len(ids)
        want = np.array([O.pq_distance(O.L2, c["qs"][i], c["enc"][r].tobytes(), c["cent"], ks, use_bits) for r in ids],
                        np.float32)
        assert np.array_equal(ds.view(np.uint32), want.view(np.uint32))
        assert np.lexsort((ids, ds)).tolist() == list(range(len(ids)))


# ---------------------------------------------------------------- (d) rows added after the graph
@pytest.fixture(scope="module")
def added():
    cache = {}

    def get(li, metric):
        if (li, metric) not in cache:
            c = H.pq_added_inputs(li, metric)
            n0, use_bits = c["n0"], c["layout"][3]
            ix = H.upload_compressed(c["ref"], c["base"][:n0], c["cent"], c["enc"][:n0], metric, use_bits, capacity=N)
            ix.add(np.arange(n0, N), c["base"][n0:])      # KMeans: encoded on the device (insert.go:91-95)
            mt = O.METRICS[metric]
            ks = c["layout"][2]
            c["ix"] = ix
            # PQ distances of every query to every added row, once
            c["delta_d"] = np.array([[O.pq_distance(mt, q, c["enc"][r].tobytes(), c["cent"], ks, use_bits)
                                      for r in range(n0, N)] for q in c["qs"][:NQ]], np.float32)
            cache[(li, metric)] = c
        return cache[(li, metric)]

    yield get
    for c in cache.values():
        c["ix"].close()


def _delta_lists(c, allowed):
    """The (dist, id)-sorted scan of the allowed added rows, per query: allowed
    is None, one id set or one per query."""
    n0 = c["n0"]
    ids = np.arange(n0, N)
    out_i = np.zeros((NQ, K), np.uint64)
    out_d = np.zeros((NQ, K), np.float32)
    out_n = np.zeros(NQ, np.int32)
    for q in range(NQ):
        a = allowed[q] if isinstance(allowed, list) else allowed
        keep = np.ones(len(ids), bool) if a is None else np.isin(ids, a)
        di, dd = ids[keep], c["delta_d"][q][keep]
        order = np.lexsort((di, dd))[:K]
        out_n[q] = len(order)
        out_i[q, : len(order)], out_d[q, : len(order)] = di[order], dd[order]
    return out_i, out_d, out_n


@pytest.mark.parametrize("kind", ["unfiltered", "shared", "per-query"])
@pytest.mark.parametrize("metric", ["l2-squared", "dot"])
@pytest.mark.parametrize("li", [0, 2])
def test_added_rows_merge_with_the_graph_search(added, li, metric, kind):
    """run_hnsw_delta on a compressed index: the graph search over the rows of
    the snapshot merged by (dist, id) with a flat PQ scan of the rows added
    since, unfiltered and under shared / per-query lists."""
    c = added(li, metric)
    ref, ix, qs, n0, ef = c["ref"], c["ix"], c["qs"][:NQ], c["n0"], 64
    m, ks, use_bits = c["layout"][1:]
    want_codes = np.array([O.pq_extract(c["enc"][r].tobytes(), m, ks, use_bits) for r in range(n0, N)], np.uint16)
    assert np.array_equal(ix.download_pq_codes(N - n0, first_id=n0), want_codes)
    if kind == "unfiltered":
        gpu_allow = words = allowed = None
    elif kind == "shared":
        gpu_allow = W.AllowList.from_ids(c["shared"], N)
        words, allowed = gpu_allow.words, c["shared"]
    else:
        gpu_allow = [W.AllowList.from_ids(p, N) for p in c["per"]]
        words, allowed = [a.words for a in gpu_allow], c["per"]
    gi, gd, gn = ix.search_batch(qs, K, ef=ef, allow=gpu_allow, mode="hnsw")
    fb = ix.last_batch_stats()["fallbacks"]
    delta = _delta_lists(c, allowed)
    wi, wd, wn = merge_lists([_ref_batch(ref, qs, K, ef, words), delta], K)
    bad, flat, waived = [], [], []
    for i in range(NQ):
        if gn[i] == wn[i] and tie_aware_equal(gi[i, : gn[i]], gd[i, : gn[i]], wi[i, : wn[i]], wd[i, : wn[i]]):
            continue
        w = words[i] if isinstance(words, list) else words
        if ref.knn_search(qs[i], K, ef, allow=w, with_stats=True)[2]["ties"] > 0:
            waived.append(i)      # the graph half took a decision between equal distances
            continue
        fi, fd, fn = (x[i:i + 1] for x in delta)
        xi, xd, xn = merge_lists([ref.search_batch(qs[i:i + 1], K, ef, allow=w, mode=1)[:3], (fi, fd, fn)], K)
        if gn[i] == xn[0] and tie_aware_equal(gi[i, : gn[i]], gd[i, : gn[i]], xi[0, : xn[0]], xd[0, : xn[0]]):
            flat.append(i)        # the graph half fell back to the flat scan
            continue
        bad.append(i)
    print(f"layout {c['layout']} {metric} added rows, {kind}: results from added rows "
          f"{int((gi >= n0).sum())} of {int(gn.sum())}, fallbacks {fb}, answered as flatSearch {len(flat)}, "
          f"tie-waived {len(waived)}")
    assert (gi >= n0).any()
    assert not bad, bad[:10]
    assert len(flat) <= fb, (len(flat), fb)
    cap = H.PQ_CAP_UNFILTERED if kind == "unfiltered" else H.PQ_CAP_FILTERED
    assert len(waived) <= cap * NQ, waived


# ---------------------------------------------------------------- (e) the flat route
def _flat_equal(ref, ix, qs, k, gpu_allow=None, words=None):
    gi, gd, gn = ix.search_batch(qs, k, allow=gpu_allow, mode="exact")
    oi, od, on = _ref_batch(ref, qs, k, 0, words, mode=1)
    assert gn.tolist() == on.tolist()
    for i in range(len(qs)):
        same_tie_aware(gi[i, : gn[i]], gd[i, : gn[i]], oi[i, : on[i]], od[i, : on[i]])
    return gi, gd, gn


def _untouched_past_count(gi, gd, gn):
    """the ABI writes the first n slots only (the wrapper hands in zeroed arrays)"""
    for i in range(len(gn)):
        assert not gi[i, gn[i]:].any() and not gd[i, gn[i]:].view(np.uint32).any()


@pytest.mark.parametrize("k", [1, 10, 100, 300])
@pytest.mark.parametrize("metric", H.PQ_METRICS)
@pytest.mark.parametrize("li", LAYOUT_IDS)
def test_flat_route_k(pairs, li, metric, k):
    c = pairs(li, metric)
    _flat_equal(c["ref"], c["ix"], c["qs"][:NQ], k)


@pytest.mark.parametrize("metric", H.PQ_METRICS)
@pytest.mark.parametrize("li", LAYOUT_IDS)
def test_flat_route_lists(pairs, li, metric):
    """k above the rows a list keeps, an empty list, per-query lists with an
    empty one among them, a list holding tombstoned rows, a single query."""
    c = pairs(li, metric)
    ref, ix, qs = c["ref"], c["ix"], c["qs"][:NQ]
    seven = W.AllowList.from_ids(c["shared"][:7], N)
    gi, gd, gn = _flat_equal(ref, ix, qs, K, seven, seven.words)
    assert gn.tolist() == [7] * NQ
    _untouched_past_count(gi, gd, gn)
    empty = W.AllowList(nbits=N)
    gi, gd, gn = _flat_equal(ref, ix, qs, K, empty, empty.words)
    assert gn.tolist() == [0] * NQ
    _untouched_past_count(gi, gd, gn)
    per = [W.AllowList.from_ids(p[:: 1 + i], N) for i, p in enumerate(c["per"][:24])]   # 1,500 rows down to ~60
    per[3] = W.AllowList(nbits=N)
    per[17] = W.AllowList.from_ids(c["per"][17][:4], N)
    gi, gd, gn = _flat_equal(ref, ix, qs[:24], K, per, [a.words for a in per])
    assert gn[3] == 0 and gn[17] == 4 and gn[0] == K
    _untouched_past_count(gi, gd, gn)
    with _tombstoned(c) as dead:
        assert dead & set(c["shared"].tolist())
        gi, gd, gn = _flat_equal(ref, ix, qs, K, c["shared_al"], c["shared_al"].words)
        assert not _returned(gi, gn) & dead
        gi, gd, gn = _flat_equal(ref, ix, qs, K)          # tombstones alone
        assert not _returned(gi, gn) & dead
    _flat_equal(ref, ix, qs[5:6], K)


def _query_as_searched(metric, q):
    return O.normalize(q) if metric == "cosine-dot" else q      # search.go:68-72


@pytest.mark.parametrize("metric", H.PQ_METRICS)
@pytest.mark.parametrize("li", LAYOUT_IDS)
def test_flat_route_equal_distances_come_back_in_id_order(pairs, li, metric):
    """The ABI's (dist, id) contract: 60 rows share the code tuple of the
    query's nearest row, so they tie as the nearest; k = 25 returns the 25
    smallest of their ids, ascending.  Reference: np.lexsort((ids, dists))
    over O.pq_distance."""
    c = pairs(li, metric)
    ix, q = c["ix"], c["qs"][7]
    m, ks, use_bits = c["layout"][1:]
    mt = O.METRICS[metric]
    x = _query_as_searched(metric, q)
    enc = c["enc"].copy()
    d0 = np.array([O.pq_distance(mt, x, enc[r].tobytes(), c["cent"], ks, use_bits) for r in range(N)], np.float32)
    nearest = int(np.lexsort((np.arange(N), d0))[0])
    twins = np.random.default_rng(li).choice(np.setdiff1d(np.arange(N), [nearest]), 59, replace=False)
    enc[twins] = enc[nearest]
    dists = d0.copy()
    dists[twins] = d0[nearest]
    group = np.sort(np.append(twins, nearest))
    order = np.lexsort((np.arange(N), dists))[:25]
    assert order.tolist() == group[:25].tolist()
    try:
        ix.upload_pq_codes(enc)
        gi, gd, gn = ix.search_batch(q[None], 25, mode="exact")
    finally:
        ix.upload_pq_codes(c["enc"])
    assert gn[0] == 25
    same(gi[0], gd[0], order, dists[order])


@pytest.mark.parametrize("li", LAYOUT_IDS)
def test_flat_route_signed_zero_under_dot(pairs, li):
    """A zero query under dot: every distance is a signed zero (-(+0) = -0 from
    Wrap), equal as keys, so the ids come back as 0..k-1 and the distances
    with the bits O.pq_distance gives them."""
    c = pairs(li, "dot")
    m, ks, use_bits = c["layout"][1:]
    q = np.zeros(c["layout"][0], np.float32)
    want = np.array([O.pq_distance(O.DOT, q, c["enc"][r].tobytes(), c["cent"], ks, use_bits) for r in range(K)],
                    np.float32)
    assert not want.any()         # zeros of either sign
    gi, gd, gn = c["ix"].search_batch(np.stack([q, c["qs"][0], q]), K, mode="exact")
    for i in (0, 2):
        assert gn[i] == K
        same(gi[i], gd[i], np.arange(K), want)


def test_flat_route_batch_across_query_chunks():
    """run_pq_flat takes the queries in chunks of 2^26 (query, row) pairs:
    4,096 rows and 2^26 / 4096 + 5 queries make a full chunk and a last one of
    five.  The queries are 64 distinct ones, tiled; every row of the batch
    equals the answer of its distinct query, and those equal the restatement's."""
    n, d, m, ks, k = 4096, 8, 4, 16, K
    nq = (1 << 26) // n + 5
    ref, ix, base, cent, enc = H.compressed_pair(n, d, m, ks, "l2-squared", False, 17)
    q64 = np.random.default_rng(18).standard_normal((64, d)).astype(np.float32)
    tile = np.arange(nq) % 64
    gi, gd, gn = ix.search_batch(q64[tile], k, mode="exact")
    ix.close()
    oi, od, on, _ = ref.search_batch(q64, k, 0, mode=1, threads=THREADS)
    assert gn.tolist() == on[tile].tolist()
    for j in range(64):
        same_tie_aware(gi[j], gd[j], oi[j], od[j])
    # (dist, id) order makes the answer a function of the query alone
    assert np.array_equal(gi, gi[:64][tile])
    assert np.array_equal(gd.view(np.uint32), gd[:64][tile].view(np.uint32))


# ---------------------------------------------------------------- (f) auto dispatch
def test_auto_dispatch_on_a_compressed_index(pairs):
    """SearchByVector (search.go:64-79) on a compressed index: a list shorter
    than flatSearchCutoff is answered as mode="exact", a longer one as
    mode="hnsw", bit for bit -- whole batches, a batch of both kinds, and
    wv_search_by_vector against the restatement's SearchByVector."""
    c = pairs(0, "l2-squared")
    ref, ix, qs = c["ref"], c["ix"], c["qs"][:NQ]
    short, long_ = c["selective_al"], c["shared_al"]
    cut = (len(short) + len(long_)) // 2
    assert len(short) < cut < len(long_)
    try:
        ix.update_user_config(flat_search_cutoff=cut)
        ref.set_search_config(flat_search_cutoff=cut)
        assert not ix.cfg.forbid_flat
        ei, ed, en = ix.search_batch(qs, K, allow=short, mode="exact")
        ai, ad, an = ix.search_batch(qs, K, allow=short, mode="auto")
        assert an.tolist() == en.tolist()
        same(ai, ad, ei, ed)
        hi, hd, hn = ix.search_batch(qs, K, allow=long_, mode="hnsw")      # ef 0: searchTimeEF(k)
        bi, bd, bn = ix.search_batch(qs, K, allow=long_, mode="auto")
        assert bn.tolist() == hn.tolist()
        same(bi, bd, hi, hd)
        mixed = [short if i % 3 == 0 else long_ for i in range(NQ)]
        mi, md, mn = ix.search_batch(qs, K, allow=mixed, mode="auto")
        flat_rows = np.arange(NQ) % 3 == 0
        assert mn.tolist() == np.where(flat_rows, en, hn).tolist()
        same(mi, md, np.where(flat_rows[:, None], ei, hi), np.where(flat_rows[:, None], ed, hd))
        # one query through wv_search_by_vector: the first one for which the
        # restatement's graph search takes no decision between equal distances
        ef = ix.search_time_ef(K)
        assert ef == O.search_time_ef(-1, 100, 500, 8, K)
        q = next(q for q in qs if ref.knn_search(q, K, ef, with_stats=True)[2]["ties"] == 0
                 and ref.knn_search(q, K, ef, allow=long_.words, with_stats=True)[2]["ties"] == 0)
        for al in (None, short, long_):
            gi, gd = ix.search_by_vector(q, K, allow=al)
            fb = ix.last_batch_stats()["fallbacks"]
            ri, rd = ref.search_by_vector(q, K, allow=None if al is None else al.words)
            if fb:      # answered by the flat scan over the same list
                fi, fd, fn, _ = ref.search_batch(q[None], K, 0, allow=al.words, mode=1)
                ri, rd = fi[0, : fn[0]], fd[0, : fn[0]]
            assert len(gi) == len(ri)
            same_tie_aware(gi, gd, ri, rd)
    finally:
        ix.update_user_config(flat_search_cutoff=40000)
        ref.set_search_config()
