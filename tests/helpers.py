"""Comparison helpers shared by the parity tests."""
import numpy as np


def same(a_ids, a_d, b_ids, b_d):
    """ids identical, distances bit-identical."""
    assert np.asarray(a_ids).tolist() == np.asarray(b_ids).tolist()
    assert np.array_equal(np.asarray(a_d, np.float32).view(np.uint32), np.asarray(b_d, np.float32).view(np.uint32))


def same_tie_aware(a_ids, a_d, b_ids, b_d):
    """Distances bit-identical; ids identical up to the order among equal
    distances, and free at the k-boundary distance (the reference breaks ties
    by heap layout, the GPU by id: SURVEY 8c)."""
    a_d = np.asarray(a_d, np.float32)
    b_d = np.asarray(b_d, np.float32)
    a_ids, b_ids = np.asarray(a_ids), np.asarray(b_ids)
    assert np.array_equal(a_d.view(np.uint32), b_d.view(np.uint32))
    if len(a_d) == 0:
        return
    last = a_d[-1]
    for v in np.unique(a_d):
        if v == last:
            continue
        assert set(a_ids[a_d == v].tolist()) == set(b_ids[b_d == v].tolist())


def tie_aware_equal(a_ids, a_d, b_ids, b_d) -> bool:
    try:
        same_tie_aware(a_ids, a_d, b_ids, b_d)
        return True
    except AssertionError:
        return False


def recall(ids, truth, k=10):
    """matches / (k * nq) against exact truths (recall_test.go:121-137)."""
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(np.asarray(ids).tolist(),
                                                                            np.asarray(truth).tolist())]))


def merge_lists(parts, k):
    """Merge per-shard (ids, dists, n) lists by (dist, id): index.go:1039-1043
    with the (dist, id) order of the ABI."""
    nq = parts[0][0].shape[0]
    out_i = np.zeros((nq, k), np.uint64)
    out_d = np.zeros((nq, k), np.float32)
    out_n = np.zeros(nq, np.int32)
    for q in range(nq):
        c = sorted((float(p[1][q, j]), int(p[0][q, j])) for p in parts for j in range(int(p[2][q])))[:k]
        out_n[q] = len(c)
        for j, (d, i) in enumerate(c):
            out_d[q, j] = d
            out_i[q, j] = i
    return out_i, out_d, out_n


def unexplained(ref, qs, k, ef, gi, gd, oi, od, with_waived=False):
    """Queries whose GPU answer differs from the restatement's beyond tie
    order, although the restatement took no decision between equal distances
    (the reference orders equal distances by heap layout).
    with_waived: also the tie-waived queries (the answer differs and the
    restatement reports ties > 0), so that a caller can cap their share."""
    bad, waived = [], []
    for i in range(len(qs)):
        if not tie_aware_equal(gi[i], gd[i], oi[i], od[i]):
            if ref.knn_search(qs[i], k, ef, with_stats=True)[2]["ties"] == 0:
                bad.append(i)
            else:
                waived.append(i)
    return (bad, waived) if with_waived else bad


def unexplained_filtered(ref, qs, k, ef, words, gi, gd, gn, oi, od, on, with_waived=False):
    """Queries whose GPU answer is neither the restatement's (up to tie order)
    nor explained: the restatement took a decision between equal distances
    (heap layout), or the query fell back to the exact filtered
    scan (its answer then equals flatSearch's: a superset in quality).
    `words`: the shared allow bitmap (or None), or one bitmap per query.
    Returns (unexplained, answered-as-flatSearch), with_waived: and the
    tie-waived queries (the answer differs and the restatement reports
    ties > 0)."""
    bad, flat, waived = [], [], []
    per_query = isinstance(words, (list, tuple))
    for i in range(len(qs)):
        if gn[i] == on[i] and tie_aware_equal(gi[i][:gn[i]], gd[i][:gn[i]], oi[i][:on[i]], od[i][:on[i]]):
            continue
        w = words[i] if per_query else words
        if ref.knn_search(qs[i], k, ef, allow=w, with_stats=True)[2]["ties"] > 0:
            waived.append(i)
            continue
        fi, fd, fn, _ = ref.search_batch(qs[i:i + 1], k, ef, allow=w, mode=1)   # flatSearch
        fi, fd, fn = fi[0], fd[0], int(fn[0])
        if fn == gn[i] and tie_aware_equal(gi[i][:fn], gd[i][:fn], fi[:fn], fd[:fn]):
            flat.append(i)
            continue
        bad.append(i)
    return (bad, flat, waived) if with_waived else (bad, flat)


# ---------------------------------------------------------------- PQ-compressed pairs
def pq_centroids(base, m, ks, seed=0):
    """A fitted-looking quantizer: per segment, ks distinct data rows' segments."""
    rng = np.random.default_rng(seed)
    n, d = base.shape
    ds = d // m
    rows = rng.choice(n, ks, replace=False)
    return np.stack([base[rows, i * ds:(i + 1) * ds] for i in range(m)]).astype(np.float32)


def compressed_inputs(n, d, m, ks, metric, use_bits, seed, M=16, efc=64, base=None):
    """The CPU half of compressed_pair: (ref, base, cent, enc) -- the
    restatement's graph over `base` (default: standard-normal rows from
    `seed`, row-normalised for cosine), compressed with a table cut from ks
    distinct data rows and the codes of O.pq_encode_kmeans."""
    import pyoracle as O
    if base is None:
        base = np.random.default_rng(seed).standard_normal((n, d)).astype(np.float32)
        if metric == "cosine-dot":
            base = O.normalize_rows(base)
    ref = O.Index(d, metric, M, efc, capacity=n, seed=seed)
    ref.add_batch(base, threads=8)
    cent = pq_centroids(base, m, ks, seed)
    enc = O.pq_encode_kmeans(base, cent, use_bits)
    ref.compress(cent, enc, use_bits)
    return ref, base, cent, enc


def upload_compressed(ref, base, cent, enc, metric, use_bits, M=16, capacity=None):
    """The GPU index serving the restatement's graph and codes, compressed on."""
    import weaviate_amd as W
    n, d = base.shape
    ix = W.GPUVectorIndex(d, metric, capacity=capacity or n, max_connections=M)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    ix.set_pq(cent, use_bits_encoding=use_bits)
    ix.upload_pq_codes(enc)
    ix.set_compressed(True)
    return ix


def compressed_pair(n, d, m, ks, metric, use_bits, seed, M=16, efc=64, base=None, capacity=None):
    """(ref, ix, base, cent, enc): the restatement and the GPU index over the
    same rows, graph, centroid table and codes, both compressed."""
    ref, base, cent, enc = compressed_inputs(n, d, m, ks, metric, use_bits, seed, M, efc, base)
    return ref, upload_compressed(ref, base, cent, enc, metric, use_bits, M, capacity), base, cent, enc


# The compressed k-NN cases of tests/test_gpu_pq_search.py, shared with the CPU
# test of the tie shares (tests/test_pq.py): (d, segments, centroids, bits-encoding)
PQ_LAYOUTS = [(32, 16, 256, False), (30, 6, 256, False), (32, 4, 1024, True), (24, 3, 1024, False),
              (20, 20, 16, True), (48, 6, 4096, True)]
PQ_METRICS = ["l2-squared", "dot", "cosine-dot"]
PQ_N, PQ_NQ, PQ_K, PQ_SEED = 5000, 200, 10, 5
PQ_EF_UNFILTERED = (10, 100, 200, 300)     # NR = 1, 2, 4 and the LDS-results kernel
PQ_EF_FILTERED = (64, 128)
PQ_CAP_UNFILTERED, PQ_CAP_FILTERED = 0.05, 0.10   # tie-waived share of a case's queries
# The selective shared list at ef 64 (L2, layouts 1 and 3) holds 5 % of the
# rows, not 2 %: with a 2 % list the restatement reports ties > 0 for 85 to 149
# of 200 queries (six list seeds, three graph seeds, both layouts), so no seed
# keeps the share under 25 %.  With the 5 % list of pq_case_data the share
# measured on the restatement alone is 34 of 200 (17 %) at layout 1 and 44 of
# 200 (22 %) at layout 3 (tests/test_pq.py recomputes both); the cap is that
# share + 5 points, never above 25 %.
PQ_CAP_SELECTIVE = {0: 0.22, 2: 0.25}
PQ_TINY_LIST = 40     # a shared list shorter than ef 64: the first rows of the 30 % list


def pq_filtered_pairs():
    """(layout index, metric) of the filtered cases: every layout under L2,
    layouts 1 and 3 under dot and cosine."""
    return [(li, "l2-squared") for li in range(len(PQ_LAYOUTS))] + \
           [(li, mt) for mt in ("dot", "cosine-dot") for li in (0, 2)]


def pq_case_data(li, metric):
    """Everything a case draws, from default_rng(d + m) in a fixed order:
    rows, 203 queries (the first 200 are the batch, 203 the short last block),
    a shared 30 % list, 200 per-query 30 % lists, 3 % tombstones and a shared
    5 % list (ids, ascending)."""
    import pyoracle as O
    d, m, ks, use_bits = PQ_LAYOUTS[li]
    rng = np.random.default_rng(d + m)
    base = rng.standard_normal((PQ_N, d)).astype(np.float32)
    qs = rng.standard_normal((PQ_NQ + 3, d)).astype(np.float32)
    if metric == "cosine-dot":
        base, qs = O.normalize_rows(base), O.normalize_rows(qs)
    shared = np.nonzero(rng.random(PQ_N) < 0.3)[0]
    per = [np.nonzero(rng.random(PQ_N) < 0.3)[0] for _ in range(PQ_NQ)]
    dead = np.sort(rng.choice(PQ_N, int(0.03 * PQ_N), replace=False))
    selective = np.nonzero(rng.random(PQ_N) < 0.05)[0]
    return dict(base=base, qs=qs, shared=shared, per=per, dead=dead, selective=selective)


def pq_case_inputs(li, metric):
    """pq_case_data plus the compressed restatement over its rows; the
    tombstones never hold the entry point."""
    d, m, ks, use_bits = PQ_LAYOUTS[li]
    c = pq_case_data(li, metric)
    ref, _, cent, enc = compressed_inputs(PQ_N, d, m, ks, metric, use_bits, PQ_SEED, base=c["base"])
    ep = int(ref.export_graph()["entrypoint"])
    c["dead"] = c["dead"][c["dead"] != ep]
    c.update(ref=ref, cent=cent, enc=enc, layout=PQ_LAYOUTS[li], metric=metric)
    return c


def pq_added_inputs(li, metric, n0=4500):
    """The case's rows with the graph, the table and the restatement over the
    first n0 only; `enc` holds the KMeans codes of all rows, those past n0 as
    an Add after the snapshot encodes them (insert.go:91-95)."""
    import pyoracle as O
    d, m, ks, use_bits = PQ_LAYOUTS[li]
    c = pq_case_data(li, metric)
    ref, _, cent, enc0 = compressed_inputs(n0, d, m, ks, metric, use_bits, PQ_SEED, base=c["base"][:n0])
    enc = np.concatenate([enc0, O.pq_encode_kmeans(c["base"][n0:], cent, use_bits)])
    c.update(ref=ref, cent=cent, enc=enc, n0=n0, layout=PQ_LAYOUTS[li], metric=metric)
    return c


def tie_share(ref, qs, k, ef, words=None):
    """Queries for which the restatement reports ties > 0 (a decision between
    equal distances): the most a comparison may waive.  `words`: None, one
    shared bitmap or one per query."""
    per_query = isinstance(words, (list, tuple))
    return sum(ref.knn_search(qs[i], k, ef, allow=(words[i] if per_query else words), with_stats=True)[2]["ties"] > 0
               for i in range(len(qs)))
