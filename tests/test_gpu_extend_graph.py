"""wv_index_extend_graph: the rows added since join the device-built graph as
wv_index_build_graph would have inserted them had it continued.

A build inserts in batches that search the graph of every batch before them,
and members of a batch never see each other.  Up to a batch boundary n0 the
schedule for n rows and the schedule for n0 rows alone are the same, so a build
of n0 rows extended to n must equal the one-shot build of n rows bit for bit.
Runs on an MI355X (-m gpu).
"""
import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W

pytestmark = pytest.mark.gpu

N, D, M, EFC, DIV = 6000, 16, 8, 32, 32
NIL = 0xFFFFFFFF
# seed 17: the ids below N0 reach level 3, id 4801 draws level 5 (the level
# stride of `upper` goes from 3 to 5 and the entrypoint moves); seed 7: level 4
# is reached below N0 and never above it.  (The draw is the oracle's and needs
# no GPU; the first test asserts both on the downloaded levels.)
SEED_GROW, SEED_SAME = 17, 7


def _boundaries(n, div=DIV):
    """Node counts after each batch of wv_index_build_graph's schedule."""
    b, done = [1], 1
    while done < n:
        done += min(n - done, max(1, min(16384, done // div)))
        b.append(done)
    return b


BOUNDS = _boundaries(N)
N0 = min(BOUNDS, key=lambda x: abs(x - N // 2))           # 2996
N1 = min(BOUNDS, key=lambda x: abs(x - 2 * N // 3))       # 3947
N_OFF = N // 2                                            # 3000: inside a batch


def _base(metric):
    rng = np.random.default_rng(71)
    base = rng.random((N, D), dtype=np.float32)
    if metric != "l2-squared":
        base -= 0.5
    return base


def _index(metric, capacity=N):
    return W.GPUVectorIndex(D, metric, capacity=capacity, max_connections=M)


def _graph(ix):
    g = ix.download_graph()
    g.update(ix.graph_info())
    return g


_one_shot = {}


def _built(metric, seed):
    """Index A: every row, one wv_index_build_graph (computed once per case)."""
    if (metric, seed) not in _one_shot:
        ix = _index(metric)
        ix.upload_vectors(_base(metric))
        ix.build_graph(ef_construction=EFC, seed=seed, batch_div=DIV)
        _one_shot[(metric, seed)] = _graph(ix)
        ix.close()
    return _one_shot[(metric, seed)]


def _split(metric, seed, steps):
    """Built at steps[0] with that capacity, then grown and extended step by step."""
    base = _base(metric)
    ix = _index(metric, capacity=steps[0])
    ix.upload_vectors(base[:steps[0]])
    ix.build_graph(ef_construction=EFC, seed=seed, batch_div=DIV)
    for a, b in zip(steps, steps[1:]):
        ix.reserve(b)
        ix.add(np.arange(a, b), base[a:b])
        assert ix.delta_size() == b - a
        assert ix.extend_graph(ef_construction=EFC, seed=seed, batch_div=DIV) == b - a
        assert ix.delta_size() == 0 and ix.graph_info()["n"] == b
    return ix


def _assert_same_graph(a, b):
    for key in ("n", "entrypoint", "max_level", "n_upper", "deg0", "degU"):
        assert a[key] == b[key], key
    assert np.array_equal(a["levels"], b["levels"])
    assert np.array_equal(a["layer0"], b["layer0"])          # every list, order and padding included
    up = np.nonzero(a["levels"] >= 1)[0]
    for g in (a, b):
        assert (g["upper_row"][up] < g["n_upper"]).all()
    # the lists above layer 0 per (node, level), through upper_row
    assert np.array_equal(a["upper"][a["upper_row"][up]], b["upper"][b["upper_row"][up]])


def _unchanged(ix, before):
    after = _graph(ix)
    for key, v in before.items():
        assert np.array_equal(v, after[key]) if isinstance(v, np.ndarray) else v == after[key], key


@pytest.mark.parametrize("metric", ["l2-squared", "dot", "cosine-dot"])
@pytest.mark.parametrize("seed", [SEED_GROW, SEED_SAME])
def test_split_build_equals_one_shot_build(metric, seed):
    a = _built(metric, seed)
    lv = a["levels"]
    assert N0 in BOUNDS and a["n"] == N
    if seed == SEED_GROW:   # the precondition: the re-layout and a new entrypoint are forced
        assert lv[:N0].max() < lv[N0:].max() and a["entrypoint"] >= N0
    else:
        assert lv[:N0].max() >= lv[N0:].max() and a["entrypoint"] < N0
    ix = _split(metric, seed, [N0, N])
    _assert_same_graph(a, _graph(ix))
    ix.close()


def test_two_steps_equal_one_shot_build():
    assert N0 < N1 < N and N1 in BOUNDS
    ix = _split("l2-squared", SEED_GROW, [N0, N1, N])
    _assert_same_graph(_built("l2-squared", SEED_GROW), _graph(ix))
    ix.close()


def test_uploaded_graph_extends_to_the_one_shot_build():
    """No counts survive an upload and its level stride is the uploaded
    max_level: the extension reads the counts off the lists and re-lays."""
    b = _split("l2-squared", SEED_GROW, [N0])
    g0 = _graph(b)
    b.close()
    c = _index("l2-squared")
    c.upload_vectors(_base("l2-squared"))
    c.upload_graph(g0)
    assert c.graph_info()["n"] == N0
    assert c.extend_graph(ef_construction=EFC, seed=SEED_GROW, batch_div=DIV) == N - N0
    _assert_same_graph(_built("l2-squared", SEED_GROW), _graph(c))
    c.close()


def _same_tie_aware(a_ids, a_d, b_ids, b_d):
    assert np.array_equal(a_d.view(np.uint32), b_d.view(np.uint32))
    last = a_d[-1]
    for v in np.unique(a_d):
        if v != last:
            assert set(a_ids[a_d == v].tolist()) == set(b_ids[b_d == v].tolist())


def _recall(ids, truth, k=10):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(ids.tolist(), truth.tolist())]))


def test_unaligned_split_keeps_invariants_and_recall():
    """Off a batch boundary the schedule differs from the one-shot build's, and
    so may the graph: it keeps the build's invariants, the recall of the
    restatement's build within 0.5 points, and the restatement answers on it
    as the GPU does."""
    assert N_OFF not in BOUNDS
    seed, ef = SEED_GROW, 64
    base = _base("l2-squared")
    qs = np.random.default_rng(72).random((500, D), dtype=np.float32)
    ix = _split("l2-squared", seed, [N_OFF, N])
    g = _graph(ix)
    l0, lv, up = g["layer0"], g["levels"], g["upper"]
    assert g["n"] == N and g["deg0"] == 2 * M and g["degU"] == M
    assert l0.shape == (N, 2 * M) and up.shape[2] == M            # degree <= 2M / <= M
    for lists in (l0, up):
        assert (lists[lists != NIL] < N).all()
    assert not (l0 == np.arange(N, dtype=np.uint32)[:, None]).any()
    nodes = np.nonzero(lv >= 1)[0]
    assert not (up[g["upper_row"][nodes]] == nodes.astype(np.uint32)[:, None, None]).any()
    assert lv[g["entrypoint"]] == g["max_level"] == lv.max()
    ref = O.Index(D, "l2-squared", M, EFC, capacity=N, seed=seed)
    ref.add_batch(base, threads=8)
    assert np.array_equal(ref.export_graph()["levels"][1:], lv[1:])
    truth, _, _ = O.flat_scan(O.L2, base, qs, 10)
    gi, gd, _ = ix.search_batch(qs, 10, ef=ef, mode="hnsw")
    oi, _, _, _ = ref.search_batch(qs, 10, ef, threads=8)
    r_gpu, r_cpu = _recall(gi, truth), _recall(oi, truth)
    print(f"recall@10 ef {ef}: extended graph {r_gpu:.4f}, restatement's build {r_cpu:.4f}")
    assert r_gpu >= r_cpu - 0.005, (r_gpu, r_cpu)
    ref2 = O.Index(D, "l2-squared", M, EFC, capacity=N, seed=seed)
    ref2.import_graph(base, g)
    ri, rd, _, _ = ref2.search_batch(qs, 10, ef, threads=8)
    for i in range(len(qs)):
        _same_tie_aware(gi[i], gd[i], ri[i], rd[i])
    ix.close()


def test_nothing_to_add_changes_nothing():
    ix = _split("l2-squared", SEED_SAME, [N0])
    before = _graph(ix)
    assert ix.extend_graph(ef_construction=EFC, seed=SEED_SAME, batch_div=DIV) == 0
    _unchanged(ix, before)
    assert ix.delta_size() == 0 and ix.graph_info()["n"] == N0
    ix.close()


def test_bad_arguments_on_a_live_index():
    ix = _split("l2-squared", SEED_SAME, [N0])
    before = _graph(ix)
    for kw in (dict(ef_construction=0), dict(ef_construction=513), dict(batch_div=0)):
        with pytest.raises(W.WvError) as e:
            ix.extend_graph(**kw)
        assert e.value.code == 1
    _unchanged(ix, before)
    ix.close()


def _refused(ix, reason):
    with pytest.raises(W.WvError) as e:
        ix.extend_graph(ef_construction=EFC, seed=SEED_SAME, batch_div=DIV)
    assert e.value.code == 4 and reason in str(e.value), str(e.value)


def test_refusals_leave_the_graph_alone():
    base = _base("l2-squared")
    # no graph
    ix = _index("l2-squared")
    ix.upload_vectors(base)
    _refused(ix, "no graph")
    with pytest.raises(W.WvError):
        ix.graph_info()
    ix.close()
    b = _split("l2-squared", SEED_SAME, [N0])
    g0 = _graph(b)
    # a tombstone on a graph node; the same call succeeds once it is gone.
    # One on a row still to be inserted is no obstacle.
    b.reserve(N)
    b.add(np.arange(N0, N), base[N0:])
    b.add_tombstones([5, N0 + 3])
    _refused(b, "tombstone")
    _unchanged(b, g0)
    assert b.delta_size() == N - N0 - 1
    b.remove_tombstones([5])
    assert b.extend_graph(ef_construction=EFC, seed=SEED_SAME, batch_div=DIV) == N - N0
    _assert_same_graph(_built("l2-squared", SEED_SAME), _graph(b))
    b.close()
    # a graph uploaded with other degrees
    wide = dict(g0)
    wide["layer0"] = np.concatenate([g0["layer0"], np.full((N0, 2), NIL, np.uint32)], axis=1)
    ix = _index("l2-squared")
    ix.upload_vectors(base)
    ix.upload_graph(wide)
    before = _graph(ix)
    assert before["deg0"] == 2 * M + 2
    _refused(ix, "degrees")
    _unchanged(ix, before)
    ix.close()
    # a nil node in an uploaded graph
    holed = dict(g0)
    holed["levels"] = g0["levels"].copy()
    nil = 7 if g0["entrypoint"] != 7 else 8
    holed["levels"][nil] = -1
    ix = _index("l2-squared")
    ix.upload_vectors(base)
    ix.upload_graph(holed)
    before = _graph(ix)
    _refused(ix, "nil")
    _unchanged(ix, before)
    ix.close()
    # a row between the graph and n_rows without a vector
    ix = _index("l2-squared")
    ix.upload_vectors(base[:N0])
    ix.upload_graph(g0)
    ix.upload_vectors(base[N0 + 10:], first_id=N0 + 10)
    before = _graph(ix)
    _refused(ix, "no vector")
    _unchanged(ix, before)
    ix.close()
