"""wv_index_cleanup_tombstones: the tombstoned nodes leave the device's graph.

Every live node with an edge to a deleted one is re-linked (or, where its
search overflowed, has the dead edges struck), a deleted entrypoint is
replaced, the deleted nodes become nil and lose their tombstones.  Checked on
the downloaded graph with plain numpy.  Runs on an MI355X (-m gpu).

Recall@10 at ef 64 against numpy's exact answer over the live rows, cleaned
graph / graph built from the live rows alone (measured, MI355X):
    l2 mixed 0.9675 / 0.9545   cos mixed 0.9875 / 0.9710
    l2 one   0.9550 / 0.9525   l2 block  0.9795 / 0.9645
"""
import numpy as np
import pytest

import weaviate_amd as W

pytestmark = pytest.mark.gpu

NIL = 0xFFFFFFFF
EFC, DIV, SEED, EF, NQ = 32, 8, 5, 64, 200
SHAPES = {"l2": (3000, 24, "l2-squared", 8), "cos": (2000, 20, "cosine-dot", 6)}
CASES = [("l2", "mixed"), ("cos", "mixed"), ("l2", "one"), ("l2", "block")]
# the build test grants a batched build 2 points of recall below the sequential one
MARGIN = 0.02


def _rows(case, extra=0):
    n, d, metric, _ = SHAPES[case]
    x = np.random.default_rng(31).random((n + extra, d), dtype=np.float32)
    return x if metric == "l2-squared" else x - 0.5


def _index(case, rows, capacity=None):
    _, d, metric, m = SHAPES[case]
    ix = W.GPUVectorIndex(d, metric, capacity=capacity or len(rows), max_connections=m)
    ix.upload_vectors(rows)
    return ix


def _graph(ix):
    g = ix.download_graph()
    g.update(ix.graph_info())
    return g


_built = {}


def _fresh(case, capacity=None):
    """An index holding the case's rows and their device-built graph (built once, then uploaded)."""
    rows = _rows(case)
    if case not in _built:
        ix = _index(case, rows)
        ix.build_graph(ef_construction=EFC, seed=SEED, batch_div=DIV)
        _built[case] = _graph(ix)
        ix.close()
    ix = _index(case, rows, capacity)
    ix.upload_graph(_built[case])
    return ix, _built[case]


def _deleted(kind, g):
    n, lv = g["n"], g["levels"]
    if kind == "one":
        return np.array([next(i for i in range(n) if lv[i] == 0 and i != g["entrypoint"])])
    if kind == "block":   # every neighbour of some nodes is dead
        return np.arange(1000, 1600)
    # 5 % by a counter-based draw, the entrypoint, and the whole top level
    x = (np.arange(n, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
    x ^= x >> np.uint64(31)
    x *= np.uint64(0xBF58476D1CE4E5B9)
    x ^= x >> np.uint64(29)
    drawn = np.nonzero(x % np.uint64(20) == 0)[0]
    return np.unique(np.concatenate([drawn, [g["entrypoint"]], np.nonzero(lv == g["max_level"])[0]]))


def _lists(g):
    """(owner node, list) for every list of the graph: layer 0, then each upper (row, level)."""
    up_nodes = np.nonzero(g["levels"] >= 1)[0]
    owner = np.full(g["n_upper"], -1, np.int64)   # (-1: the row of a nil node)
    owner[g["upper_row"][up_nodes]] = up_nodes
    out = [(np.arange(g["n"]), g["layer0"])]
    if g["max_level"] > 0:
        out += [(owner, g["upper"][:, l, :]) for l in range(g["max_level"])]
    return out


def _flagged(g, dead):
    """Live nodes with an edge into `dead`, by numpy."""
    is_dead = np.zeros(g["n"] + 1, bool)
    is_dead[dead] = True
    hit = np.zeros(g["n"], bool)
    for owner, rows in _lists(g):
        names = is_dead[np.where(rows == NIL, g["n"], rows)].any(axis=1)
        hit[owner[names & (owner >= 0)]] = True
    return hit & ~is_dead[:-1] & (g["levels"] >= 0)


def _check_graph(g, gone, m):
    n, lv = g["n"], g["levels"]
    assert g["deg0"] == 2 * m and g["degU"] == m and g["layer0"].shape == (n, 2 * m)
    assert (lv[gone] == -1).all()
    live = lv >= 0
    assert live.sum() == n - len(gone) and live.sum() > 1
    ok = np.append(live, False)   # (index n: the pad)
    for owner, rows in _lists(g):
        pad = rows == NIL
        assert (rows[~pad] < n).all()
        assert ok[rows[~pad]].all()                              # no deleted or nil id
        assert (pad[:, 1:] | ~pad[:, :-1]).all()                 # dense prefixes
        assert not (rows == owner[:, None]).any()                # no self link
        s = np.sort(rows, axis=1)
        assert not ((s[:, 1:] == s[:, :-1]) & (s[:, 1:] != NIL)).any()   # no duplicate
        dead_owner = (owner < 0) | ~ok[np.where(owner < 0, n, owner)]
        assert pad[dead_owner].all()
    assert (g["layer0"][live, 0] != NIL).all()                   # every live node is linked
    top = lv[live].max()
    assert g["max_level"] == top and g["entrypoint"] == np.nonzero(live & (lv == top))[0][0]


def _truth(case, rows, live_ids, qs, k=10):
    x, q = rows[live_ids].astype(np.float64), qs.astype(np.float64)
    if SHAPES[case][2] == "cosine-dot":
        x /= np.linalg.norm(x, axis=1, keepdims=True)
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        d = -q @ x.T
    else:
        d = ((q[:, None, :] - x[None, :, :]) ** 2).sum(-1)
    return live_ids[np.argsort(d, axis=1, kind="stable")[:, :k]]


def _recall(ids, truth):
    return float(np.mean([len(set(a) & set(b)) / len(b) for a, b in zip(ids.tolist(), truth.tolist())]))


def _queries(case):
    q = np.random.default_rng(32).random((NQ, SHAPES[case][1]), dtype=np.float32)
    return q if SHAPES[case][2] == "l2-squared" else q - 0.5


def _cleaned(case, kind, capacity=None):
    ix, g0 = _fresh(case, capacity)
    dead = _deleted(kind, g0)
    ix.add_tombstones(dead.tolist())
    return ix, g0, dead, ix.cleanup_tombstones(ef_construction=EFC, batch_div=DIV)


@pytest.mark.parametrize("case,kind", CASES)
def test_cleanup_removes_the_deleted_nodes(case, kind):
    m, rows, qs = SHAPES[case][3], _rows(case), _queries(case)
    ix, g0, dead, counts = _cleaned(case, kind)
    g = _graph(ix)
    _check_graph(g, dead, m)
    assert counts["removed"] == len(dead)
    assert counts["reassigned"] + counts["struck"] == _flagged(g0, dead).sum()
    assert (g["levels"][g["levels"] >= 0] == g0["levels"][g["levels"] >= 0]).all()   # a node keeps its level
    if kind == "mixed":
        assert g["max_level"] < g0["max_level"]
    gi, _, _ = ix.search_batch(qs, 10, ef=EF, mode="hnsw")
    ei, _, _ = ix.search_batch(qs, 10, mode="exact")
    assert not np.isin(gi, dead).any() and not np.isin(ei, dead).any()
    # recall: the cleaned graph against one built from the live rows alone
    live_ids = np.nonzero(g["levels"] >= 0)[0]
    truth = _truth(case, rows, live_ids, qs)
    ref = _index(case, rows[live_ids])
    ref.build_graph(ef_construction=EFC, seed=SEED, batch_div=DIV)
    ri, _, _ = ref.search_batch(qs, 10, ef=EF, mode="hnsw")
    ref.close()
    r_new, r_ref = _recall(gi, truth), _recall(live_ids[ri.astype(np.int64)], truth)
    print(f"{case} {kind}: recall@10 ef {EF} cleaned {r_new:.4f}, built from the live rows {r_ref:.4f}, counts {counts}")
    assert r_new >= r_ref - MARGIN, (r_new, r_ref)
    ix.close()


def test_overflowed_members_are_struck(monkeypatch):
    """A side set of one entry overflows wherever a search meets two deleted
    nodes: those members keep their lists less the dead edges."""
    monkeypatch.setenv("WV_CLEANUP_SIDE_CAP", "1")
    ix, g0, dead, counts = _cleaned("l2", "block")
    g = _graph(ix)
    _check_graph(g, dead, SHAPES["l2"][3])
    assert counts["struck"] > 0 and counts["reassigned"] + counts["struck"] == _flagged(g0, dead).sum()
    ix.close()


def test_two_runs_give_the_same_bits():
    a, _, _, ca = _cleaned("l2", "mixed")
    b, _, _, cb = _cleaned("l2", "mixed")
    ga, gb = _graph(a), _graph(b)
    assert ca == cb
    for key, v in ga.items():
        assert np.array_equal(v, gb[key]) if isinstance(v, np.ndarray) else v == gb[key], key
    a.close()
    b.close()


def test_nothing_deleted_changes_nothing():
    ix, g0 = _fresh("l2")
    assert ix.cleanup_tombstones(ef_construction=EFC, batch_div=DIV) == dict(reassigned=0, removed=0, struck=0)
    g = _graph(ix)
    for key, v in g0.items():
        assert np.array_equal(v, g[key]) if isinstance(v, np.ndarray) else v == g[key], key
    ix.close()
    bare = _index("l2", _rows("l2"))
    with pytest.raises(W.WvError) as e:
        bare.cleanup_tombstones(ef_construction=EFC, batch_div=DIV)
    assert e.value.code == 4 and "no graph" in str(e.value)
    bare.close()


@pytest.mark.parametrize("case", ["l2", "cos"])
def test_extend_after_cleanup(case):
    n, _, _, m = SHAPES[case]
    rows = _rows(case, extra=500)
    ix, _, dead, _ = _cleaned(case, "mixed", capacity=n + 500)
    ix.add(np.arange(n, n + 500), rows[n:])
    assert ix.extend_graph(ef_construction=EFC, seed=SEED, batch_div=DIV) == 500
    g = _graph(ix)
    assert g["n"] == n + 500
    _check_graph(g, dead, m)
    gi, _, _ = ix.search_batch(rows[n:], 10, ef=EF, mode="hnsw")
    found = (gi == np.arange(n, n + 500)[:, None]).any(axis=1).mean()
    # a row that is a graph node is its own nearest neighbour: no harder to
    # find than the ten nearest, so the recall bound of the build applies
    assert found >= 1.0 - MARGIN, found
    assert not np.isin(gi, dead).any()
    ix.close()
