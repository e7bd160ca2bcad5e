"""Insertion events of the f16 key passes (wv_topk.h min_extract): the column
minimum goes in by its position, the column's second smallest key (v_med3
tree, no clearing) decides whether the per-key scan runs, and the wave votes
are scalar compares of the two columns' own lane masks.

Lane (khalf, column) of a wave holds rows 4 khalf + (i & 3) + 8 (i >> 2) of
each 32-row half; queries q and q + 32 of a wave are a lane's two columns.  One
case per batch, its rows planted accordingly in one tile:

  dup      two exact copies at rows 0 and 1 of a tile (one lane, one half):
           the second key equals the minimum
  second   two distinct near neighbours at rows 0 and 2 (one lane, one half)
  crowded  twelve near copies at rows 0-3, 8-11, 16-19: more than BF_KP = 8
           hits in one list (tail handling; the device fallback is allowed
           for a query whose list they crowd)
  columns  queries q and q + 32 identical, one planted neighbour: both columns
           of a lane in one event
  halves   near neighbours at rows 0 and 4: both lane halves in one tile
  padding  the last query of a batch that is no multiple of 64, rows 0 and 1

Every case runs in three modes (running threshold, cross-slot exchange,
seeded), at D = 16 and 128, on every metric, and once at D = 768 (the wide
kernel).  Each batch is checked against the restatement (tie-aware) and bit
for bit against the fp32 pass -- test_gpu_h16_tile_loop._check.  Before any
launch the restatement confirms on the planted query alone that the rows are
in the top k and that the tie or near-tie exists.

No planted row is longer than the corpus's longest: for dot the rows are
a_j r, a_j <= 1, r the corpus's longest row (whose own slot gets half of it),
and the query is r scaled down -- a longer row would widen every query's
certificate and send queries to the fallback, past the event path.

Fallbacks: a query that falls back is answered by the fallback kernel and
says nothing about its events, so the count is asserted.  The parent commit
reports 0 on all 95 batches of the five other cases: 0 is asserted there.  In
the crowded batches it reports 1, the planted query, on 13 of 19: at most 1
there.  On the other six the twelve rows crowd other queries' lists as well
-- with 8,193 queries some lie near the planted one, and for dot a row as long
as the corpus's longest is near many queries -- and the parent commit reports
2-41: PARENT_CROWDED holds its counts as the caps, and before the launch the
restatement confirms that at least as many queries have a planted row in
their top k, i.e. that those fallbacks can be crowded lists too
(profiles/h16_events/README.md).  Runs on an MI355X (-m gpu).
"""
import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from test_gpu_h16_tile_loop import BQ, METRIC_NAMES, _check, _data, _unit

pytestmark = pytest.mark.gpu

K = 10
MODES = {"running": (20001, 513), "xslot": (20001, 16 * BQ + 1), "seeded": (70001, 513)}
# rows of a tile (offsets from its first row) per case
ROWS = {"dup": [0, 1], "second": [0, 2], "crowded": [0, 1, 2, 3, 8, 9, 10, 11, 16, 17, 18, 19], "columns": [0],
        "halves": [0, 4], "padding": [0, 1]}
QUERY = {"dup": 3, "second": 70, "crowded": 140, "columns": 200, "halves": 44, "padding": None}   # None: the last
# crowded batches on which the parent commit reports more fallbacks than the
# planted query: (mode, dim, metric name) -> its count
PARENT_CROWDED = {("running", 128, "dot"): 3, ("xslot", 16, "l2-squared"): 4, ("xslot", 16, "dot"): 41,
                  ("xslot", 128, "l2-squared"): 2, ("xslot", 128, "dot"): 7, ("xslot", 128, "cosine-dot"): 3}


def _plant(base, qs, metric, case, q, row0):
    """Writes the case's rows into base (and the query, for dot; the twin
    query for `columns`); returns (query ids, planted row ids).  Copy j is
    q + b_j u for L2 and cosine (a fixed direction u), a_j r for dot."""
    d = base.shape[1]
    u = np.random.default_rng(99).random(d, dtype=np.float32) - np.float32(0.5)
    offs = ROWS[case]
    if metric == O.DOT:
        longest = int(np.argmax(np.einsum("ij,ij->i", base.astype(np.float64), base.astype(np.float64))))
        r = base[longest].copy()
        base[longest] = np.float32(0.5) * r
        qs[q] = np.float32(0.5) * r
    for j, off in enumerate(offs):
        jj = 0 if case in ("dup", "padding") else j   # exact copies
        if metric == O.DOT:
            x = np.float32(1.0 - 0.005 * jj) * r
        else:
            x = qs[q] + np.float32((0.01 if metric == O.L2 else 0.02) * (jj + 1)) * u
        base[row0 + off] = x
    ids = [q]
    if case == "columns":
        qs[q + 32] = qs[q]
        ids.append(q + 32)
    return ids, [row0 + off for off in offs]


def _confirm(base, qs, metric, case, ids, rows):
    """The restatement on the planted queries alone, before any launch."""
    b, q = (_unit(base), _unit(qs)) if metric == O.COSINE else (base, qs)
    oi, od, on = O.flat_scan(metric, b, q[ids], K, threads=16)
    for r in range(len(ids)):
        top = [int(i) for i in oi[r, : on[r]]]
        pos = [top.index(x) for x in rows if x in top]
        if case == "crowded":   # twelve copies, k = 10: the whole answer is planted rows
            assert set(top) <= set(rows), (case, top)
        else:
            assert len(pos) == len(rows) and max(pos) == len(rows) - 1, (case, top, rows)
        dd = od[r, : on[r]].astype(np.float64)
        if case in ("dup", "padding"):   # the tie
            assert dd[0] == dd[1], (case, dd)
        elif case == "crowded":          # ten distinct keys, all the planted rows'
            assert np.all(np.diff(dd) > 0), (case, dd)
        elif len(rows) > 1:              # the near-tie: apart, and far nearer than the next row
            assert 0 < dd[1] - dd[0] < 0.25 * (dd[2] - dd[0]), (case, dd)


def _fallbacks(base, qs, metric):
    ix = W.GPUVectorIndex(base.shape[1], METRIC_NAMES[metric], capacity=len(base))
    ix.upload_vectors(base)
    ix.search_batch(qs, K, mode="exact")
    fb = ix.last_batch_stats()["fallbacks"]
    ix.close()
    return int(fb)


def _run(case, mode, rows, nq, dim, metric):
    key = (case, mode, dim, METRIC_NAMES[metric])
    base, qs = _data(rows, dim, nq, seed=1000 + dim + 7 * metric + rows % 13, metric=metric)
    norm_max = float(np.max(np.einsum("ij,ij->i", base.astype(np.float64), base.astype(np.float64))))
    q = nq - 1 if QUERY[case] is None else QUERY[case]
    ids, planted = _plant(base, qs, metric, case, q, 256 * (2 + list(ROWS).index(case)))
    if metric == O.DOT:   # (L2 and cosine rows sit beside a query: an ordinary row's length)
        assert float(np.max(np.einsum("ij,ij->i", base.astype(np.float64), base.astype(np.float64)))) <= norm_max
    _confirm(base, qs, metric, case, ids, planted)
    cap = 0
    if case == "crowded":
        cap = PARENT_CROWDED.get(key[1:], 1)
        if cap > 1:   # as many queries, at least, whose answer holds rows of the crowded list
            b, q = (_unit(base), _unit(qs)) if metric == O.COSINE else (base, qs)
            oi, _, _ = O.flat_scan(metric, b, q, K, threads=16)
            reached = int(np.isin(oi, np.array(planted, dtype=oi.dtype)).any(axis=1).sum())
            assert reached >= cap, (key, reached, cap)
    fb = _fallbacks(base, qs, metric)
    print("fallback_queries", key, fb)
    _check(base, qs, metric=metric, k=K)
    assert fb <= cap, (key, fb)


@pytest.mark.parametrize("metric", [O.L2, O.DOT, O.COSINE], ids=lambda m: METRIC_NAMES[m])
@pytest.mark.parametrize("dim", [16, 128])
@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("case", list(ROWS))
def test_planted_event(case, mode, dim, metric):
    rows, nq = MODES[mode]
    _run(case, mode, rows, nq, dim, metric)


@pytest.mark.parametrize("case", list(ROWS))
def test_planted_event_wide_kernel(case):
    """D = 768: wv_bf_h16w_kernel (256-row tiles, 256-query blocks, the same
    lane layout per 32-row group)."""
    _run(case, "wide", 3000, 300, 768, O.L2)
