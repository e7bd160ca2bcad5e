"""The f16 MFMA threshold filter of search_by_vector_distance_batch
(set_sbd_key_pass) on a graphless index, where every round is exact.

The reference is numpy float64: per query the eligible rows (not tombstoned,
allowed) sorted by (distance, id) and cut at the target.  Data A (integers
0..15) makes fp32, f16 and float64 distances the same integers: ids, counts and
distances must be equal.  Data B (Gaussian) puts each target in the middle of
a gap of the sorted float64 distances: the id set must be equal, the distances
within the fp32 accumulation bound, and everything bit-identical to the same
index with the switch off.  Runs on an MI355X (-m gpu).
"""
import functools
import zlib

import numpy as np
import pytest

import weaviate_amd as W

pytestmark = pytest.mark.gpu

RANKS = (0, 7, 150, 1500)
U = 2.0 ** -24


def _dist64(metric, base, qs):
    b, q = base.astype(np.float64), qs.astype(np.float64)
    if metric == "l2-squared":
        return (q * q).sum(1)[:, None] - 2.0 * q @ b.T + (b * b).sum(1)[None, :]
    if metric == "cosine-dot":
        b = b / np.linalg.norm(b, axis=1, keepdims=True)
        q = q / np.linalg.norm(q, axis=1, keepdims=True)
        return 1.0 - q @ b.T
    return -(q @ b.T)


def _tolerance(metric, d, base, qs):
    """|fp32 reference-order distance - float64| per query: 6 (D + 4) 2^-24 times
    (|q| + max|x|)^2 (L2) or |q| max|x| (dot), the accumulation bound h16_eps uses;
    cosine has unit norms and two fp32 normalisations of (D + 4) 2^-24 each."""
    qn = np.linalg.norm(qs.astype(np.float64), axis=1)
    xn = np.linalg.norm(base.astype(np.float64), axis=1).max()
    if metric == "l2-squared":
        return 6 * (d + 4) * U * (qn + xn) ** 2
    if metric == "dot":
        return 6 * (d + 4) * U * qn * xn + 4 * U
    return np.full(len(qs), 8 * (d + 4) * U + 4 * U)


@functools.lru_cache(maxsize=None)
def _case(kind, metric, n, nq, d, allow_kind, rank=None):
    """(base, qs, dead, allow masks or None, targets, reference id lists, dist64);
    computed once per parameter set.  Query q's rank is RANKS[q % 4] (or `rank`),
    clamped to its eligible rows; with nq >= 3 query 1's target is below every
    distance and query 2's above.  A Gaussian query whose gap at the rank is
    under 1e-4 max(1, |d|) is redrawn (never dropped: asserted)."""
    rng = np.random.default_rng(zlib.crc32(repr((kind, metric, n, nq, d, allow_kind, rank)).encode()))
    draw = (lambda m: rng.integers(0, 16, (m, d)).astype(np.float32)) if kind == "A" else \
        (lambda m: rng.standard_normal((m, d)).astype(np.float32))
    base, qs = draw(n), draw(nq)
    dead = np.unique(np.concatenate([[0, n - 1], rng.choice(n, max(1, n * 3 // 100), replace=False)]))
    elig = np.ones((nq, n), bool)
    masks = None
    if allow_kind == "shared":
        masks = np.broadcast_to(rng.random(n) < 0.6, (nq, n))
    elif allow_kind == "perq":
        masks = rng.random((nq, n)) < 0.6
    if masks is not None:
        elig &= masks
    elig[:, dead] = False
    targets, ref = np.zeros(nq, np.float32), []
    for q in range(nq):
        for _ in range(50):
            d64 = _dist64(metric, base, qs[q:q + 1])[0]
            rows = np.flatnonzero(elig[q])
            rows = rows[np.lexsort((rows, d64[rows]))]
            ds = d64[rows]
            r = min(RANKS[q % 4] if rank is None else rank, len(rows) - 2)
            if nq >= 3 and q == 1:
                t = ds[0] - 1.0 - abs(ds[0])
            elif nq >= 3 and q == 2:
                t = ds[-1] + 1.0 + abs(ds[-1])
            elif kind == "A":
                t = np.floor(ds[r]) + 0.5
            else:
                t = 0.5 * (ds[r] + ds[r + 1])
                if ds[r + 1] - ds[r] < 1e-4 * max(1.0, abs(ds[r])):
                    qs[q] = draw(1)[0]
                    continue
            break
        else:
            raise AssertionError("no query with a wide enough gap in 50 draws")
        targets[q] = np.float32(t)
        ref.append(rows[ds <= np.float64(targets[q])])
    return base, qs, dead, masks, targets, ref, _dist64(metric, base, qs)


def _index(metric, base, dead):
    n, d = base.shape
    ix = W.GPUVectorIndex(d, metric, capacity=n)
    ix.upload_vectors(base)
    ix.add_tombstones(dead)
    return ix


def _allow(masks, allow_kind, n):
    if masks is None:
        return None
    if allow_kind == "shared":
        return W.AllowList.from_ids(np.flatnonzero(masks[0]), n)
    return [W.AllowList.from_ids(np.flatnonzero(m), n) for m in masks]


def _run(ix, on, qs, targets, allow, cap):
    ix.set_sbd_key_pass(on)
    res, n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=allow, cap=cap)
    return res, n, ix.last_sbd_key_pass_stats()


CASES = [
    pytest.param("l2-squared", 5037, 33, 100, None, "3", id="l2-5037x100-q33"),
    pytest.param("l2-squared", 5037, 600, 128, "shared", "3", id="l2-5037x128-q600-shared"),
    pytest.param("dot", 5037, 33, 128, "perq", "3", id="dot-5037x128-q33-perq"),
    pytest.param("cosine-dot", 5037, 600, 100, None, None, id="cos-5037x100-q600"),
    pytest.param("cosine-dot", 37, 1, 4, "shared", None, id="cos-37x4-q1-shared"),
    pytest.param("dot", 37, 33, 4, None, None, id="dot-37x4-q33"),
    pytest.param("l2-squared", 37, 1, 128, "perq", None, id="l2-37x128-q1-perq"),
    pytest.param("l2-squared", 5037, 1, 4, None, "3", id="l2-5037x4-q1"),
]


@pytest.mark.parametrize("metric,n,nq,d,allow_kind,blocks", CASES)
def test_gaussian_sets_match_float64_and_bits_match_the_scan(monkeypatch, metric, n, nq, d, allow_kind, blocks):
    if blocks:
        monkeypatch.setenv("WV_SBD_H16_BLOCKS", blocks)
    base, qs, dead, masks, targets, ref, d64 = _case("B", metric, n, nq, d, allow_kind)
    ix = _index(metric, base, dead)
    allow = _allow(masks, allow_kind, n)
    want, want_n, off = _run(ix, False, qs, targets, allow, n)
    got, got_n, st = _run(ix, True, qs, targets, allow, n)
    ix.close()
    assert off == {"key_pass_queries": 0, "candidates": 0, "overflow_queries": 0}
    assert st["key_pass_queries"] == nq and st["overflow_queries"] == 0 and st["candidates"] >= int(got_n.sum()), st
    tol = _tolerance(metric, d, base, qs)
    assert got_n.tolist() == want_n.tolist() == [len(r) for r in ref]
    for q in range(nq):
        gi, gd = got[q]
        assert gi.tolist() == want[q][0].tolist(), q
        assert np.array_equal(gd.view(np.uint32), want[q][1].view(np.uint32)), q
        assert set(gi.tolist()) == set(ref[q].tolist()), q
        assert np.abs(gd.astype(np.float64) - d64[q, gi.astype(np.int64)]).max(initial=0.0) <= tol[q], q


@pytest.mark.parametrize("metric,n,nq,d,allow_kind,blocks", [
    pytest.param("l2-squared", 5037, 33, 100, "perq", "3", id="l2-5037x100-q33-perq"),
    pytest.param("dot", 5037, 600, 128, None, "3", id="dot-5037x128-q600"),
    pytest.param("l2-squared", 37, 1, 4, "shared", None, id="l2-37x4-q1-shared"),
])
def test_integer_data_is_exact(monkeypatch, metric, n, nq, d, allow_kind, blocks):
    if blocks:
        monkeypatch.setenv("WV_SBD_H16_BLOCKS", blocks)
    base, qs, dead, masks, targets, ref, d64 = _case("A", metric, n, nq, d, allow_kind)
    ix = _index(metric, base, dead)
    got, got_n, st = _run(ix, True, qs, targets, _allow(masks, allow_kind, n), n)
    ix.close()
    assert st["key_pass_queries"] == nq and st["overflow_queries"] == 0
    assert got_n.tolist() == [len(r) for r in ref]
    for q in range(nq):
        assert got[q][0].tolist() == ref[q].tolist(), q
        assert got[q][1].astype(np.float64).tolist() == d64[q, ref[q]].tolist(), q


def test_wider_vectors_keep_the_scan():
    base, qs, dead, _, targets, ref, _ = _case("B", "l2-squared", 537, 3, 132, None, 7)
    ix = _index("l2-squared", base, dead)
    want, want_n, _ = _run(ix, False, qs, targets, None, 537)
    got, got_n, st = _run(ix, True, qs, targets, None, 537)
    ix.close()
    assert st == {"key_pass_queries": 0, "candidates": 0, "overflow_queries": 0}
    assert got_n.tolist() == want_n.tolist() == [len(r) for r in ref]
    for (gi, gd), (wi, wd) in zip(got, want):
        assert gi.tolist() == wi.tolist() and np.array_equal(gd.view(np.uint32), wd.view(np.uint32))


@pytest.mark.parametrize("env,overflow", [
    pytest.param({"WV_SBD_H16_CAND": "64"}, True, id="candidates-overflow-to-the-scan"),
    pytest.param({"WV_SBD_CAP": "128"}, None, id="list-overflow-to-the-per-query-path"),
])
def test_overflow_routes(monkeypatch, env, overflow):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base, qs, dead, _, targets, ref, _ = _case("B", "l2-squared", 5037, 5, 100, None, 1500)
    ix = _index("l2-squared", base, dead)
    got, got_n, st = _run(ix, True, qs, targets, None, 5037)
    legacy = ix.last_sbd_stats()["legacy_queries"]
    ix.close()
    assert st["key_pass_queries"] == 5
    if overflow:
        assert st["overflow_queries"] > 0 and legacy == 0, st
    else:
        assert legacy > 0   # (1501 rows within the target outgrow a 128-entry list: as before the filter)
    assert got_n.tolist() == [len(r) for r in ref] and 1501 in got_n.tolist()
    for q in range(5):
        assert set(got[q][0].tolist()) == set(ref[q].tolist()), q
