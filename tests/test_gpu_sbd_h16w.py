"""The f16 MFMA threshold filter of search_by_vector_distance_batch for
128 < D <= 1024 (set_sbd_wide_key_pass) on a graphless index.

Cases, reference (numpy float64) and tolerance are test_gpu_sbd_h16.py's; every
case is also compared bit for bit with the same index with the switch off,
where only set_sbd_key_pass is on: alone it leaves these dimensions to the scan
and reports no key-pass stats.  Between them the shapes take both query-block
widths (64 and 256, the last block partial), a partial last tile and a tile
past the segment's end in the ring's last stage, D that is no multiple of 16,
6 to 32 chunks per tile and several segments over 4-6 tiles.  Runs on an
MI355X (-m gpu).
"""
import numpy as np
import pytest

from test_gpu_sbd_h16 import _allow, _case, _index, _tolerance

pytestmark = pytest.mark.gpu

ZERO = {"key_pass_queries": 0, "candidates": 0, "overflow_queries": 0}


def _run(ix, wide, qs, targets, allow, cap):
    ix.set_sbd_key_pass(True)
    ix.set_sbd_wide_key_pass(wide)
    res, n = ix.search_by_vector_distance_batch(qs, targets, -1, allow=allow, cap=cap)
    return res, n, ix.last_sbd_key_pass_stats()


@pytest.mark.parametrize("metric,n,nq,d,allow_kind,blocks", [
    pytest.param("l2-squared", 777, 33, 132, None, "2", id="l2-777x132-q33"),
    pytest.param("dot", 777, 300, 260, "shared", None, id="dot-777x260-q300-shared"),
    pytest.param("cosine-dot", 777, 33, 768, "perq", "2", id="cos-777x768-q33-perq"),
    pytest.param("l2-squared", 1303, 300, 768, "perq", "3", id="l2-1303x768-q300-perq"),
    pytest.param("dot", 1303, 1, 1024, None, "3", id="dot-1303x1024-q1"),
    pytest.param("cosine-dot", 1303, 300, 1024, "shared", None, id="cos-1303x1024-q300-shared"),
    pytest.param("l2-squared", 37, 1, 132, "shared", None, id="l2-37x132-q1-shared"),
])
def test_gaussian_sets_match_float64_and_bits_match_the_scan(monkeypatch, metric, n, nq, d, allow_kind, blocks):
    if blocks:
        monkeypatch.setenv("WV_SBD_H16_BLOCKS", blocks)
    base, qs, dead, masks, targets, ref, d64 = _case("B", metric, n, nq, d, allow_kind)
    ix = _index(metric, base, dead)
    allow = _allow(masks, allow_kind, n)
    want, want_n, off = _run(ix, False, qs, targets, allow, n)
    got, got_n, st = _run(ix, True, qs, targets, allow, n)
    ix.close()
    assert off == ZERO
    assert st["key_pass_queries"] == nq and st["overflow_queries"] == 0 and st["candidates"] >= int(got_n.sum()), st
    tol = _tolerance(metric, d, base, qs)
    assert got_n.tolist() == want_n.tolist() == [len(r) for r in ref]
    for q in range(nq):
        gi, gd = got[q]
        assert gi.tolist() == want[q][0].tolist(), q
        assert np.array_equal(gd.view(np.uint32), want[q][1].view(np.uint32)), q
        assert set(gi.tolist()) == set(ref[q].tolist()), q
        assert np.abs(gd.astype(np.float64) - d64[q, gi.astype(np.int64)]).max(initial=0.0) <= tol[q], q


@pytest.mark.parametrize("metric,n,nq,d,allow_kind", [
    pytest.param("l2-squared", 1303, 33, 260, "perq", id="l2-1303x260-q33-perq"),
    pytest.param("dot", 777, 300, 768, None, id="dot-777x768-q300"),
])
def test_integer_data_is_exact(metric, n, nq, d, allow_kind):
    base, qs, dead, masks, targets, ref, d64 = _case("A", metric, n, nq, d, allow_kind)
    ix = _index(metric, base, dead)
    allow = _allow(masks, allow_kind, n)
    want, want_n, off = _run(ix, False, qs, targets, allow, n)
    got, got_n, st = _run(ix, True, qs, targets, allow, n)
    ix.close()
    assert off == ZERO
    assert st["key_pass_queries"] == nq and st["overflow_queries"] == 0 and st["candidates"] >= int(got_n.sum()), st
    assert got_n.tolist() == want_n.tolist() == [len(r) for r in ref]
    for q in range(nq):
        assert got[q][0].tolist() == want[q][0].tolist() == ref[q].tolist(), q
        assert np.array_equal(got[q][1].view(np.uint32), want[q][1].view(np.uint32)), q
        assert got[q][1].astype(np.float64).tolist() == d64[q, ref[q]].tolist(), q


@pytest.mark.parametrize("env,overflow", [
    pytest.param({"WV_SBD_H16_CAND": "64"}, True, id="candidates-overflow-to-the-scan"),
    pytest.param({"WV_SBD_CAP": "128"}, False, id="list-overflow-to-the-per-query-path"),
])
def test_overflow_routes(monkeypatch, env, overflow):
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    base, qs, dead, _, targets, ref, _ = _case("B", "l2-squared", 1303, 5, 260, None, 700)
    ix = _index("l2-squared", base, dead)
    got, got_n, st = _run(ix, True, qs, targets, None, 1303)
    legacy = ix.last_sbd_stats()["legacy_queries"]
    ix.close()
    assert st["key_pass_queries"] == 5
    if overflow:
        assert st["overflow_queries"] > 0 and legacy == 0, st
    else:
        assert legacy > 0   # (701 rows within the target outgrow a 128-entry list: as before the filter)
    assert got_n.tolist() == [len(r) for r in ref]
    for q in range(5):
        assert set(got[q][0].tolist()) == set(ref[q].tolist()), q
