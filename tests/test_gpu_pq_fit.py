"""wv_index_fit_pq on the device against the numpy restatement of
ProductQuantizer.Fit (tests/pq_fit_restatement.py): the fitted table bit for
bit, the passes run per segment and the empty clusters re-seeded; then Compress
end to end against the oracle, and the refusals.  The cases and what each one
reaches: pq_fit_restatement.CASES, checked by tests/test_pq_fit_args.py."""
import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
import pq_fit_restatement as R
from test_pq import _same_tie_aware

WV_EINVAL, WV_ESTATE = 1, 4


def _index(case, **kw):
    ix = W.GPUVectorIndex(case.d, case.metric, capacity=case.n, **kw)
    if case.hole:
        lo, hi = case.hole                        # ids lo..hi-1 never get a vector: position j != id
        ix.upload_vectors(case.base[:lo])
        ix.upload_vectors(case.base[hi:], first_id=hi)
    else:
        ix.upload_vectors(case.base)
    if case.tombstones:                           # cache.all() does not look at tombstones
        dead = np.random.default_rng(99).choice(case.n, case.tombstones, replace=False)
        ix.set_tombstones(dead.tolist())
    return ix


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


@pytest.mark.gpu
@pytest.mark.parametrize("case", R.CASES, ids=[c.name for c in R.CASES])
def test_fit_equals_the_restatement(case):
    want = R.fitted(case)
    ix = _index(case)
    table, iters, reseeded = ix.fit_pq(case.m, case.ks, init=case.init, seed=case.seed)
    print(case.name, "iterations", iters.tolist(), "want", want.iterations.tolist(), "reseeded", reseeded, "want",
          want.reseeded, "table words differing", int((_bits(table) != _bits(want.table)).sum()))
    assert iters.tolist() == want.iterations.tolist()
    assert reseeded == want.reseeded
    assert np.array_equal(_bits(table), _bits(want.table))
    # the index is as set_pq(table) leaves it: encoding gives the oracle's codes of the fitted table
    ix.pq_encode()
    ids = np.nonzero(case.keep)[0]
    got = ix.download_pq_codes(case.n)[ids]
    assert np.array_equal(got.astype(np.int64), R.nearest(case.data, want.table))
    if case.init is None:
        again, it2, rs2 = ix.fit_pq(case.m, case.ks, seed=case.seed)
        assert np.array_equal(_bits(again), _bits(table)) and it2.tolist() == iters.tolist() and rs2 == reseeded
        other, _, _ = ix.fit_pq(case.m, case.ks, seed=case.seed + 1)
        assert not np.array_equal(_bits(other), _bits(table))
    ix.close()


@pytest.mark.gpu
def test_segments_default_to_dim():
    """segments <= 0 means dim (compress.go:54-56)."""
    case = next(c for c in R.CASES if c.name == "tiny")
    want = R.Fit(case.data, case.d, case.ks, seed=case.seed)
    ix = _index(case)
    table, iters, reseeded = ix.fit_pq(0, case.ks, seed=case.seed)
    assert table.shape == (case.d, case.ks, 1)
    assert np.array_equal(_bits(table), _bits(want.table))
    assert iters.tolist() == want.iterations.tolist() and reseeded == want.reseeded
    ix.close()


@pytest.mark.gpu
def test_compress_end_to_end():
    """ix.compress = Compress (compress.go:39-88): the device's codes and its
    compressed flat and HNSW searches against the oracle compressed with the
    restatement's table; the fit lowers the reconstruction error."""
    case = next(c for c in R.CASES if c.name == "collide")
    want = R.fitted(case)
    base, n, d, k = case.base, case.n, case.d, 10
    ref = O.Index(d, case.metric, 16, 64, capacity=n, seed=5)
    ref.add_batch(base, threads=8)
    enc = O.pq_encode_kmeans(base, want.table)
    ref.compress(want.table, enc)
    ix = _index(case, max_connections=16)
    ix.upload_graph(ref.export_graph())
    table, _, _ = ix.compress(case.m, case.ks, seed=case.seed)
    want_codes = np.array([O.pq_extract(enc[r].tobytes(), case.m, case.ks) for r in range(n)], np.uint16)
    assert np.array_equal(ix.download_pq_codes(n), want_codes)
    qs = np.random.default_rng(21).standard_normal((40, d)).astype(np.float32)
    gi, gd, gn = ix.search_batch(qs, k, mode="exact")
    oi, od, on, _ = ref.search_batch(qs, k, 0, mode=1, threads=8)
    for i in range(len(qs)):
        _same_tie_aware(gi[i, : gn[i]], gd[i, : gn[i]], oi[i, : on[i]], od[i, : on[i]])
    gi, gd, gn = ix.search_batch(qs, k, ef=64, mode="hnsw")
    oi, od, on, _ = ref.search_batch(qs, k, 64, threads=8)
    for i in range(len(qs)):
        _same_tie_aware(gi[i, : gn[i]], gd[i, : gn[i]], oi[i, : on[i]], od[i, : on[i]])
    before, after = R.reconstruction_error(base, want.initial), R.reconstruction_error(base, table)
    print("reconstruction error ratio %.3f" % (after / before))
    assert after < before
    ix.close()


@pytest.mark.gpu
def test_refusals_leave_the_index_alone():
    rng = np.random.default_rng(8)
    n, d, m, ks = 300, 16, 4, 16
    base = rng.standard_normal((n, d)).astype(np.float32)
    qs = rng.standard_normal((8, d)).astype(np.float32)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    table, _, _ = ix.compress(m, ks, seed=1)

    def state():
        ids, ds, cnt = ix.search_batch(qs, 5, mode="exact")
        return ix.download_pq_codes(n).copy(), ids.copy(), ds.view(np.uint32).copy(), cnt.copy()

    s0 = state()
    with pytest.raises(W.WvError) as e:            # compressed: switch it off first
        ix.fit_pq(m, ks, seed=2)
    assert e.value.code == WV_ESTATE and "wv_index_fit_pq" in str(e.value)
    assert all(np.array_equal(a, b) for a, b in zip(s0, state()))
    ix.set_compressed(False)
    with pytest.raises(W.WvError) as e:            # "Too few data to fit KMeans"
        ix.fit_pq(m, 512, seed=2)
    assert e.value.code == WV_ESTATE and "wv_index_fit_pq" in str(e.value)
    ix.set_compressed(True)                        # the quantizer and every row's code are still there
    assert all(np.array_equal(a, b) for a, b in zip(s0, state()))
    ix.set_compressed(False)
    for bad_segments in (3, 5):                    # not dividing 16
        assert W.lib().wv_index_fit_pq(ix._h, bad_segments, ks, 0, None, 0, None, None, None) == WV_EINVAL
        assert "wv_index_fit_pq" in W.lib().wv_last_error().decode()
        with pytest.raises(W.WvError) as e:
            ix.fit_pq(bad_segments, ks)
        assert e.value.code == WV_EINVAL
    for bad_ks in (1, 65537):
        assert W.lib().wv_index_fit_pq(ix._h, m, bad_ks, 0, None, 0, None, None, None) == WV_EINVAL
    ix.set_compressed(True)
    assert all(np.array_equal(a, b) for a, b in zip(s0, state()))
    ix.close()
