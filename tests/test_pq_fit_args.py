"""wv_index_fit_pq: present in the ABI and the binding, refuses a null index,
and the GPU test's cases reach the branches they are there for (no GPU needed:
the restatement alone runs here)."""
import numpy as np

import weaviate_amd as W
import pq_fit_restatement as R


def test_symbol_exists():
    assert hasattr(W.lib(), "wv_index_fit_pq")
    assert "wv_index_fit_pq" in W.header_symbols()
    assert hasattr(W.GPUVectorIndex, "fit_pq")
    assert hasattr(W.GPUVectorIndex, "compress")


def test_needs_an_index():
    assert W.lib().wv_index_fit_pq(None, 8, 256, 0, None, 0, None, None, None) == 1
    assert "wv_index_fit_pq" in W.lib().wv_last_error().decode()


def test_draws_are_in_range_and_counter_based():
    assert R.mix64(0) == 0
    seen = {R.draw(3, s, i, ci, a, 1000) for s in (0, 5) for i in (0, 15) for ci in (0, 255) for a in (0, 63)}
    assert all(0 <= j < 1000 for j in seen) and len(seen) > 8
    assert R.draw(3, 1, 2, 3, 4, 1000) == R.draw(3, 1, 2, 3, 4, 1000)


def test_cases_reach_their_branches():
    """What keeps tests/test_gpu_pq_fit.py from passing vacuously."""
    fits = {c.name: R.fitted(c) for c in R.CASES}
    for c in R.CASES:
        f = fits[c.name]
        print(c.name, f.iterations.tolist(), f.reseeded, f.ended)
        assert f.table.shape == (c.m, c.ks, c.d // c.m) and np.isfinite(f.table).all()
        assert ((1 <= f.iterations) & (f.iterations <= 11)).all()
    assert fits["collide"].reseeded > 0            # drawn centres collide: an empty cluster gets a donor
    assert fits["ds32-dup-init"].reseeded > 0      # centre 3 = centre 7: the last of equals wins, 3 is empty
    assert any(e == "cap" and it == 11 for f in fits.values() for e, it in zip(f.ended, f.iterations))
    assert 11 in fits["ds1-cap"].iterations.tolist()
    assert any(e == "delta" for f in fits.values() for e in f.ended)
    assert "settled" in fits["tiny"].ended        # 1 % of 60 rows truncates to 0: runs to changes == 0
    assert len(set(fits["clustered"].iterations.tolist())) > 1   # segments stop at different rounds
    # the 128 KiB of centres of "chunks" is two LDS chunks on the device
    c = next(c for c in R.CASES if c.name == "chunks")
    assert c.ks * (c.d // c.m) * 4 > 64 << 10


def test_fitting_lowers_the_reconstruction_error():
    """The restatement's ratio is below 1 on every case, so the GPU test's
    assertion can fail only through the device code."""
    for c in R.CASES:
        f = R.fitted(c)
        before, after = R.reconstruction_error(c.data, f.initial), R.reconstruction_error(c.data, f.table)
        print(c.name, "ratio %.3f" % (after / before))
        assert after < before


def test_a_different_seed_is_a_different_fit():
    c = next(c for c in R.CASES if c.name == "tiny")
    a, b = R.fitted(c), c.fit(seed=c.seed + 1)
    assert not np.array_equal(a.table.view(np.uint32), b.table.view(np.uint32))
    assert np.array_equal(a.table.view(np.uint32), c.fit().table.view(np.uint32))
