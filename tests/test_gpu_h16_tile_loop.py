"""The D <= 128 f16 key pass's tile loop (wv_bf_h16_kernel): running tile
state, fill bursts issued between the MFMAs, group barriers.

It can go wrong where a block's segments are short, end inside a stage group,
wrap with the per-query-block rotation, or change query block.  The shapes
below are the smallest that reach those points; every case is checked against
the CPU restatement (tie-aware) and bit for bit against the same call through
the fp32 pass (WV_BF_FP32=1).  Runs on an MI355X (-m gpu).
"""
import contextlib
import os

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from helpers import same, same_tie_aware

pytestmark = pytest.mark.gpu

METRIC_NAMES = {O.L2: "l2-squared", O.DOT: "dot", O.COSINE: "cosine-dot"}
BQ, TILE = 512, 64   # queries per block, corpus rows per tile


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update(kv)
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def segment_lengths(rows, nq, blocks):
    """bf_schedule restated: the (query block, tile) units qb * ntiles + tile
    are cut into runs of U = ceil(nqb * ntiles / blocks); a block scans its run
    in segments that end at query-block ends."""
    nqb = (nq + BQ - 1) // BQ
    ntiles = (rows + TILE - 1) // TILE
    total = nqb * ntiles
    nb = min(blocks, total)
    u_run = (total + nb - 1) // nb
    out = set()
    for b in range((total + u_run - 1) // u_run):
        u, u_last = b * u_run, min((b + 1) * u_run, total)
        while u < u_last:
            t0 = u % ntiles
            t1 = min(t0 + (u_last - u), ntiles)
            out.add(t1 - t0)
            u += t1 - t0
    return out


# (rows, nq, dim): rows 63 / 64 / 65, counts that are no multiple of 64, one,
# two and three query blocks, D = 16 (one k-step), 100 (seven) and 128
SEGMENT_CASES = [(63, 1, 128), (64, 1, 128), (65, 513, 128), (33000, 1100, 128), (70001, 1100, 128),
                 (65536, 1100, 16), (71000, 1100, 100)]


@pytest.fixture(scope="module")
def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def covered(cu_count):
    """Before any launch: the cases' segments have every length 1 .. 7 and a
    length >= 12 of each residue mod 3 (a stage group is 3 tiles)."""
    lens = set()
    for rows, nq, _ in SEGMENT_CASES:
        lens |= segment_lengths(rows, nq, cu_count)
    assert set(range(1, 8)) <= lens, sorted(lens)
    assert {n % 3 for n in lens if n >= 12} == {0, 1, 2}, sorted(lens)
    return lens


def _data(n, d, nq, seed, metric=O.L2):
    rng = np.random.default_rng(seed)
    base = rng.random((n, d), dtype=np.float32)
    qs = rng.random((nq, d), dtype=np.float32)
    if metric != O.L2:
        base -= 0.5
        qs -= 0.5
    return base, qs


def _unit(a):
    return np.stack([O.normalize(r) for r in a])


def _check(base, qs, metric=O.L2, k=10, tomb=None, allow_ids=None, env=None, also=None, twice=False):
    """One exact batch against the restatement and against the fp32 pass;
    `also`: a switch under which the answer must not change by a bit."""
    n, d = base.shape
    al = W.AllowList.from_ids(allow_ids, n) if allow_ids is not None else None

    def index():
        ix = W.GPUVectorIndex(d, METRIC_NAMES[metric], capacity=n)
        ix.upload_vectors(base)
        if tomb is not None:
            ix.set_tombstones(tomb)
        return ix

    with _env(**(env or {})):
        ix = index()
        got = ix.search_batch(qs, k, allow=al, mode="exact")
        if twice:   # stale stage contents of an earlier segment would show here
            again = ix.search_batch(qs, k, allow=al, mode="exact")
            same(got[0], got[1], again[0], again[1])
            assert got[2].tolist() == again[2].tolist()
        other = None
        if also:
            with _env(**also):
                other = ix.search_batch(qs, k, allow=al, mode="exact")
        ix.close()
        with _env(WV_BF_FP32="1"):   # (the pass is chosen when the index is made)
            ix = index()
            ref32 = ix.search_batch(qs, k, allow=al, mode="exact")
            ix.close()
    for r in (ref32, other):
        if r is not None:
            same(got[0], got[1], r[0], r[1])
            assert got[2].tolist() == r[2].tolist()
    b, q = (_unit(base), _unit(qs)) if metric == O.COSINE else (base, qs)
    oi, od, on = O.flat_scan(metric, b, q, k, allow_bits=al.words if al is not None else None,
                             tomb_bits=O.bits_from_ids(tomb, n) if tomb is not None else None, threads=16)
    ids, ds, cnt = got
    assert cnt.tolist() == on.tolist()
    for i in range(len(qs)):
        same_tie_aware(ids[i, : cnt[i]], ds[i, : cnt[i]], oi[i, : on[i]], od[i, : on[i]])


@pytest.mark.parametrize("rows,nq,dim", SEGMENT_CASES)
def test_segment_lengths(covered, rows, nq, dim):
    base, qs = _data(rows, dim, nq, seed=rows + nq)
    _check(base, qs, twice=rows == 70001)


@pytest.mark.parametrize("metric", [O.DOT, O.COSINE])
def test_metrics_without_the_norm_word(metric):
    base, qs = _data(20000, 128, 513, seed=7, metric=metric)
    _check(base, qs, metric=metric)


def test_seed_pre_pass_with_another_stride():
    """tile_stride > 1 and the sampled range's own tile count (default stride:
    the 70 001-row cases above)."""
    base, qs = _data(70001, 128, 513, seed=8)
    _check(base, qs, env={"WV_H16_SAMPLE": "8"})


def test_tombstones_after_a_clean_prefix():
    n = 33000
    base, qs = _data(n, 128, 513, seed=9)
    rng = np.random.default_rng(10)
    tomb = (2 * n // 3 + np.nonzero(rng.random(n - 2 * n // 3) < 0.02)[0]).astype(np.uint64)
    _check(base, qs, tomb=tomb)


def test_shared_allow_list_masked_scan():
    n = 33000
    base, qs = _data(n, 128, 513, seed=11)
    allow = np.nonzero(np.random.default_rng(12).random(n) < 0.6)[0]
    _check(base, qs, allow_ids=allow)


def test_cross_slot_instantiation(cu_count):
    """17 query blocks over 70 001 rows: at most 16 slots per query block, so
    the pass with the cross-slot threshold runs; switching it off changes no
    bit."""
    rows, nq = 70001, 16 * BQ + 1
    nqb, ntiles = 17, (rows + TILE - 1) // TILE
    u_run = -(-nqb * ntiles // cu_count)
    assert 2 * (-(-ntiles // u_run) + 1) <= 32
    base, qs = _data(rows, 16, nq, seed=13)
    _check(base, qs, also={"WV_H16_XSLOT": "0"})
