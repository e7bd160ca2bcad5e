"""The D <= 128 f16 key pass's cross-slot exchange (wv_bf_h16_kernel, XS):
heads published at 1/16 and at every eighth of a segment, sorted by one slot
in four, and the published thresholds returned to every slot once per tile
group through an LDS-DMA of the wave's gtau words.

Thresholds only ever drop keys above a certified bound, so every case must
equal the CPU restatement (tie-aware), the same call with WV_H16_XSLOT=0 bit
for bit, and the fp32 pass (WV_BF_FP32=1) bit for bit.  The `shapes` fixture
restates bf_schedule and asserts, before any launch, what each shape is there
for.  Runs on an MI355X (-m gpu).
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
BQ, TILE, TPS = 512, 64, 3   # queries per block, corpus rows per tile, tiles per stage group
SEED_MIN_TILES = 1024        # corpora of fewer tiles run without the seed pre-pass

ENGAGED = (70001, 16 * BQ + 1)   # 1 094 tiles (seeded), 17 query blocks
COLLAPSED = (10240, 8300)        # 160 tiles (no seed), 17 query blocks, 44 live columns in the last wave
SMALL = (20000, 8300)            # 313 tiles (no seed), 17 query blocks


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


def schedule(rows, nq, blocks):
    """bf_schedule restated: the (query block, tile) units qb * ntiles + tile
    are cut into runs of U = ceil(nqb * ntiles / blocks).  Returns the slots
    per query block and, per block, its segments as (query block, tiles)."""
    nqb = (nq + BQ - 1) // BQ
    ntiles = (rows + TILE - 1) // TILE
    total = nqb * ntiles
    nb = min(blocks, total)
    u_run = (total + nb - 1) // nb
    n_slots = (ntiles + u_run - 1) // u_run + 1
    segs = []
    for b in range((total + u_run - 1) // u_run):
        u, u_last = b * u_run, min((b + 1) * u_run, total)
        mine = []
        while u < u_last:
            t0 = u % ntiles
            t1 = min(t0 + (u_last - u), ntiles)
            mine.append((u // ntiles, t1 - t0))
            u += t1 - t0
        segs.append(mine)
    return n_slots, ntiles, segs


def publish_points(ntile):
    """The exchange tiles of a segment: 1/16, then every eighth to 7/8."""
    return [ntile // 16] + [i * ntile // 8 for i in range(1, 8)]


@pytest.fixture(scope="module")
def shapes():
    """Before any launch: every shape reaches the code it is there for."""
    import torch
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    out = {}
    for name, (rows, nq) in (("engaged", ENGAGED), ("collapsed", COLLAPSED), ("small", SMALL)):
        n_slots, ntiles, segs = schedule(rows, nq, cus)
        # the exchange engages: <= 32 list heads per query, and k of them exist
        k_max = 32 if name == "engaged" else 10
        assert k_max <= 2 * n_slots <= 32, (name, n_slots)
        out[name] = (n_slots, ntiles, segs)
    n_slots, ntiles, segs = out["engaged"]
    assert ntiles >= SEED_MIN_TILES   # the seeded path, at every stride
    # some block goes from one query block to the next with more than a tile
    # group of each: its refresh slot and thresholds change query block
    assert any(len(m) >= 2 and m[0][0] != m[1][0] and min(m[0][1], m[1][1]) > TPS for m in segs), segs[:20]
    n_slots, ntiles, segs = out["collapsed"]
    assert ntiles == 160 and ntiles < SEED_MIN_TILES
    assert (COLLAPSED[1] + BQ - 1) // BQ == 17 and COLLAPSED[1] % 64 == 44
    lens = {n for m in segs for _, n in m}
    assert max(lens) <= 12, sorted(lens)
    assert any(len(set(publish_points(n))) < 8 for n in lens if n > TPS), sorted(lens)
    assert out["small"][1] < SEED_MIN_TILES
    return out


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


def _check(base, qs, metric=O.L2, ks=(10,), tomb=None, allow_ids=None, env=None, twice=False):
    """Exact batches (one per k) with the exchange on: against the same calls
    with WV_H16_XSLOT=0 and through the fp32 pass, bit for bit, and against
    the restatement, tie-aware."""
    n, d = base.shape
    al = W.AllowList.from_ids(allow_ids, n) if allow_ids is not None else None

    def index():
        ix = W.GPUVectorIndex(d, METRIC_NAMES[metric], capacity=n)
        ix.upload_vectors(base)
        if tomb is not None:
            ix.set_tombstones(tomb)
        return ix

    with _env(**(env or {})):
        assert os.environ.get("WV_H16_XSLOT", "1") != "0"
        ix = index()
        got = [ix.search_batch(qs, k, allow=al, mode="exact") for k in ks]
        if twice:   # stale refresh-slot, gslot or gtau contents of an earlier batch would show here
            for k, g in zip(ks, got):
                again = ix.search_batch(qs, k, allow=al, mode="exact")
                same(g[0], g[1], again[0], again[1])
                assert g[2].tolist() == again[2].tolist()
        with _env(WV_H16_XSLOT="0"):
            off = [ix.search_batch(qs, k, allow=al, mode="exact") for k in ks]
        ix.close()
        with _env(WV_BF_FP32="1"):   # (the pass is chosen when the index is made)
            ix = index()
            ref32 = [ix.search_batch(qs, k, allow=al, mode="exact") for k in ks]
            ix.close()
    b, q = (_unit(base), _unit(qs)) if metric == O.COSINE else (base, qs)
    for k, g, o, r in zip(ks, got, off, ref32):
        for other in (o, r):
            same(g[0], g[1], other[0], other[1])
            assert g[2].tolist() == other[2].tolist()
        oi, od, on = O.flat_scan(metric, b, q, k, allow_bits=al.words if al is not None else None,
                                 tomb_bits=O.bits_from_ids(tomb, n) if tomb is not None else None, threads=16)
        ids, ds, cnt = g
        assert cnt.tolist() == on.tolist()
        for i in range(len(qs)):
            same_tie_aware(ids[i, : cnt[i]], ds[i, : cnt[i]], oi[i, : on[i]], od[i, : on[i]])


def test_engaged_over_two_query_blocks(shapes):
    """k = 10 and 32, each twice on one index."""
    rows, nq = ENGAGED
    base, qs = _data(rows, 16, nq, seed=21)
    _check(base, qs, ks=(10, 32), twice=True)


def test_collapsed_publish_points(shapes):
    rows, nq = COLLAPSED
    base, qs = _data(rows, 128, nq, seed=22)
    _check(base, qs)


@pytest.mark.parametrize("stride", [8, 16, 32, 64])
def test_seed_strides(shapes, stride):
    rows, nq = ENGAGED
    base, qs = _data(rows, 16, nq, seed=23)
    _check(base, qs, env={"WV_H16_SAMPLE": str(stride)})


def test_dot_with_tombstones_after_a_clean_prefix(shapes):
    rows, nq = SMALL
    base, qs = _data(rows, 100, nq, seed=24, metric=O.DOT)
    rng = np.random.default_rng(25)
    tomb = (2 * rows // 3 + np.nonzero(rng.random(rows - 2 * rows // 3) < 0.01)[0]).astype(np.uint64)
    _check(base, qs, metric=O.DOT, tomb=tomb)


def test_cosine_with_shared_allow_list(shapes):
    """60 % of the rows allowed for every query: the masked scan."""
    rows, nq = SMALL
    base, qs = _data(rows, 100, nq, seed=26, metric=O.COSINE)
    allow = np.nonzero(np.random.default_rng(27).random(rows) < 0.6)[0]
    _check(base, qs, metric=O.COSINE, allow_ids=allow)


@pytest.mark.parametrize("dim,metric", [(16, O.L2), (48, O.L2), (16, O.DOT), (48, O.DOT)])
def test_short_k_steps(shapes, dim, metric):
    """One and three k-steps per half, with and without the norm word: the
    refresh entry lands in another k-step of the fill burst."""
    rows, nq = SMALL
    base, qs = _data(rows, dim, nq, seed=28 + dim, metric=metric)
    _check(base, qs, metric=metric)
