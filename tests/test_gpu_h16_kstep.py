"""The D <= 128 f16 key pass's fill hooks (wv_bf_h16_kernel): a tile's LDS-DMA
entries and the threshold refresh sit at fixed k-steps of the two halves behind
a group barrier, and one scalar word says which of them the tile runs.

Where an entry sits depends on the number of k-steps (D = 16, 32, 48, 100, 128:
3 / 2 / 1 / 1 / 1 entries per k-step, with or without entries left for the
second half), on the burst's length (a segment's last group may be partial) and
on the wave.  A misplaced, dropped or repeated entry leaves a stage with
another tile's rows, so every case is checked against the CPU restatement
(tie-aware) and bit for bit against the same call through the fp32 pass
(WV_BF_FP32=1).  Runs on an MI355X (-m gpu).
"""
import numpy as np
import pytest

import pyoracle as O
from test_gpu_h16_tile_loop import BQ, TILE, _check, _data, segment_lengths

pytestmark = pytest.mark.gpu

DIMS = [16, 32, 48, 100, 128]
# (rows, nq) per test below: 17 query blocks (the cross-slot instantiation),
# three, two and one, the last block partial in each
XS_SHAPE = (20001, 16 * BQ + 1)
SHORT_SHAPE = (33000, 1100)
SEED_SHAPE = (70001, 513)    # >= 1,024 tiles: the seed pre-pass runs
MASK_SHAPE = (33000, 513)
DOT_SHAPE = (20000, 300)
SHAPES = [XS_SHAPE, SHORT_SHAPE, SEED_SHAPE, MASK_SHAPE, DOT_SHAPE]


@pytest.fixture(scope="module")
def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.fixture(scope="module")
def covered(cu_count):
    """Before any launch: the shapes (the same at every D) give segments of
    every length 1 .. 7 and a length >= 12 of each residue mod 3 (a stage group
    is 3 tiles), and the 17-block shape meets the cross-slot exchange's
    conditions (at most 16 slots per query block, k = 10 <= two lists per
    slot)."""
    lens = set()
    for rows, nq in SHAPES:
        lens |= segment_lengths(rows, nq, cu_count)
    assert set(range(1, 8)) <= lens, sorted(lens)
    assert {n % 3 for n in lens if n >= 12} == {0, 1, 2}, sorted(lens)
    rows, nq = XS_SHAPE
    nqb, ntiles = -(-nq // BQ), -(-rows // TILE)
    u_run = -(-nqb * ntiles // cu_count)
    assert 10 <= 2 * (ntiles // u_run) and 2 * (-(-ntiles // u_run) + 1) <= 32
    assert -(-SEED_SHAPE[0] // TILE) >= 1024
    return lens


@pytest.mark.parametrize("dim", DIMS)
def test_default_path_with_the_refresh_hook(covered, dim):
    """Cross-slot exchange on (the refresh entry behind the fills'); switching
    it off changes no bit."""
    rows, nq = XS_SHAPE
    base, qs = _data(rows, dim, nq, seed=100 + dim)
    _check(base, qs, also={"WV_H16_XSLOT": "0"})


@pytest.mark.parametrize("dim", DIMS)
def test_short_segments_same_batch_twice(covered, dim):
    """Three query blocks, segments of 1 .. 7 tiles: bursts shorter than a
    group, and hook state left by the batch before."""
    rows, nq = SHORT_SHAPE
    base, qs = _data(rows, dim, nq, seed=200 + dim)
    _check(base, qs, twice=True)


@pytest.mark.parametrize("dim", DIMS)
def test_seeded_and_unseeded(covered, dim):
    """>= 1,024 tiles: the seed pre-pass (the kernel's SEED instantiation, with
    a tile stride) and the seeded main pass; WV_H16_NO_SEED=1 runs the main
    pass with the running threshold instead and changes no bit."""
    rows, nq = SEED_SHAPE
    base, qs = _data(rows, dim, nq, seed=300 + dim)
    _check(base, qs, also={"WV_H16_NO_SEED": "1"})


@pytest.mark.parametrize("dim", DIMS)
def test_masked_tiles_while_a_burst_is_live(covered, dim):
    """A shared allow list and tombstones: every tile takes the mask path,
    the tiles that carry a burst included."""
    rows, nq = MASK_SHAPE
    base, qs = _data(rows, dim, nq, seed=400 + dim)
    rng = np.random.default_rng(500 + dim)
    allow = np.nonzero(rng.random(rows) < 0.6)[0]
    tomb = np.nonzero(rng.random(rows) < 0.02)[0].astype(np.uint64)
    _check(base, qs, allow_ids=allow, tomb=tomb)


@pytest.mark.parametrize("dim", DIMS)
def test_dot_without_the_norm_word(covered, dim):
    """dot: a tile has no s|x|^2 entry, so its last entry is an image op (one
    partial query block)."""
    rows, nq = DOT_SHAPE
    base, qs = _data(rows, dim, nq, seed=600 + dim, metric=O.DOT)
    _check(base, qs, metric=O.DOT)
