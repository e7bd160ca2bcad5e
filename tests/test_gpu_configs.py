"""Parity at the BASELINE configs' own parameters (-m gpu).

Each test runs the HIP path through the C ABI at the graph / data shape a
headline number is quoted on, scaled down so the CPU restatement (oracle/)
finishes in seconds:

  configs[0]  SIFT-shaped 128-d L2, hnsw M=64 (layer-0 degree 128 fills the
              kernel's 128-slot neighbour batch), efConstruction=128, ef=64
  configs[2]  GloVe-shaped 100-d cosine (ldx 128 vs dpad 100), ef 128 / 256
              (the largest LDS beams, the visited cache squeezed)
  configs[4]  Deep-shaped 96-d L2, two id-range shards with their own graphs,
              merged on the device (index.go:967-1044)
  configs[3]/(e)  two processes on the GPU, each searching its shard through
              libwvgpu.so, all-gathered (gloo) and merged by the device kernel:
              identical to one search of the whole corpus

plus SearchByVector's dispatch (flat vs HNSW by flatSearchCutoff,
search.go:64-79) and searchTimeEF's default ef through the ABI.
"""
import os
import socket

import numpy as np
import pytest

import pyoracle as O
import weaviate_amd as W
from bench import counter_gauss, counter_glove, counter_sift, counter_uniform
from helpers import merge_lists, recall, same, same_tie_aware, tie_aware_equal
from helpers import unexplained as _unexplained, unexplained_filtered as _unexplained_filtered

pytestmark = pytest.mark.gpu

THREADS = 16


def test_configs0_gpu_built_graph_recall_vs_sequential_build():
    """north_star: HNSW recall@10 within 0.5 pt of the *reference* index on
    identical data and ef -- the reference builds its graph by inserting one
    node at a time (insert.go:103-217), here the restatement's build; the GPU
    serves a graph it built itself in batches (wv_index_build_graph).  At
    configs[0]'s parameters (SIFT-shaped 128-d, M=64, efConstruction=128,
    ef=64), scaled to 100k rows; bench.py --seq-build reports the same at 1M."""
    n, d, nq, k, ef = 100_000, 128, 1000, 10, 64
    base = counter_sift(1, 0, n, d)
    qs = counter_sift(2, 0, nq, d)
    truth, _, _ = O.flat_scan(O.L2, base, qs, k, threads=THREADS)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=64)
    ix.upload_vectors(base)
    ix.build_graph(ef_construction=128, seed=1, batch_div=64)
    gi, gd, gn = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    ref = O.Index(d, "l2-squared", 64, 128, capacity=n, seed=1)
    ref.add_batch(base, threads=THREADS)
    oi, od, on, _ = ref.search_batch(qs, k, ef, threads=THREADS)
    r_gpu, r_ref = recall(gi, truth), recall(oi, truth)
    # and the GPU searching the restatement's own graph answers as the restatement does
    ix.upload_graph(ref.export_graph())
    si, sd, sn = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    ix.close()
    print(f"recall@10 GPU-built {r_gpu:.4f}, sequential build {r_ref:.4f}, GPU on the sequential graph "
          f"{recall(si, truth):.4f}")
    assert abs(r_gpu - r_ref) <= 0.005, (r_gpu, r_ref)
    assert abs(recall(si, truth) - r_ref) <= 0.001


def test_configs0_sift_hnsw_m64_efc128_ef64():
    """configs[0]: maxConnections=64 -> layer-0 lists of up to 128 ids, two per
    lane of the neighbour batch; recall within 0.5 pt of the restatement."""
    n, d, nq, k, ef = 24000, 128, 600, 10, 64
    base = counter_sift(1, 0, n, d)
    qs = counter_sift(2, 0, nq, d)
    ref = O.Index(d, "l2-squared", 64, 128, capacity=n, seed=1)
    ref.add_batch(base, threads=THREADS)
    g = ref.export_graph()
    assert g["deg0"] == 128 and int(g["counts0"].max()) > 64   # rows longer than one lane's slot
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=64)
    ix.upload_vectors(base)
    ix.upload_graph(g)
    gi, gd, gn = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    oi, od, on, _ = ref.search_batch(qs, k, ef, threads=THREADS)
    assert gn.tolist() == on.tolist()
    assert not _unexplained(ref, qs, k, ef, gi, gd, oi, od)
    truth, _, _ = O.flat_scan(O.L2, base, qs, k, threads=THREADS)
    r_gpu, r_cpu = recall(gi, truth), recall(oi, truth)
    assert abs(r_gpu - r_cpu) <= 0.005, (r_gpu, r_cpu)
    assert r_gpu >= 0.95, r_gpu
    ix.close()


def _variants_identical(ix, qs, k, ef, allow, ref_out, monkeypatch):
    """Every launch variant of the side-register path answers bit for bit as
    the default one: one wave per query (no workgroup launch), the exact
    visited bitmap forced on / off for the first pass (off: overflows re-run
    exactly)."""
    gi, gd, gn = ref_out
    for key, val in (("WV_HNSW_WG_MAX", "0"), ("WV_HNSW_EV_BELOW", "0"), ("WV_HNSW_EV_BELOW", "2")):
        monkeypatch.setenv(key, val)
        vi, vd, vn = ix.search_batch(qs, k, ef=ef, allow=allow, mode="hnsw")
        monkeypatch.delenv(key)
        assert np.array_equal(vn, gn), (key, val)
        assert np.array_equal(vi, gi) and np.array_equal(vd.view(np.uint32), gd.view(np.uint32)), (key, val)


@pytest.mark.parametrize("frac", [0.01, 0.1, 0.5])
def test_filtered_hnsw_selective_list_parity_and_fallback_rate(frac, monkeypatch):
    """Filtered HNSW (search.go:74-78 with |allow| >= flatSearchCutoff or
    forbidFlat; the list applied at layer 0, :282-298) on the configs[0]
    graph shape at 1 %, 10 % and 50 % of the rows: the traversal keeps every
    ineligible node with d <= worst as a side candidate (the live ones peak
    near 1.4 ef (1-p)/p: ~900 at 10 %, ~9k at 1 %).  The side-register path
    keeps an exact layer-0 visited bitmap in HBM and the side set's smallest
    keys in LDS (the rest spilled to HBM), sized from the list's selectivity;
    every query's answer equals the restatement's knnSearchByVector with the
    list (up to tie order, or a tie-dependent decision the restatement
    reports), or -- only for a query the device reported as overflowed and
    answered exactly -- flatSearch's.  No unexplained difference."""
    import bench
    n, d, nq, k, ef = 100_000, 128, 500 if frac > 0.05 else 200, 10, 64
    base = counter_sift(1, 0, n, d)
    qs = counter_sift(2, 0, nq, d)
    ref = O.Index(d, "l2-squared", 64, 128, capacity=n, seed=1)
    ref.add_batch(base, threads=THREADS)
    a = type("A", (), {"allow_frac": frac})()
    words, n_allowed = bench._allow_words(a, 0, n)
    allow = W.AllowList.from_ids(np.nonzero(counter_uniform(3, 0, n, 1)[:, 0] < frac)[0], n)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=64)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    gi, gd, gn = ix.search_batch(qs, k, ef=ef, allow=allow, mode="hnsw")
    st = ix.last_batch_stats()
    ss = ix.last_side_stats()
    _variants_identical(ix, qs, k, ef, allow, (gi, gd, gn), monkeypatch)
    oi, od, on, ost = ref.search_batch(qs, k, ef, allow=words, threads=THREADS)
    ix.close()
    fb = st["fallbacks"]
    bad, flat = _unexplained_filtered(ref, qs, k, ef, words, gi, gd, gn, oi, od, on)
    print(f"allow {frac:.0%} ({n_allowed} rows): side array {ss['side_rows']} x 64, spill {ss['spill_cap']}, "
          f"overflowed {ss['overflowed']}, redone {ss['redone']}, exact fallbacks {fb} of {nq}; GPU evaluations "
          f"{st['dist_evals'] / nq:.0f} vs the restatement's {ost['dist_evals'] / nq:.0f} per query")
    assert ss["side_rows"] > 0   # (the side-register path ran)
    assert not bad, bad[:10]
    assert len(flat) <= fb, (len(flat), fb)
    # no query overflows; below 40 % eligible (the exact layer-0 visited
    # list) the GPU evaluates what the restatement evaluates (the upper
    # levels' lossy cache aside), above it the lossy cache re-evaluates some
    assert fb == 0 and ss["overflowed"] == 0, (fb, ss)
    bound = 1.02 if frac < 0.4 else 1.3
    assert st["dist_evals"] <= bound * ost["dist_evals"], (st["dist_evals"], ost["dist_evals"])


@pytest.mark.parametrize("tomb_frac", [0.01, 0.2])
def test_tombstoned_hnsw_side_register_path(tomb_frac, monkeypatch):
    """Tombstones (delete.go:546-551) make nodes ineligible but traversed
    (search.go:294-296, :347-349) at every level: an unfiltered search of a
    shard with tombstones runs the side-register path (results in
    registers); answers equal the restatement's with the same tombstones."""
    n, d, nq, k, ef = 60_000, 128, 400, 10, 64
    base = counter_sift(1, 0, n, d)
    qs = counter_sift(2, 0, nq, d)
    ref = O.Index(d, "l2-squared", 64, 128, capacity=n, seed=1)
    ref.add_batch(base, threads=THREADS)
    g = ref.export_graph()
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=64)
    ix.upload_vectors(base)
    ix.upload_graph(g)
    rng = np.random.default_rng(11)
    ep = int(g["entrypoint"])
    dead = [int(x) for x in rng.choice(n, int(tomb_frac * n), replace=False) if int(x) != ep]
    for t in dead:
        ref.add_tombstone(t)
    ix.add_tombstones(dead)
    for ef_ in (ef, 128):
        gi, gd, gn = ix.search_batch(qs, k, ef=ef_, mode="hnsw")
        ss = ix.last_side_stats()
        _variants_identical(ix, qs, k, ef_, None, (gi, gd, gn), monkeypatch)
        oi, od, on, _ = ref.search_batch(qs, k, ef_, threads=THREADS)
        assert ss["side_rows"] > 0
        returned = {int(x) for i in range(nq) for x in gi[i][:gn[i]]}
        assert not returned & set(dead)
        assert gn.tolist() == on.tolist()
        assert not _unexplained(ref, qs, k, ef_, gi, gd, oi, od)
    ix.close()


def test_exact_visited_counts_equal_restatement(monkeypatch):
    """The configs[4] line's byte basis (E and X of the reference's
    traversal) is measured on the GPU where the corpus is too large to restate
    on the host: WV_HNSW_UNIQUE_COUNTS counts each node's layer-0 evaluation
    once (an exact per-query visited bitmap beside the lossy LDS cache, as the
    reference's visited list, search.go:256-264).  On a graph the restatement
    also searches, those counts equal the restatement's E and X -- with the
    visited cache squeezed so that the GPU re-evaluates."""
    n, d, nq, k, ef = 24000, 96, 300, 10, 64
    base = counter_sift(1, 0, n, d)
    qs = counter_sift(2, 0, nq, d)
    ref = O.Index(d, "l2-squared", 64, 128, capacity=n, seed=1)
    ref.add_batch(base, threads=THREADS)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=64)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    oi, od, on, ost = ref.search_batch(qs, k, ef, threads=THREADS)
    monkeypatch.setenv("WV_HNSW_WAVE_KB", "6")   # a small visited cache: re-evaluations
    gi, gd, gn = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    lossy = ix.last_batch_stats()
    monkeypatch.setenv("WV_HNSW_UNIQUE_COUNTS", "1")
    ui, ud, un = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    exact = ix.last_batch_stats()
    ix.close()
    same(ui, ud, gi, gd)   # counting changes nothing in the search
    assert not _unexplained(ref, qs, k, ef, gi, gd, oi, od)
    print(f"E per query: restatement {ost['dist_evals'] / nq:.1f}, GPU lossy {lossy['dist_evals'] / nq:.1f}, "
          f"GPU exact-visited {exact['dist_evals'] / nq:.1f}; X {ost['expansions'] / nq:.1f} / "
          f"{exact['expansions'] / nq:.1f}")
    assert lossy["dist_evals"] > ost["dist_evals"]   # the squeezed cache did re-evaluate
    assert abs(exact["expansions"] - ost["expansions"]) <= 0.001 * ost["expansions"]
    assert abs(exact["dist_evals"] - ost["dist_evals"]) <= 0.001 * ost["dist_evals"]


@pytest.mark.parametrize("ef", [64, 128, 256])
def test_configs2_glove_cosine_d100_large_ef(ef):
    """configs[2]: 100-d cosine (stored rows normalized on upload, queries
    per search) on the bench's GloVe-shaped generator (bench.py
    counter_glove: Zipf-sized clusters in a 24-d latent family, full-rank
    residual, log-normal norms), ef across the sweep: ids and distances as
    the restatement's, and the recall operating point the bench reports."""
    n, d, nq, k = 20000, 100, 300, 10
    base = counter_glove(1, 0, n, d)
    qs = counter_glove(2, 0, nq, d)
    ref = O.Index(d, "cosine-dot", 32, 128, capacity=n, seed=2)
    ref.add_batch(base, threads=THREADS)
    ix = W.GPUVectorIndex(d, "cosine-dot", capacity=n, max_connections=32)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    gi, gd, gn = ix.search_batch(qs, k, ef=ef, mode="hnsw")
    oi, od, on, _ = ref.search_batch(qs, k, ef, threads=THREADS)
    assert gn.tolist() == on.tolist()
    assert not _unexplained(ref, qs, k, ef, gi, gd, oi, od)
    assert ix.last_batch_stats()["fallbacks"] == 0
    truth, _, _ = O.flat_scan(O.COSINE, O.normalize_rows(base), O.normalize_rows(qs), k, threads=THREADS)
    r_gpu = recall(gi, truth)
    assert abs(r_gpu - recall(oi, truth)) <= 0.005
    assert r_gpu >= 0.9, r_gpu   # (an operating point: i.i.d. Gaussians had none)
    ix.close()


def test_configs4_deep_d96_two_shards_device_merge():
    """configs[4] scaled down: 96-d L2 over two id-range shards, each with its
    own graph (M=64, efC=128) and index (id_base), searched with ef=64 and
    merged on the device == the restatement's per-shard searches merged."""
    import torch
    n, d, nq, k, ef = 16000, 96, 400, 10, 64
    base = O.normalize_rows(counter_gauss(1, 0, n, d))
    qs = O.normalize_rows(counter_gauss(2, 0, nq, d))
    gpu_parts, ref_parts, refs = [], [], []
    for lo, hi in ((0, n // 2), (n // 2, n)):
        ref = O.Index(d, "l2-squared", 64, 128, capacity=hi - lo, seed=3 + lo)
        ref.add_batch(base[lo:hi], threads=THREADS)
        sh = W.GPUVectorIndex(d, "l2-squared", capacity=hi - lo, max_connections=64, id_base=lo)
        sh.upload_vectors(base[lo:hi])
        sh.upload_graph(ref.export_graph())
        gi, gd, gn = sh.search_batch(qs, k, ef=ef, mode="hnsw")
        oi, od, on, _ = ref.search_batch(qs, k, ef, threads=THREADS)
        assert not _unexplained(ref, qs, k, ef, gi - np.uint64(lo), gd, oi, od)
        gpu_parts.append((gi, gd, gn))
        ref_parts.append((oi + np.uint64(lo), od, on))
        sh.close()
    dev = torch.device("cuda:0")
    g_i = torch.from_numpy(np.stack([p[0] for p in gpu_parts]).view(np.int64)).to(dev)
    g_d = torch.from_numpy(np.stack([p[1] for p in gpu_parts])).to(dev)
    g_n = torch.from_numpy(np.stack([p[2] for p in gpu_parts])).to(dev)
    m_d = torch.empty((nq, k), dtype=torch.float32, device=dev)
    m_i = torch.empty((nq, k), dtype=torch.int64, device=dev)
    m_n = torch.empty(nq, dtype=torch.int32, device=dev)
    W.merge_shards_device(g_d.data_ptr(), g_i.data_ptr(), g_n.data_ptr(), 2, nq, k, m_d.data_ptr(), m_i.data_ptr(),
                          m_n.data_ptr())
    torch.cuda.synchronize()
    mi, md, mn = m_i.cpu().numpy().view(np.uint64), m_d.cpu().numpy(), m_n.cpu().numpy()
    wi, wd, wn = merge_lists(gpu_parts, k)
    same(mi, md, wi, wd)                       # the device merge == (dist, id) merge
    ri, rd, rn = merge_lists(ref_parts, k)
    assert mn.tolist() == rn.tolist()
    n_tie = sum(not tie_aware_equal(mi[i], md[i], ri[i], rd[i]) for i in range(nq))
    assert n_tie <= nq // 100, n_tie           # only tie-order decisions (checked per shard above)


def _gloo_rank(rank, world, port, n, d, nq, k, q):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    import torch
    import torch.distributed as dist
    from weaviate_amd.sharded import allgather_topk, merge_topk, shard_bounds
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        base = counter_uniform(1, 0, n, d)
        qs = counter_uniform(2, 0, nq, d)
        lo, hi = shard_bounds(n, rank, world)
        ix = W.GPUVectorIndex(d, "l2-squared", capacity=hi - lo, id_base=lo, device=0)
        ix.upload_vectors(base[lo:hi])
        ids, ds, cnt = ix.search_batch(qs, k, mode="exact")        # HIP key pass + exact re-rank
        g_ids, g_d, g_n = allgather_topk(torch.from_numpy(ids.view(np.int64)), torch.from_numpy(ds),
                                         torch.from_numpy(cnt), world)
        dev = torch.device("cuda", 0)
        m_ids, m_d, m_n = merge_topk(g_ids.to(dev), g_d.to(dev), g_n.to(dev), k)   # device merge kernel
        torch.cuda.synchronize()
        q.put((rank, m_ids.cpu().numpy().view(np.uint64), m_d.cpu().numpy(), m_n.cpu().numpy()))
        ix.close()
    finally:
        dist.destroy_process_group()


def test_two_processes_on_gpu_gloo_shards_equal_single_search():
    """(e): two ranks (one process each, both on this GPU) search their id
    range through libwvgpu.so; the gathered [world, nq, k] lists merged by the
    device kernel equal a single-index search of the whole corpus, bit for bit."""
    import multiprocessing as mp
    n, d, nq, k, world = 40000, 128, 300, 10, 2
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    ps = [ctx.Process(target=_gloo_rank, args=(r, world, port, n, d, nq, k, q)) for r in range(world)]
    for p in ps:
        p.start()
    res = [q.get(timeout=100) for _ in range(world)]
    for p in ps:
        p.join(30)
        assert p.exitcode == 0
    base = counter_uniform(1, 0, n, d)
    qs = counter_uniform(2, 0, nq, d)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n)
    ix.upload_vectors(base)
    si, sd, sn = ix.search_batch(qs, k, mode="exact")
    ix.close()
    oi, od, on = O.flat_scan(O.L2, base, qs, k, threads=THREADS)
    same(si, sd, oi, od)
    for rank, mi, md, mn in res:
        assert mn.tolist() == sn.tolist()
        same(mi, md, si, sd)


def _graph(n, d, metric, M=16, efc=64, seed=11):
    base = counter_uniform(seed, 0, n, d)
    ref = O.Index(d, metric, M, efc, capacity=n, seed=seed)
    ref.add_batch(base, threads=THREADS)
    return base, ref


@pytest.mark.parametrize("forbid_flat", [False, True])
def test_auto_dispatch_flat_cutoff_matches_restatement(forbid_flat):
    """SearchByVector (search.go:64-79): an allow list shorter than
    flatSearchCutoff is answered by flatSearch, otherwise (or with forbidFlat)
    knnSearchByVector with searchTimeEF(k) -- per query, through
    wv_search_by_vector and through one AUTO batch of mixed lists."""
    n, d, k, cut = 6000, 32, 10, 1500
    base, ref = _graph(n, d, "l2-squared")
    ref.set_search_config(flat_search_cutoff=cut, forbid_flat=forbid_flat)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=16, flat_search_cutoff=cut,
                          forbid_flat=forbid_flat)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    rng = np.random.default_rng(5)
    sizes = [200, cut - 1, cut, cut + 1, 3000, 5999]
    qs = counter_uniform(12, 0, 4 * len(sizes), d)
    allows = [W.AllowList.from_ids(rng.choice(n, sizes[i % len(sizes)], replace=False), n) for i in range(len(qs))]
    assert sorted({len(a) for a in allows}) == sorted(sizes)
    want = []
    n_fb = 0
    for q, al in zip(qs, allows):
        gi, gd = ix.search_by_vector(q, k, allow=al)
        if ix.last_batch_stats()["fallbacks"]:
            # a filtered graph search whose side candidates outgrew LDS is
            # answered by flatSearch over the same list (a superset in quality,
            # SURVEY 8b): exact, not the restatement's graph answer
            n_fb += 1
            fi, fd, fn = O.flat_scan(O.L2, base, q[None], k, allow_bits=al.words)
            ri, rd = fi[0, : fn[0]], fd[0, : fn[0]]
        else:
            ri, rd = ref.search_by_vector(q, k, allow=al.words)
        same(gi, gd, ri, rd)
        want.append((ri, rd))
    bi, bd, bn = ix.search_batch(qs, k, allow=allows, mode="auto")
    for i, (ri, rd) in enumerate(want):
        same(bi[i, : bn[i]], bd[i, : bn[i]], ri, rd)
    # unfiltered: always the graph (search.go:74-78)
    ui, ud = ix.search_by_vector(qs[0], k)
    ri, rd = ref.search_by_vector(qs[0], k)
    same(ui, ud, ri, rd)
    ix.close()


def test_default_ef_through_the_abi_matches_restatement():
    """ef = -1 (the default): the search runs with searchTimeEF(k) =
    clamp(k * 8, 100, 500) (search.go:30-62) -- checked on the index's own
    entry point and on the results of an ef=0 batch."""
    n, d = 5000, 24
    base, ref = _graph(n, d, "l2-squared", seed=13)
    ix = W.GPUVectorIndex(d, "l2-squared", capacity=n, max_connections=16)
    ix.upload_vectors(base)
    ix.upload_graph(ref.export_graph())
    assert [ix.search_time_ef(k) for k in (10, 23, 100)] == [100, 184, 500]
    qs = counter_uniform(14, 0, 100, d)
    for k in (10, 23):
        gi, gd, gn = ix.search_batch(qs, k, ef=0, mode="hnsw")
        oi, od, on, _ = ref.search_batch(qs, k, O.search_time_ef(-1, 100, 500, 8, k), threads=THREADS)
        same(gi, gd, oi, od)
        for i in range(0, len(qs), 10):
            ri, rd = ref.search_by_vector(qs[i], k)
            same(gi[i], gd[i], ri, rd)
    ix.update_user_config(ef=78)
    assert ix.search_time_ef(5) == 78
    ix.close()
