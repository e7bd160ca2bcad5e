#!/usr/bin/env python3
"""SearchByVectorDistance over per-query allow lists: ids against bitmaps, same build.

Times one batch two ways, interleaved: wv_search_by_vector_distance_batch_ids
(the threshold pass walks the lists) and wv_search_by_vector_distance_batch
with one bitmap row per query (the route such a batch took before; unchanged
code).  Wall time around the C call, host in to host out, so the host work of
either route is inside: the popcount of every bitmap row and the upload of the
rows on one side, the ascending check and the narrowing of the ids on the
other.  The inputs of both calls (the bitmap matrix, the concatenated ids) are
prepared beforehand; filling bitmap rows from ids, which the micro-batcher
does for the bitmap route, is timed apart (numpy, "fill_rows_ms").

Lists are Bernoulli samples of the ids, one per query; a query's target is the
distance of its 150th-nearest listed row.  The two routes' answers are
compared on every shape.  One JSON line per shape (stdout, and --out).

    python tools/sbd_ids_ab.py --out profiles/sbd_ids/ab.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import weaviate_amd as W  # noqa: E402


def vp(a):
    return C.c_void_p(a.ctypes.data)


def bernoulli_lists(rng, n, nq, share):
    """nq ascending samples of [0, n), each id kept with probability `share`."""
    lens = rng.binomial(n, share, nq)
    return [np.sort(rng.choice(n, int(L), replace=False)).astype(np.uint64) for L in lens]


def bench(ix, n, qs, lists, rank, reps, warmup, cap, out):
    nq = len(lists)
    q = np.ascontiguousarray(qs[:nq])
    # targets: the rank-th nearest listed row, from the exact id-list search
    _, kd, kn = ix.search_batch_ids(q, rank, lists, mode="exact")
    targets = np.ascontiguousarray(np.array([kd[i, kn[i] - 1] if kn[i] else 0.0 for i in range(nq)], np.float32))
    flat = np.ascontiguousarray(np.concatenate(lists))
    off = np.zeros(nq + 1, np.uint64)
    off[1:] = np.cumsum([a.size for a in lists])
    words = (n + 63) // 64
    t0 = time.perf_counter()
    bits = np.zeros((nq, words), np.uint64)
    for i, a in enumerate(lists):
        np.bitwise_or.at(bits[i], (a >> np.uint64(6)).astype(np.int64), np.uint64(1) << (a & np.uint64(63)))
    fill_ms = (time.perf_counter() - t0) * 1e3
    res = {r: (np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32), np.zeros(nq, np.int64))
           for r in ("ids", "bitmap")}
    lib = W.lib()

    def run(route):
        oi, od, on = res[route]
        t0 = time.perf_counter()
        if route == "ids":
            rc = lib.wv_search_by_vector_distance_batch_ids(ix._h, vp(q), nq, vp(targets), -1, vp(flat), vp(off), vp(oi),
                                                            vp(od), cap, vp(on))
        else:
            rc = lib.wv_search_by_vector_distance_batch(ix._h, vp(q), nq, vp(targets), -1, vp(bits), n, words, vp(oi),
                                                        vp(od), cap, vp(on))
        dt = time.perf_counter() - t0
        if rc:
            raise RuntimeError(lib.wv_last_error().decode())
        return dt * 1e3

    for _ in range(warmup):
        run("ids")
        run("bitmap")
    t = {"ids": [], "bitmap": []}
    same = True
    for _ in range(reps):
        for r in ("ids", "bitmap"):
            t[r].append(run(r))
        a, b = res["ids"], res["bitmap"]
        same = same and a[2].tolist() == b[2].tolist() and all(
            a[0][i, :m].tolist() == b[0][i, :m].tolist()
            and np.array_equal(a[1][i, :m].view(np.uint32), b[1][i, :m].view(np.uint32))
            for i, m in enumerate(np.minimum(a[2], cap)))
    rec = {"n": n, "dim": int(qs.shape[1]), "nq": nq, "list_share": float(np.mean([a.size for a in lists]) / n),
           "list_len_mean": float(np.mean([a.size for a in lists])), "target_rank": rank, "reps": reps,
           "warmup": warmup, "results_per_query_mean": float(res["ids"][2].mean()),
           "fill_rows_ms": fill_ms, "answers_identical": bool(same), "stats": ix.last_sbd_ids_stats()}
    for r in ("ids", "bitmap"):
        rec[r + "_ms_median"] = float(np.median(t[r]))
        rec[r + "_ms_min"] = float(np.min(t[r]))
        rec[r + "_ms_max"] = float(np.max(t[r]))
    rec["speedup_median"] = rec["bitmap_ms_median"] / rec["ids_ms_median"]
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 1024])
    ap.add_argument("--shares", type=float, nargs="+", default=[0.0003, 0.01, 0.1])
    ap.add_argument("--rank", type=int, default=150)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--cap", type=int, default=256, help="results written per query")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "w")
    rng = np.random.default_rng(5)
    base = rng.random((a.n, a.dim), dtype=np.float32)
    qs = rng.random((max(a.batches), a.dim), dtype=np.float32)
    ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n)
    ix.upload_vectors(base)
    del base
    for share in a.shares:
        lists = bernoulli_lists(rng, a.n, max(a.batches), share)
        for nq in a.batches:
            bench(ix, a.n, qs, lists[:nq], a.rank, a.reps, a.warmup, a.cap, out)
    ix.close()


if __name__ == "__main__":
    main()
