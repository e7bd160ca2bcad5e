#!/usr/bin/env python3
"""Per-query id lists on a manhattan or hamming index: ms per batch.

Times the wall time around the C call, host in to host out, of one batch of
nq queries with distinct ascending lists of L ids each over an n x dim index
(uniform [-1, 1) rows for manhattan, {0, 1, 2} for hamming):

    knn     wv_search_batch_ids, k = --k; the list kernel's device time
            (wv_last_sparse_time: HIP events, chunk merge included) comes from
            a pass of its own with timing on
    thresh  wv_search_by_vector_distance_batch_ids, max_limit -1, the target of
            a query the --within-th smallest distance of its list

One JSON line per (metric, mode, nq, L): median, minimum, maximum and
inter-quartile range of --steps timed calls after --warmup, the route counts
and the answers' SHA-256, to compare processes.  WV_LIBPATH names another
build of the library (the parent commit's, or an A/B build of tools/ab_build.sh
with -DWV_L1_IDS_R=1|2|4).

    python tools/bench_l1_ids.py --points 1024x1000 1x1000 --out profiles/l1_ids/new.jsonl
"""
import argparse
import ctypes as C
import hashlib
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


def make_lists(rng, n, nq, L):
    """nq distinct ascending lists of L ids: windows of one permutation."""
    perm = rng.permutation(n).astype(np.uint64)
    step = max(1, (n - L) // max(nq, 1))
    return [np.sort(perm[(q * step + np.arange(L)) % n]) for q in range(nq)]


def summary(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "ms_iqr": float(q3 - q1)}


def chain(metric, q, rows):
    """the float32 chains of one query against rows, dimension by dimension"""
    s = np.zeros(rows.shape[0], np.float32)
    for i in range(rows.shape[1]):
        s += np.abs(q[i] - rows[:, i]) if metric == "manhattan" else (q[i] != rows[:, i]).astype(np.float32)
    return s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--metrics", nargs="+", default=["manhattan", "hamming"])
    ap.add_argument("--modes", nargs="+", default=["knn", "thresh"])
    ap.add_argument("--points", nargs="+", default=["1024x100", "1024x1000", "1024x10000", "1024x100000", "1x1000",
                                                    "64x1000"], help="NQxL")
    ap.add_argument("--within", type=int, default=100)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    points = [tuple(int(x) for x in p.split("x")) for p in a.points]
    nq_max = max(p[0] for p in points)
    for metric in a.metrics:
        rng = np.random.default_rng(5)
        if metric == "hamming":
            draw = lambda m: rng.integers(0, 3, (m, a.dim)).astype(np.float32)
        else:
            draw = lambda m: rng.random((m, a.dim), dtype=np.float32) * 2 - 1
        base, qs_all = draw(a.n), np.ascontiguousarray(draw(nq_max))
        ix = W.GPUVectorIndex(a.dim, metric, capacity=a.n)
        ix.upload_vectors(base)
        cache = {}
        for nq, L in points:
            if L not in cache:
                cache.clear()
                cache[L] = make_lists(np.random.default_rng(1000 + L), a.n, nq_max, L)
            lists = cache[L][:nq]
            qs = np.ascontiguousarray(qs_all[:nq])
            flat = np.ascontiguousarray(np.concatenate(lists))
            off = np.zeros(nq + 1, np.uint64)
            off[1:] = np.cumsum([x.size for x in lists])
            lib, cap = W.lib(), 4096

            def checked(rc):
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            for mode in a.modes:
                if mode == "knn":
                    res = (np.zeros((nq, a.k), np.uint64), np.zeros((nq, a.k), np.float32), np.zeros(nq, np.int32))
                    call = lambda: checked(lib.wv_search_batch_ids(ix._h, vp(qs), nq, a.k, 0, vp(flat), vp(off),
                                                                   W.MODE_AUTO, vp(res[0]), vp(res[1]), vp(res[2])))
                else:
                    # the target from a sample of at most ~4096 of the list's rows, at the rank
                    # that leaves about --within rows of the whole list under it
                    targets = np.zeros(nq, np.float32)
                    for q in range(nq):
                        smp = chain(metric, qs[q], base[lists[q][:: max(1, L // 2048)].astype(np.int64)])
                        r = min(len(smp) - 1, max(0, a.within * len(smp) // L - 1))
                        targets[q] = np.partition(smp, r)[r]
                    res = (np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32), np.zeros(nq, np.int64))
                    call = lambda: checked(lib.wv_search_by_vector_distance_batch_ids(
                        ix._h, vp(qs), nq, vp(targets), -1, vp(flat), vp(off), vp(res[0]), vp(res[1]), cap, vp(res[2])))
                t = []
                for step in range(a.warmup + a.steps):
                    t0 = time.perf_counter()
                    call()
                    if step >= a.warmup:
                        t.append((time.perf_counter() - t0) * 1e3)
                rec = {"label": a.label, "metric": metric, "mode": mode, "n": a.n, "dim": a.dim, "nq": nq,
                       "list_len": L, "steps": a.steps, "warmup": a.warmup,
                       "WV_LIBPATH": os.path.basename(os.path.dirname(os.environ["WV_LIBPATH"]))
                       if os.environ.get("WV_LIBPATH") else None, **summary(t)}
                # (the rows up to each query's count: the slots past it are the caller's)
                width = res[0].shape[1]
                rec["answers_sha256"] = hashlib.sha256(b"".join(
                    res[0][q, :min(int(res[2][q]), width)].tobytes() + res[1][q, :min(int(res[2][q]), width)].tobytes()
                    for q in range(nq)) + res[2].tobytes()).hexdigest()
                if mode == "knn":
                    rec["k"] = a.k
                    rec["stats"] = ix.last_sparse_stats()
                    if rec["stats"]["sparse_queries"]:
                        ix.set_timing(True)
                        kt = []
                        for _ in range(max(3, a.steps)):
                            call()
                            kt.append(ix.last_sparse_time())
                        ix.set_timing(False)
                        rec["list_kernel_ms_median"] = float(np.median(kt))
                        rec["list_kernel_ms_min"] = float(np.min(kt))
                else:
                    rec["stats"] = ix.last_sbd_ids_stats()
                    rec["within_mean"] = float(np.mean(res[2]))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
        ix.close()
        del base


if __name__ == "__main__":
    main()
