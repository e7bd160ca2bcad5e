#!/usr/bin/env python3
"""SearchByVectorDistance on a PQ-compressed index: ms per batch of the batch entry points.

Builds a compressed flat-plus-graph index (wv_index_build_graph; a KMeans
table drawn from data rows, one row's segment per centroid; codes encoded on
the device) and times, per leg, the wall time around the C call, host in to
host out:

  ids_1pct, ids_10pct  64 queries with per-query id lists of 1 % / 10 % of the
                       rows (wv_search_by_vector_distance_batch_ids)
  unfiltered           64 queries, no filter: HNSW round 1
                       (wv_search_by_vector_distance_batch)
  single               one query per call, no filter

A query's target is its 150th-nearest PQ distance over the rows it may return
(from the exact search), so every query deepens to the second round.

The library reads its switches per call, so one process times several
variants of a leg alternately, step by step (--variants): "default", "pq0"
(WV_SBD_PQ=0: the per-query rounds, the route of before), "lut0" and "lut1"
(WV_SBD_PQ_LUT: direct evaluation / the lookup table everywhere).  One JSON
line per leg and variant: the median, minimum and maximum of --steps timed
calls after --warmup, the inter-quartile range as the run-to-run spread, and
whether the variant's answers (ids, distance bits, counts) equal the first
variant's.  WV_LIBPATH names another build of the library (an older one is
bound as far as its symbols go; it ignores switches it does not know).
--leg runs single legs, so a driver can give every leg its own time limit.

    python tools/sbd_pq_bench.py --n 1000000 --variants default pq0 lut0 lut1 --out profiles/sbd_pq/new_1m.jsonl
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
from weaviate_amd import _lib  # noqa: E402

if os.environ.get("WV_LIBPATH"):
    _probe = C.CDLL(_lib.LIBPATH)
    for _name in [s for s in _lib.SIGNATURES if not hasattr(_probe, s)]:
        del _lib.SIGNATURES[_name]
import weaviate_amd as W  # noqa: E402

LEGS = ("ids_1pct", "ids_10pct", "unfiltered", "single")


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def centroids(base, m, ks, seed):
    rng = np.random.default_rng(seed)
    ds = base.shape[1] // m
    rows = rng.choice(base.shape[0], ks, replace=False)
    return np.stack([base[rows, i * ds:(i + 1) * ds] for i in range(m)]).astype(np.float32)


VARIANTS = {"default": {}, "pq0": {"WV_SBD_PQ": "0"}, "lut0": {"WV_SBD_PQ_LUT": "0"}, "lut1": {"WV_SBD_PQ_LUT": "1"}}


def set_variant(v):
    for k in ("WV_SBD_PQ", "WV_SBD_PQ_LUT"):
        os.environ.pop(k, None)
    os.environ.update(VARIANTS[v])


def timed(call, variants, steps, warmup):
    """ms of every step of every variant, the variants alternating (the call blocks until the answer is on the host)."""
    t = {v: [] for v in variants}
    for step in range(warmup + steps):
        for v in variants:
            set_variant(v)
            t0 = time.perf_counter()
            call()
            if step >= warmup:
                t[v].append((time.perf_counter() - t0) * 1e3)
    return t


def summary(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "ms_iqr": float(q3 - q1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--nq", type=int, default=64)
    ap.add_argument("--rank", type=int, default=150)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=256, help="results written per query")
    ap.add_argument("--leg", choices=LEGS, action="append", help="legs to run (default: all)")
    ap.add_argument("--variants", choices=list(VARIANTS), nargs="+", default=["default"])
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    legs = a.leg or list(LEGS)
    lib = W.lib()
    rng = np.random.default_rng(5)
    base = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    qs = np.ascontiguousarray(rng.standard_normal((a.nq, a.dim)).astype(np.float32))
    ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n, max_connections=32)
    ix.upload_vectors(base)
    t0 = time.perf_counter()
    if any(leg in ("unfiltered", "single") for leg in legs):
        ix.build_graph(ef_construction=64)
    build_s = time.perf_counter() - t0
    ix.set_pq(centroids(base, a.segments, a.centroids, 5))
    ix.pq_encode()
    ix.set_compressed(True)
    del base
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    nq, cap = a.nq, a.cap
    oi, od, on = np.zeros((nq, cap), np.uint64), np.zeros((nq, cap), np.float32), np.zeros(nq, np.int64)
    for leg in legs:
        rec = {"leg": leg, "label": a.label, "n": a.n, "dim": a.dim, "segments": a.segments, "centroids": a.centroids,
               "steps": a.steps, "warmup": a.warmup, "target_rank": a.rank, "graph_build_s": build_s,
               "WV_LIBPATH": os.path.basename(os.path.dirname(os.environ["WV_LIBPATH"])) if os.environ.get("WV_LIBPATH")
               else None}
        if leg.startswith("ids"):
            share = 0.01 if leg == "ids_1pct" else 0.1
            lists = [np.sort(rng.choice(a.n, int(a.n * share), replace=False)).astype(np.uint64) for _ in range(nq)]
            allow = [W.AllowList.from_ids(x, a.n) for x in lists]
            _, kd, kn = ix.search_batch(qs, a.rank, allow=allow, mode="exact")
            targets = np.ascontiguousarray(np.array([kd[i, kn[i] - 1] for i in range(nq)], np.float32))
            del allow
            flat = np.ascontiguousarray(np.concatenate(lists))
            off = np.zeros(nq + 1, np.uint64)
            off[1:] = np.cumsum([x.size for x in lists])

            def call():
                rc = lib.wv_search_by_vector_distance_batch_ids(ix._h, vp(qs), nq, vp(targets), -1, vp(flat), vp(off),
                                                                vp(oi), vp(od), cap, vp(on))
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            rec["nq"] = nq
            rec["list_len"] = int(a.n * share)
        else:
            n1 = nq if leg == "unfiltered" else 1
            _, kd, kn = ix.search_batch(qs[:n1], a.rank, mode="exact")
            targets = np.ascontiguousarray(np.array([kd[i, kn[i] - 1] for i in range(n1)], np.float32))

            def call():
                rc = lib.wv_search_by_vector_distance_batch(ix._h, vp(qs), n1, vp(targets), -1, None, 0, 0, vp(oi),
                                                            vp(od), cap, vp(on))
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            rec["nq"] = n1
        times = timed(call, a.variants, a.steps, a.warmup)
        first = None
        for v in a.variants:
            set_variant(v)
            call()
            k = rec["nq"]
            m = np.minimum(on[:k], cap)
            ans = (on[:k].tolist(), [oi[i, : m[i]].tolist() for i in range(k)],
                   [od[i, : m[i]].view(np.uint32).tolist() for i in range(k)])
            first = first or ans
            r = dict(rec, variant=v, **summary(times[v]))
            r["results_per_query_mean"] = float(on[:k].mean())
            r["answers_equal_first_variant"] = ans == first
            # (a fingerprint of the answers, to compare processes)
            r["answer_sum"] = int(sum(sum(x) for x in ans[1]))
            if leg.startswith("ids"):
                r["stats"] = ix.last_sbd_ids_stats()
            elif "wv_last_sbd_stats" in _lib.SIGNATURES:
                r["stats"] = ix.last_sbd_stats()
            line = json.dumps(r)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
        set_variant("default")
    ix.close()


if __name__ == "__main__":
    main()
