#!/usr/bin/env python3
"""Flat k-NN on a PQ-compressed index: ms per batch of wv_search_batch, mode exact.

Builds a compressed flat index (a KMeans table drawn from data rows, one row's
segment per centroid; codes encoded on the device) and times the wall time
around the C call, host in to host out, of one batch of --nq queries under a
filter: none, one shared bitmap, or a bitmap per query (--frac of the rows).

The variants of a batch are timed alternately, step by step, in one process.
A variant is "off" (the scan-and-sort route: the library's default), "on"
(wv_index_set_pq_scan: the fused scan) or "list" (wv_index_set_pq_list_search
and wv_search_batch_ids with every query handed every id: the list kernel as
a dense scan; --list-max-nq bounds it), optionally followed by switches the
library reads per call:

    on,WV_PQ_SCAN_GROUP=1       one query per workgroup (2, 4 likewise)
    on,WV_PQ_SCAN_ROWS=65536    rows per workgroup

One JSON line per (nq, filter, variant): median, minimum, maximum and
inter-quartile range of --steps timed calls after --warmup, the route counts,
whether the answers (ids, distance bits, counts) equal the first variant's,
and their SHA-256, to compare processes.  WV_LIBPATH names another build of
the library (an older one is bound as far as its symbols go: only "off" runs
there).

    python tools/bench_pq_scan.py --variants off on --out profiles/pq_scan/new.jsonl
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
from weaviate_amd import _lib  # noqa: E402

if os.environ.get("WV_LIBPATH"):
    _probe = C.CDLL(_lib.LIBPATH)
    for _name in [s for s in _lib.SIGNATURES if not hasattr(_probe, s)]:
        del _lib.SIGNATURES[_name]
import weaviate_amd as W  # noqa: E402

SWITCHES = ("WV_PQ_SCAN_GROUP", "WV_PQ_SCAN_ROWS")
HAS_SETTER = "wv_index_set_pq_scan" in _lib.SIGNATURES


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def centroids(base, m, ks, seed):
    rng = np.random.default_rng(seed)
    ds = base.shape[1] // m
    rows = rng.choice(base.shape[0], ks, replace=False)
    return np.stack([base[rows, i * ds:(i + 1) * ds] for i in range(m)]).astype(np.float32)


def set_variant(ix, v):
    parts = v.split(",")
    if parts[0] not in ("on", "off", "list"):
        raise SystemExit(f"variant {v!r}: starts with on, off or list")
    for k in SWITCHES:
        os.environ.pop(k, None)
    for kv in parts[1:]:
        k, val = kv.split("=", 1)
        os.environ[k] = val
    if HAS_SETTER:
        ix.set_pq_scan(parts[0] == "on")
    elif parts[0] == "on":
        raise SystemExit("this build has no wv_index_set_pq_scan: only 'off' runs")
    return parts[0]


def summary(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "ms_iqr": float(q3 - q1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 8, 64, 1024])
    ap.add_argument("--filters", nargs="+", default=["none", "shared", "each"])
    ap.add_argument("--frac", type=float, default=0.1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", nargs="+", default=["off", "on"])
    ap.add_argument("--list-max-nq", type=int, default=64)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lib = W.lib()
    rng = np.random.default_rng(5)
    base = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    nq_max = max(a.nq)
    qs_all = np.ascontiguousarray(rng.standard_normal((nq_max, a.dim)).astype(np.float32))
    ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n)
    ix.upload_vectors(base)
    ix.set_pq(centroids(base, a.segments, a.centroids, 5))
    ix.pq_encode()
    ix.set_compressed(True)
    ix.update_user_config(flat_search_cutoff=1 << 40)   # "list": every list is searched flat
    ix.set_pq_list_search(True)
    del base
    words = (a.n + 63) // 64
    # bitmaps of --frac of the rows: bit r of word r / 64, rows past n clear
    # (row 0: the shared one; rows 1..: one per query)
    maps = np.zeros(((nq_max if "each" in a.filters else 0) + 1, words), np.uint64)
    for r in range(maps.shape[0]):
        bits = rng.random(words * 64) < a.frac
        bits[a.n:] = False
        maps[r] = np.packbits(bits, bitorder="little").view(np.uint64)
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    k = a.k
    all_ids = np.arange(a.n, dtype=np.uint64)
    for nq in a.nq:
        qs = np.ascontiguousarray(qs_all[:nq])
        oi, od, on = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)
        for flt in a.filters:
            allow = {"none": None, "shared": maps[:1], "each": maps[1:nq + 1]}[flt]
            stride = words if flt == "each" else 0
            variants = [v for v in a.variants if not v.startswith("list") or (flt == "none" and nq <= a.list_max_nq)]
            flat = np.ascontiguousarray(np.tile(all_ids, nq)) if any(v.startswith("list") for v in variants) else None
            off = np.arange(nq + 1, dtype=np.uint64) * np.uint64(a.n)

            def call(kind):
                if kind == "list":
                    rc = lib.wv_search_batch_ids(ix._h, vp(qs), nq, k, 0, vp(flat), vp(off), W.MODE_AUTO, vp(oi),
                                                 vp(od), vp(on))
                else:
                    rc = lib.wv_search_batch(ix._h, vp(qs), nq, k, 0, vp(allow), a.n if allow is not None else 0,
                                             stride, W.MODE_EXACT, vp(oi), vp(od), vp(on))
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            t = {v: [] for v in variants}
            for step in range(a.warmup + a.steps):
                for v in variants:
                    kind = set_variant(ix, v)
                    t0 = time.perf_counter()
                    call(kind)
                    if step >= a.warmup:
                        t[v].append((time.perf_counter() - t0) * 1e3)
            first = None
            for v in variants:
                call(set_variant(ix, v))
                ans = oi.tobytes() + od.tobytes() + on.tobytes()
                first = first if first is not None else ans
                rec = {"label": a.label, "variant": v, "n": a.n, "dim": a.dim, "segments": a.segments,
                       "centroids": a.centroids, "k": k, "nq": nq, "filter": flt, "frac": a.frac, "steps": a.steps,
                       "warmup": a.warmup,
                       "WV_LIBPATH": os.path.basename(os.path.dirname(os.environ["WV_LIBPATH"]))
                       if os.environ.get("WV_LIBPATH") else None, **summary(t[v])}
                if HAS_SETTER:
                    rec["stats"] = ix.last_pq_scan_stats()
                rec["answers_equal_first_variant"] = ans == first
                rec["answers_sha256"] = hashlib.sha256(ans).hexdigest()
                rec["results_per_query_mean"] = float(on.mean())
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    ix.close()


if __name__ == "__main__":
    main()
