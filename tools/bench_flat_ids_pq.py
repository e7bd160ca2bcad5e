#!/usr/bin/env python3
"""Per-query id lists on a PQ-compressed index: ms per batch of wv_search_batch_ids.

Builds a compressed flat index (a KMeans table drawn from data rows, one row's
segment per centroid; codes encoded on the device) and times the wall time
around the C call, host in to host out, of one batch of --nq queries with
distinct lists of --lens ids each.

The variants of a batch are timed alternately, step by step, in one process.
A variant is "off" (the bitmap route: the library's default) or "on"
(wv_index_set_pq_list_search: the list kernel over the codes), optionally
followed by switches the library reads per call:

    on,WV_FLAT_IDS_PQ_LUT=0      every workgroup evaluates rows directly
    on,WV_FLAT_IDS_PQ_LUT=1      the lookup table wherever it fits
    on,WV_FLAT_IDS_PQ_CHUNK=0    no floor under a workgroup's chunk of a list

One JSON line per (nq, list length, variant): median, minimum, maximum and
inter-quartile range of --steps timed calls after --warmup, the list kernel's
device time (HIP events, in a pass of its own), the route counts, whether the
answers (ids, distance bits, counts) equal the first variant's, and their
SHA-256, to compare processes.  WV_LIBPATH names another build of the library
(an older one is bound as far as its symbols go: only "off" runs there).

    python tools/bench_flat_ids_pq.py --variants off on --out profiles/flat_ids_pq/new.jsonl
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

SWITCHES = ("WV_FLAT_IDS_PQ_LUT", "WV_FLAT_IDS_PQ_CHUNK")
HAS_SETTER = "wv_index_set_pq_list_search" in _lib.SIGNATURES


def vp(a):
    return C.c_void_p(a.ctypes.data)


def centroids(base, m, ks, seed):
    rng = np.random.default_rng(seed)
    ds = base.shape[1] // m
    rows = rng.choice(base.shape[0], ks, replace=False)
    return np.stack([base[rows, i * ds:(i + 1) * ds] for i in range(m)]).astype(np.float32)


def set_variant(ix, v):
    parts = v.split(",")
    if parts[0] not in ("on", "off"):
        raise SystemExit(f"variant {v!r}: starts with on or off")
    for k in SWITCHES:
        os.environ.pop(k, None)
    for kv in parts[1:]:
        k, val = kv.split("=", 1)
        os.environ[k] = val
    if HAS_SETTER:
        ix.set_pq_list_search(parts[0] == "on")
    elif parts[0] == "on":
        raise SystemExit("this build has no wv_index_set_pq_list_search: only 'off' runs")


def make_lists(rng, n, nq, L):
    """nq distinct ascending lists of L ids: windows of one permutation."""
    perm = rng.permutation(n).astype(np.uint64)
    step = max(1, (n - L) // max(nq, 1))
    return [np.sort(perm[(q * step + np.arange(L)) % n]) for q in range(nq)]


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
    ap.add_argument("--nq", type=int, nargs="+", default=[1024])
    ap.add_argument("--lens", type=int, nargs="+", default=[100, 1000, 10000, 100000])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--variants", nargs="+", default=["off", "on"])
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
    del base
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    k = a.k
    for L in a.lens:
        lists = make_lists(rng, a.n, nq_max, L)
        for nq in a.nq:
            qs = np.ascontiguousarray(qs_all[:nq])
            flat = np.ascontiguousarray(np.concatenate(lists[:nq]))
            off = np.zeros(nq + 1, np.uint64)
            off[1:] = np.cumsum([x.size for x in lists[:nq]])
            oi, od, on = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)

            def call():
                rc = lib.wv_search_batch_ids(ix._h, vp(qs), nq, k, 0, vp(flat), vp(off), W.MODE_AUTO, vp(oi), vp(od),
                                             vp(on))
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            t = {v: [] for v in a.variants}
            for step in range(a.warmup + a.steps):
                for v in a.variants:
                    set_variant(ix, v)
                    t0 = time.perf_counter()
                    call()
                    if step >= a.warmup:
                        t[v].append((time.perf_counter() - t0) * 1e3)
            first = None
            for v in a.variants:
                set_variant(ix, v)
                call()
                ans = oi.tobytes() + od.tobytes() + on.tobytes()
                first = first if first is not None else ans
                rec = {"label": a.label, "variant": v, "n": a.n, "dim": a.dim, "segments": a.segments,
                       "centroids": a.centroids, "k": k, "nq": nq, "list_len": L, "steps": a.steps, "warmup": a.warmup,
                       "WV_LIBPATH": os.path.basename(os.path.dirname(os.environ["WV_LIBPATH"]))
                       if os.environ.get("WV_LIBPATH") else None, **summary(t[v])}
                rec["stats"] = ix.last_sparse_stats()
                rec["answers_equal_first_variant"] = ans == first
                rec["answers_sha256"] = hashlib.sha256(ans).hexdigest()
                rec["results_per_query_mean"] = float(on.mean())
                if v.startswith("on"):
                    ix.set_timing(True)
                    kt = []
                    for _ in range(max(3, a.steps)):
                        call()
                        kt.append(ix.last_sparse_time())
                    ix.set_timing(False)
                    rec["list_kernel_ms_median"] = float(np.median(kt))
                    rec["list_kernel_ms_min"] = float(np.min(kt))
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    ix.close()


if __name__ == "__main__":
    main()
