#!/usr/bin/env python3
"""Large-k exact search on manhattan, hamming and PQ-compressed indexes: ms per
wv_search_batch call, the large-k route on against off in one process.

Per --kind an index of --n x --dim rows (manhattan: uniform in [-1, 1);
hamming: integers 0..7; pq: standard normal rows, --segments x --centroids
codes encoded on the device, the fused scan on as a deployment would have it).
Per (k, nq) the two variants are timed alternately, call by call: wall time
around the C call, host in to host out, which ends in the batch's device
synchronise.  One JSON line per (kind, variant, k, nq): median, minimum and
maximum of --steps calls after --warmup, the route's counts, the device time
of one further call by stage (timing events: bound pass, threshold pass, sort +
emit) and the SHA-256 of the answers, equal between the variants.

    python tools/bench_large_k_kinds.py --out profiles/large_k_kinds/ab.jsonl
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


def build(W, kind, a, rng):
    if kind == "pq":
        base = rng.standard_normal((a.n, a.dim)).astype(np.float32)
        ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n)
        ix.upload_vectors(base)
        ds = a.dim // a.segments
        rows = rng.choice(a.n, a.centroids, replace=False)
        ix.set_pq(np.stack([base[rows, i * ds:(i + 1) * ds] for i in range(a.segments)]).astype(np.float32))
        ix.pq_encode()
        ix.set_compressed(True)
        ix.set_pq_scan(True)
        return ix, np.ascontiguousarray(rng.standard_normal((max(a.nq), a.dim)).astype(np.float32))
    if kind == "hamming":
        draw = lambda m: rng.integers(0, 8, (m, a.dim)).astype(np.float32)   # noqa: E731
    else:
        draw = lambda m: rng.random((m, a.dim), dtype=np.float32) * 2 - 1    # noqa: E731
    ix = W.GPUVectorIndex(a.dim, kind, capacity=a.n)
    ix.upload_vectors(draw(a.n))
    return ix, np.ascontiguousarray(draw(max(a.nq)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kind", nargs="+", default=["manhattan", "hamming", "pq"])
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--k", type=int, nargs="+", default=[1000])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 3, 1024])
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import weaviate_amd as W
    lib = W.lib()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    vp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    for kind in a.kind:
        ix, qs_all = build(W, kind, a, np.random.default_rng(5))
        for k in a.k:
            for nq in a.nq:
                qs = np.ascontiguousarray(qs_all[:nq])
                oi, od, on = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)

                def call(variant):
                    ix.set_large_k(variant == "on")
                    t0 = time.perf_counter()
                    if lib.wv_search_batch(ix._h, vp(qs), nq, k, 0, None, 0, 0, W.MODE_EXACT, vp(oi), vp(od), vp(on)):
                        raise RuntimeError(lib.wv_last_error().decode())
                    return (time.perf_counter() - t0) * 1e3

                t = {"off": [], "on": []}
                for step in range(a.warmup + a.steps):
                    for v in t:
                        ms = call(v)
                        if step >= a.warmup:
                            t[v].append(ms)
                for v in t:
                    ix.set_timing(True)
                    call(v)
                    kt = ix.last_kernel_times()
                    ix.set_timing(False)
                    batched, legacy = ix.last_large_k_stats()
                    rec = {"kind": kind, "variant": v, "n": a.n, "dim": a.dim, "k": k, "nq": nq, "steps": a.steps,
                           "warmup": a.warmup, "ms_median": float(np.median(t[v])), "ms_min": float(np.min(t[v])),
                           "ms_max": float(np.max(t[v])), "batched_queries": batched, "legacy_queries": legacy,
                           "bound_ms": kt["seed_ms"], "threshold_ms": kt["bf_mfma_ms"],
                           "sort_emit_ms": kt["bf_finalize_ms"],
                           "answers_sha256": hashlib.sha256(oi.tobytes() + od.tobytes() + on.tobytes()).hexdigest()}
                    if kind == "pq":
                        rec.update(segments=a.segments, centroids=a.centroids)
                    line = json.dumps(rec)
                    print(line, flush=True)
                    if out:
                        out.write(line + "\n")
                        out.flush()
        ix.close()


if __name__ == "__main__":
    main()
