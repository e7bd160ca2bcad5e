#!/usr/bin/env python3
"""Fitting the KMeans product quantizer on the device: seconds per wv_index_fit_pq.

Uploads --n standard-normal rows of --dim floats and times the wall time around
the C call (host in to host out: the fit blocks, the fitted table is copied
back) of --steps fits after --warmup, centres drawn from --seed.  One JSON line:
median, minimum, maximum of the fits, the assignment passes run per segment
and the empty clusters re-seeded.

Beside it, the CPU restatement's time (tests/pq_fit_restatement.py: numpy plus
the oracle's C encoder on one thread -- NOT the reference's Go code) on the
first --cpu-n rows, a size it finishes, with the device's fit of the same rows
and whether the two tables have the same bits.  --cpu-n 0 skips it.

    python tools/bench_pq_fit.py --out profiles/pq_fit/fit.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import weaviate_amd as W  # noqa: E402


def timed_fits(ix, a, steps, warmup):
    t, last = [], None
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        last = ix.fit_pq(a.segments, a.centroids, seed=a.seed)
        if step >= warmup:
            t.append(time.perf_counter() - t0)
    return t, last


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--segments", type=int, default=32)
    ap.add_argument("--centroids", type=int, default=256)
    ap.add_argument("--seed", type=int, default=5)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--cpu-n", type=int, default=20_000)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + "\n")
            out.flush()

    rng = np.random.default_rng(5)
    base = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    shape = {"label": a.label, "dim": a.dim, "segments": a.segments, "centroids": a.centroids, "seed": a.seed}
    ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n)
    ix.upload_vectors(base)
    t, (table, iters, reseeded) = timed_fits(ix, a, a.steps, a.warmup)
    t0 = time.perf_counter()
    ix.pq_encode()
    ix.set_compressed(True)
    t_rest = time.perf_counter() - t0
    ix.close()
    emit({"what": "device fit (wv_index_fit_pq), wall time around the call", "n": a.n, **shape, "steps": a.steps,
          "warmup": a.warmup, "s_median": float(np.median(t)), "s_min": float(np.min(t)), "s_max": float(np.max(t)),
          "passes_per_segment": iters.tolist(), "reseeded": int(reseeded),
          "encode_and_switch_s": t_rest, "table_finite": bool(np.isfinite(table).all())})

    if a.cpu_n > 0:
        import pq_fit_restatement as R
        small = np.ascontiguousarray(base[: a.cpu_n])
        t0 = time.perf_counter()
        want = R.Fit(small, a.segments, a.centroids, seed=a.seed)
        t_cpu = time.perf_counter() - t0
        ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.cpu_n)
        ix.upload_vectors(small)
        t, (table, iters, reseeded) = timed_fits(ix, a, a.steps, a.warmup)
        ix.close()
        emit({"what": "the same rows: CPU restatement (numpy + the oracle's C encoder, one thread; not the Go code) "
                      "against the device", "n": a.cpu_n, **shape, "cpu_restatement_s": t_cpu,
              "device_s_median": float(np.median(t)), "device_s_min": float(np.min(t)),
              "passes_per_segment": iters.tolist(), "reseeded": int(reseeded),
              "tables_bit_identical": bool(np.array_equal(table.view(np.uint32), want.table.view(np.uint32))),
              "passes_equal": iters.tolist() == want.iterations.tolist(), "reseeded_equal": reseeded == want.reseeded})


if __name__ == "__main__":
    main()
