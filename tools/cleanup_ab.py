#!/usr/bin/env python3
"""wv_index_cleanup_tombstones against the rebuild it replaces: time and recall.

Uniform random rows (--n x --d, l2-squared), M = --m, efConstruction = --efc.
For every --rates entry (per cent of the ids tombstoned, drawn without
replacement) one JSON line: the cleanup's wall time and counts on a freshly
built graph, recall@10 at --ef of the cleaned graph, and the time and recall
of wv_index_build_graph over the live rows alone (what a caller without the
cleanup has to do).  Recall is against the exact search of the live rows.
WV_BUILD_TRACE=1 makes the library print the cleanup's phases on stderr.

    python tools/cleanup_ab.py --n 1000000 --m 64 --rates 0.1 1 10 --out profiles/cleanup/ab.jsonl
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import weaviate_amd as W  # noqa: E402


def recall(ids, truth, k):
    return float(np.mean([len(set(a[:k]) & set(b[:k])) / k for a, b in zip(ids.tolist(), truth.tolist())]))


def timed(f):
    t = time.perf_counter()
    r = f()
    return r, (time.perf_counter() - t) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1000000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--m", type=int, default=64)
    ap.add_argument("--efc", type=int, default=128)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--batch-div", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--rates", type=float, nargs="*", default=[0.1, 1, 10])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    rng = np.random.default_rng(a.seed)
    base = rng.random((a.n, a.d), dtype=np.float32)
    qs = rng.random((a.queries, a.d), dtype=np.float32)
    lines = []
    for pct in a.rates:
        dead = np.sort(rng.choice(a.n, max(1, int(round(a.n * pct / 100))), replace=False))
        live = np.setdiff1d(np.arange(a.n), dead)
        ix = W.GPUVectorIndex(a.d, "l2-squared", capacity=a.n, max_connections=a.m)
        ix.upload_vectors(base)
        _, ms_build = timed(lambda: ix.build_graph(a.efc, a.seed, a.batch_div))
        ix.add_tombstones(dead)
        truth = ix.search_batch(qs, a.k, mode="exact")[0]
        counts, ms = timed(lambda: ix.cleanup_tombstones(a.efc, a.batch_div))
        r_clean = recall(ix.search_batch(qs, a.k, ef=a.ef, mode="hnsw")[0], truth, a.k)
        ix.close()
        ref = W.GPUVectorIndex(a.d, "l2-squared", capacity=len(live), max_connections=a.m)
        ref.upload_vectors(base[live])
        _, ms_ref = timed(lambda: ref.build_graph(a.efc, a.seed, a.batch_div))
        r_ref = recall(live[ref.search_batch(qs, a.k, ef=a.ef, mode="hnsw")[0].astype(np.int64)], truth, a.k)
        ref.close()
        rec = dict(rate_pct=pct, deleted=len(dead), cleanup_ms=round(ms, 1), flagged=counts["reassigned"] + counts["struck"],
                   flagged_share=round((counts["reassigned"] + counts["struck"]) / len(live), 4), struck=counts["struck"],
                   recall_cleaned=round(r_clean, 5), rebuild_live_ms=round(ms_ref, 1), recall_rebuilt=round(r_ref, 5),
                   build_all_ms=round(ms_build, 1), n=a.n, d=a.d, M=a.m, efc=a.efc, ef=a.ef, batch_div=a.batch_div)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
