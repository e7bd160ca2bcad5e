#!/usr/bin/env python3
"""wv_index_extend_graph against a whole build: time and recall.

Uniform random rows (--n x --d, l2-squared), M = --m, efConstruction = --efc.
One JSON line per leg:

  build          upload every row, wv_index_build_graph, recall@10 at --ef of
                 the graph against the exact answers (the exact search of the
                 same index).  This leg calls nothing new, so with WV_LIBPATH
                 naming another build of the library it measures that build.
  extend_<pct>   upload and build the first (100 - pct) % of the rows (n0 is
                 moved to the nearest batch boundary of the schedule unless
                 --off-boundary), upload the rest, wv_index_extend_graph: the
                 time of that call alone, the time of the build before it, and
                 the recall of the extended graph.

Times are wall times around the C call (the call returns when the device is
done).  WV_BUILD_TRACE=1 in the environment makes the library print, on
stderr, the extension's preparation -- array growth, the counts pass, the
`upper` re-layout -- and the batch loop's phases.

    python tools/extend_graph_ab.py --n 1000000 --shares 1 5 20 --out profiles/extend_graph/ab.jsonl
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


def boundaries(n, div):
    b, done = [1], 1
    while done < n:
        done += min(n - done, max(1, min(16384, done // div)))
        b.append(done)
    return b


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
    ap.add_argument("--m", type=int, default=16)
    ap.add_argument("--efc", type=int, default=128)
    ap.add_argument("--ef", type=int, default=64)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--queries", type=int, default=2000)
    ap.add_argument("--batch-div", type=int, default=32)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--shares", type=float, nargs="*", default=[1, 5, 20], help="per cent of the rows extended")
    ap.add_argument("--no-build", action="store_true", help="skip the whole-build leg")
    ap.add_argument("--off-boundary", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    rng = np.random.default_rng(a.seed)
    base = rng.random((a.n, a.d), dtype=np.float32)
    qs = rng.random((a.queries, a.d), dtype=np.float32)
    lines = []

    def emit(rec):
        rec.update(n=a.n, d=a.d, M=a.m, efc=a.efc, ef=a.ef, batch_div=a.batch_div)
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)

    def new_index():
        return W.GPUVectorIndex(a.d, "l2-squared", capacity=a.n, max_connections=a.m)

    truth = None

    def measure(ix, rec):
        nonlocal truth
        if truth is None:
            truth = ix.search_batch(qs, a.k, mode="exact")[0]
        ids = ix.search_batch(qs, a.k, ef=a.ef, mode="hnsw")[0]
        rec["recall"] = round(recall(ids, truth, a.k), 5)
        emit(rec)

    if not a.no_build:
        ix = new_index()
        ix.upload_vectors(base)
        _, ms = timed(lambda: ix.build_graph(a.efc, a.seed, a.batch_div))
        measure(ix, dict(leg="build", rows=a.n, ms=round(ms, 1)))
        ix.close()
    bounds = np.asarray(boundaries(a.n, a.batch_div))
    for pct in a.shares:
        n0 = int(round(a.n * (1 - pct / 100)))
        if not a.off_boundary:
            n0 = int(bounds[np.argmin(np.abs(bounds - n0))])
        ix = new_index()
        ix.upload_vectors(base[:n0])
        _, ms0 = timed(lambda: ix.build_graph(a.efc, a.seed, a.batch_div))
        ix.upload_vectors(base[n0:], first_id=n0)
        k, ms = timed(lambda: ix.extend_graph(a.efc, a.seed, a.batch_div))
        assert k == a.n - n0, (k, a.n - n0)
        info = ix.graph_info()
        measure(ix, dict(leg=f"extend_{pct:g}", rows=k, n0=n0, ms=round(ms, 1), build_n0_ms=round(ms0, 1),
                         max_level=info["max_level"], n_upper=info["n_upper"]))
        ix.close()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
