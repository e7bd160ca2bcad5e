#!/usr/bin/env python3
"""Per-query allow lists as ids against per-query bitmaps, same build, same batch.

Times one batch two ways, alternating: wv_search_batch_ids (the sparse flat
kernel) and wv_search_batch with one bitmap row per query (the route such a
batch took before).  Host in to host out around the C call, inputs prepared
beforehand; the sparse kernel's own time from HIP events in a pass of its own;
its share of HBM peak counts sum(L) * D * 4 gathered bytes.  Then the
10,000-id case through a 64-thread Batcher with WV_BATCHER_IDS=1 and 0.
One JSON line per measurement (stdout, and --out).

    python tools/bench_flat_ids.py --out profiles/flat_ids/bench.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from weaviate_amd import _lib  # noqa: E402

if os.environ.get("WV_LIBPATH"):   # an older build is bound as far as its symbols go
    _probe = C.CDLL(_lib.LIBPATH)
    for _name in [s for s in _lib.SIGNATURES if not hasattr(_probe, s)]:
        del _lib.SIGNATURES[_name]
import weaviate_amd as W  # noqa: E402

HBM_PEAK = 8.0e12   # bytes/s (spec)


def vp(a):
    return C.c_void_p(a.ctypes.data)


def emit(rec, out):
    line = json.dumps(rec)
    print(line, flush=True)
    if out:
        out.write(line + "\n")
        out.flush()


def make_lists(rng, n, nq, L):
    return [np.sort(rng.choice(n, L, replace=False)).astype(np.uint64) for _ in range(nq)]


def bench_batch(ix, n, qs, k, lists, reps, warmup, out):
    nq = len(lists)
    L = int(lists[0].size)
    flat = np.ascontiguousarray(np.concatenate(lists))
    off = np.zeros(nq + 1, np.uint64)
    off[1:] = np.cumsum([a.size for a in lists])
    words = (n + 63) // 64
    bits = np.zeros((nq, words), np.uint64)
    for i, a in enumerate(lists):
        np.bitwise_or.at(bits[i], (a >> np.uint64(6)).astype(np.int64), np.uint64(1) << (a & np.uint64(63)))
    q = np.ascontiguousarray(qs[:nq])
    res = {r: (np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32))
           for r in ("ids", "bitmap")}
    lib = W.lib()

    def run(route):
        oi, od, on = res[route]
        t0 = time.perf_counter()
        if route == "ids":
            rc = lib.wv_search_batch_ids(ix._h, vp(q), nq, k, 0, vp(flat), vp(off), W.MODE_AUTO, vp(oi), vp(od), vp(on))
        else:
            rc = lib.wv_search_batch(ix._h, vp(q), nq, k, 0, vp(bits), n, words, W.MODE_AUTO, vp(oi), vp(od), vp(on))
        dt = time.perf_counter() - t0
        if rc:
            raise RuntimeError(lib.wv_last_error().decode())
        return dt * 1e3

    for _ in range(warmup):
        run("ids")
        run("bitmap")
    same = (res["ids"][0].tolist() == res["bitmap"][0].tolist()
            and np.array_equal(res["ids"][1].view(np.uint32), res["bitmap"][1].view(np.uint32))
            and res["ids"][2].tolist() == res["bitmap"][2].tolist())
    t = {"ids": [], "bitmap": []}
    for _ in range(reps):
        for r in ("ids", "bitmap"):
            t[r].append(run(r))
    run("ids")
    st = ix.last_sparse_stats()
    # the kernel alone: events on, a pass of its own
    ix.set_timing(True)
    kt = []
    for _ in range(max(5, reps // 2)):
        run("ids")
        kt.append(ix.last_sparse_time())
    ix.set_timing(False)
    kms = float(np.median(kt))
    gathered = float(nq) * L * qs.shape[1] * 4
    rec = {"what": "batch", "n": n, "dim": int(qs.shape[1]), "k": k, "nq": nq, "list_len": L, "reps": reps,
           "ids_ms_p50": float(np.median(t["ids"])), "ids_ms_min": float(np.min(t["ids"])),
           "ids_ms_p90": float(np.percentile(t["ids"], 90)),
           "bitmap_ms_p50": float(np.median(t["bitmap"])), "bitmap_ms_min": float(np.min(t["bitmap"])),
           "bitmap_ms_p90": float(np.percentile(t["bitmap"], 90)),
           "speedup_p50": float(np.median(t["bitmap"]) / np.median(t["ids"])),
           "sparse_kernel_ms": kms, "gathered_bytes": gathered,
           "hbm_peak_fraction": gathered / (kms * 1e-3) / HBM_PEAK if kms > 0 else None,
           "results_identical": bool(same), "sparse_stats": st}
    emit(rec, out)
    return rec


def bench_batcher(ix, n, qs, k, lists, send_ids, per_thread, out):
    os.environ["WV_BATCHER_IDS"] = "1" if send_ids else "0"
    b = W.Batcher(ix, max_batch=256, max_wait_us=0)
    nt = 64
    lat = [[] for _ in range(nt)]
    answers = [None] * nt

    def worker(t, rounds, record):
        for r in range(rounds):
            i = (t + nt * r) % len(lists)
            t0 = time.perf_counter()
            a = b.search_ids(qs[i % len(qs)], k, lists[i])
            if record:
                lat[t].append((time.perf_counter() - t0) * 1e3)
                if r == 0:
                    answers[t] = a

    def go(rounds, record):
        th = [threading.Thread(target=worker, args=(t, rounds, record)) for t in range(nt)]
        t0 = time.perf_counter()
        for x in th:
            x.start()
        for x in th:
            x.join()
        return time.perf_counter() - t0

    go(3, False)
    wall = go(per_thread, True)
    stats = b.stats()
    b.close()
    al = np.concatenate([np.asarray(x) for x in lat])
    rec = {"what": "batcher", "WV_BATCHER_IDS": int(send_ids), "threads": nt, "list_len": int(lists[0].size), "k": k,
           "requests": int(al.size), "qps": float(al.size / wall), "p50_ms": float(np.percentile(al, 50)),
           "p99_ms": float(np.percentile(al, 99)), "batches": stats["batches"],
           "sparse_stats": ix.last_sparse_stats()}
    emit(rec, out)
    return answers


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--batches", type=int, nargs="+", default=[256, 16])
    ap.add_argument("--lens", type=int, nargs="+", default=[1000, 10000, 39999])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--batcher-requests", type=int, default=40, help="timed requests per thread (0: skip the batcher)")
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
    for L in a.lens:
        lists = make_lists(rng, a.n, max(a.batches), L)
        for nq in a.batches:
            bench_batch(ix, a.n, qs, a.k, lists[:nq], a.reps, a.warmup, out)
        if L == 10000 and a.batcher_requests:
            got = {s: bench_batcher(ix, a.n, qs, a.k, lists, s, a.batcher_requests, out) for s in (True, False)}
            same = all(x[0].tolist() == y[0].tolist() and np.array_equal(x[1].view(np.uint32), y[1].view(np.uint32))
                       for x, y in zip(got[True], got[False]))
            emit({"what": "batcher_check", "answers_identical": bool(same)}, out)
    ix.close()


if __name__ == "__main__":
    main()
