#!/usr/bin/env python3
"""SearchByVectorDistance on raw vectors: ms per wv_search_by_vector_distance_batch
with the f16 MFMA threshold filter (wv_index_set_sbd_key_pass) on or off.

A flat 1M x 128 L2 index of synthetic Gaussian rows (tools/synth.py, written on
the device); batches of --nq queries, no filter; per query a target that puts
about --within rows inside it: the 100th-nearest distance from the exact
search, or for larger sets that quantile of the query's distances to a 100k-row
sample.  Wall time around the C call, host in to host out: --warmup calls,
then --steps timed ones; one JSON line per (nq, within) with the median,
minimum, maximum and inter-quartile range (the run-to-run spread), the mean
|Q|, the filter's candidates per query and candidates / |Q| (how wide the
certificate's margin is), and a fingerprint of the answers to compare
processes.  --mode off leaves the switch alone; WV_LIBPATH names another build
(a parent build has no switch: only --mode off runs there), and a driver
alternates processes of the two builds.  --dim above 128 with --wide measures
the wide filter (wv_index_set_sbd_wide_key_pass, wv_sbd_h16w.hip) instead;
--metric picks l2-squared (the default), dot or cosine-dot.

    python tools/bench_sbd_h16.py --mode on --out profiles/sbd_h16/new_on.jsonl
    python tools/bench_sbd_h16.py --dim 768 --metric dot --wide --mode on --out profiles/sbd_h16w/new_on.jsonl
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np
import torch

torch.cuda.init()   # (before the library is loaded: torch brings its own HIP runtime and must see the device first)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from weaviate_amd import _lib  # noqa: E402

if os.environ.get("WV_LIBPATH"):
    _probe = C.CDLL(_lib.LIBPATH)
    for _name in [s for s in _lib.SIGNATURES if not hasattr(_probe, s)]:
        del _lib.SIGNATURES[_name]
import weaviate_amd as W  # noqa: E402


def vp(a):
    return C.c_void_p(a.ctypes.data) if a is not None else None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--within", type=int, nargs="+", default=[100, 5000])
    ap.add_argument("--metric", choices=["l2-squared", "dot", "cosine-dot"], default="l2-squared")
    ap.add_argument("--wide", action="store_true", help="--mode on sets wv_index_set_sbd_wide_key_pass (D > 128)")
    ap.add_argument("--mode", choices=["on", "off"], default="on")
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--cap", type=int, default=256, help="results written per query")
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import synth
    switch = "wv_index_set_sbd_wide_key_pass" if a.wide else "wv_index_set_sbd_key_pass"
    has_switch = "wv_index_set_sbd_key_pass" in _lib.SIGNATURES
    if a.mode == "on" and switch not in _lib.SIGNATURES:
        raise SystemExit(f"this build has no {switch}: only --mode off runs")
    lib = W.lib()
    nq_max = max(a.nq)
    ix = W.GPUVectorIndex(a.dim, a.metric, capacity=a.n)
    t = torch.empty((a.n, a.dim), dtype=torch.float32, device="cuda")
    synth.fill("gauss", 1, 0, t)
    torch.cuda.synchronize()
    ix.upload_vectors_device(t.data_ptr(), a.n, first_id=0)
    tq = torch.empty((nq_max, a.dim), dtype=torch.float32, device="cuda")
    synth.fill("gauss", 2, 0, tq)
    qs = np.ascontiguousarray(tq.cpu().numpy())
    sample = t[torch.randperm(a.n, device="cuda", generator=torch.Generator("cuda").manual_seed(3))[:100_000]]
    if a.metric == "l2-squared":
        ds = torch.cdist(tq, sample).square_()   # [nq_max, 100k]
    elif a.metric == "dot":
        ds = -(tq @ sample.T)
    else:
        ds = 1.0 - torch.nn.functional.normalize(tq, dim=1) @ torch.nn.functional.normalize(sample, dim=1).T
    targets = {}
    for w in a.within:
        if w <= 256:
            _, kd, kn = ix.search_batch(qs, w, mode="exact")
            targets[w] = np.ascontiguousarray(kd[:, w - 1])
        else:
            k = max(1, int(round(w * sample.shape[0] / a.n)))
            targets[w] = np.ascontiguousarray(ds.kthvalue(k, dim=1).values.cpu().numpy().astype(np.float32))
    del t, sample, ds
    if a.mode == "on":
        (ix.set_sbd_wide_key_pass if a.wide else ix.set_sbd_key_pass)(True)
    out = None
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        out = open(a.out, "a")
    for nq in a.nq:
        oi, od, on = np.zeros((nq, a.cap), np.uint64), np.zeros((nq, a.cap), np.float32), np.zeros(nq, np.int64)
        for w in a.within:
            tg = np.ascontiguousarray(targets[w][:nq])

            def call():
                rc = lib.wv_search_by_vector_distance_batch(ix._h, vp(qs), nq, vp(tg), -1, None, 0, 0, vp(oi), vp(od),
                                                            a.cap, vp(on))
                if rc:
                    raise RuntimeError(lib.wv_last_error().decode())

            ms = []
            for step in range(a.warmup + a.steps):
                t0 = time.perf_counter()
                call()
                if step >= a.warmup:
                    ms.append((time.perf_counter() - t0) * 1e3)
            q1, med, q3 = np.percentile(ms, [25, 50, 75])
            m = np.minimum(on, a.cap)
            rec = {"label": a.label, "mode": a.mode, "n": a.n, "dim": a.dim, "metric": a.metric, "wide": a.wide,
                   "nq": nq, "within": w,
                   "steps": a.steps, "warmup": a.warmup, "ms_median": float(med), "ms_min": float(min(ms)),
                   "ms_max": float(max(ms)), "ms_iqr": float(q3 - q1), "results_median": float(np.median(on)),
                   "results_mean": float(on.mean()),
                   "answer_sum": int(sum(int(oi[i, : m[i]].sum()) for i in range(nq))) + int(on.sum()),
                   "WV_LIBPATH": os.environ.get("WV_LIBPATH")}
            if has_switch:
                st = ix.last_sbd_key_pass_stats()
                rec["key_pass"] = st
                if st["key_pass_queries"]:
                    rec["candidates_per_query"] = st["candidates"] / nq
                    rec["candidates_per_result"] = st["candidates"] / max(1, int(on.sum()))
            line = json.dumps(rec)
            print(line, flush=True)
            if out:
                out.write(line + "\n")
                out.flush()
    ix.close()


if __name__ == "__main__":
    main()
