#!/usr/bin/env python3
"""Exact k-NN for k > 256: ms per wv_search_batch call, large-k route on against off.

Times the wall time around the C call, host in to host out, of one exact batch
of --nq queries at each --k over an l2-squared index of --n x --dim standard
normal rows.  The route is a per-index switch, so a process runs one variant:
"off" (a scan and sort per query, the library's default) or "on"
(wv_index_set_large_k), the latter also with the f16 threshold filter
(wv_index_set_sbd_key_pass).  Without --child the tool starts --rounds fresh
child processes per variant, alternating off and on, one at a time.

One JSON line per (variant, key pass, k, nq): median, minimum, maximum and
inter-quartile range of --steps timed calls after --warmup, the route's counts,
the device time of one further call by stage (timing events: bound pass,
threshold pass, sort + emit) and the SHA-256 of the answers, to compare the
processes.  For up to 16 queries the bound is restated on the host (the 36th
smallest distance over every (k / 16)-th row) to give the median |Q| / k.

    python tools/bench_large_k.py --out profiles/large_k/ab.jsonl
"""
import argparse
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def summary(t):
    q1, med, q3 = np.percentile(t, [25, 50, 75])
    return {"ms_median": float(med), "ms_min": float(np.min(t)), "ms_max": float(np.max(t)), "ms_iqr": float(q3 - q1)}


def listed_over_k(base, qs, k):
    """median over qs of |{rows within tau}| / k, tau restated on the host"""
    step = max(1, k // 16)
    d = ((base * base).sum(1)[None, :] - 2.0 * (qs @ base.T)).astype(np.float64)   # + |q|^2: the same order
    tau = np.partition(d[:, ::step], 35, axis=1)[:, 35]
    return float(np.median((d <= tau[:, None]).sum(1) / k))


def child(a):
    import weaviate_amd as W
    lib = W.lib()
    rng = np.random.default_rng(5)
    base = rng.standard_normal((a.n, a.dim)).astype(np.float32)
    qs_all = np.ascontiguousarray(rng.standard_normal((max(a.nq), a.dim)).astype(np.float32))
    ix = W.GPUVectorIndex(a.dim, "l2-squared", capacity=a.n)
    ix.upload_vectors(base)
    ix.set_large_k(a.child == "on")
    out = open(a.out, "a") if a.out else None
    vp = lambda x: C.c_void_p(x.ctypes.data)   # noqa: E731
    for key_pass in ([False, True] if a.child == "on" else [False]):
        ix.set_sbd_key_pass(key_pass)
        for k in a.k:
            ratio = listed_over_k(base, qs_all[:16], k) if a.child == "on" and not key_pass else None
            for nq in a.nq:
                qs = np.ascontiguousarray(qs_all[:nq])
                oi, od, on = np.zeros((nq, k), np.uint64), np.zeros((nq, k), np.float32), np.zeros(nq, np.int32)

                def call():
                    if lib.wv_search_batch(ix._h, vp(qs), nq, k, 0, None, 0, 0, W.MODE_EXACT, vp(oi), vp(od), vp(on)):
                        raise RuntimeError(lib.wv_last_error().decode())

                t = []
                for step in range(a.warmup + a.steps):
                    t0 = time.perf_counter()
                    call()
                    if step >= a.warmup:
                        t.append((time.perf_counter() - t0) * 1e3)
                batched, legacy = ix.last_large_k_stats()
                ix.set_timing(True)
                call()
                kt = ix.last_kernel_times()
                ix.set_timing(False)
                rec = {"label": a.label, "variant": a.child, "key_pass": key_pass, "n": a.n, "dim": a.dim, "k": k,
                       "nq": nq, "steps": a.steps, "warmup": a.warmup, **summary(t), "batched_queries": batched,
                       "legacy_queries": legacy, "fallback_share": legacy / nq, "listed_over_k_median": ratio,
                       "bound_ms": kt["seed_ms"], "threshold_ms": kt["bf_mfma_ms"], "sort_emit_ms": kt["bf_finalize_ms"],
                       "answers_sha256": hashlib.sha256(oi.tobytes() + od.tobytes() + on.tobytes()).hexdigest()}
                line = json.dumps(rec)
                print(line, flush=True)
                if out:
                    out.write(line + "\n")
                    out.flush()
    ix.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--k", type=int, nargs="+", default=[257, 1000, 4096])
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--child", choices=["on", "off"], default=None)
    ap.add_argument("--child-timeout", type=int, default=240)
    ap.add_argument("--label", default="")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    if a.child:
        return child(a)
    for r in range(a.rounds):
        for v in ("off", "on"):
            # a fresh process per variant; the first failure ends the run
            subprocess.run([sys.executable, os.path.abspath(__file__), *sys.argv[1:], "--child", v, "--label",
                            f"{a.label}r{r}"], check=True, timeout=a.child_timeout)


if __name__ == "__main__":
    main()
