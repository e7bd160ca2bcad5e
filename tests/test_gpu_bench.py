"""bench.py's multi-rank path on one GPU (-m gpu): a plain `--gpus 2`
invocation (no launcher) starts two ranks itself; with the gloo backend both
share this GPU.  The line must report n_gpus 2, weak scaling over the query
split, and the corpus-sharded leg (id-range shards, all-gather, device merge)
must answer rank 0's batch exactly like rank 0's whole-corpus search."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_bench_gpus2_gloo_rehearsal():
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--rows", "60000",
           "--nq", "1000", "--steps", "2", "--warmup", "1", "--full", "--no-cpu-baseline", "--no-hnsw-line"]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["n_gpus"] == 2 and r["scaling"] == "weak" and r["config"]["split"] == "query"
    assert r["value"] > 0
    assert r["corpus_sharded"]["ids_equal_query_split"] is True
    assert r["corpus_sharded"]["scaling"] == "strong"


def test_bench_refuses_mismatched_world_size():
    """CPU: the check runs before anything touches a GPU."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=60)
    assert out.returncode == 2 and "WORLD_SIZE" in out.stdout


def test_dump_outputs_formats_and_seeded_sample(tmp_path, monkeypatch):
    """CPU: ids and counts leave as float64, distances as float32; past the
    size limit the same seeded sample of query rows is kept on every call."""
    sys.path.insert(0, ROOT)
    import bench
    ids = np.arange(400 * 10, dtype=np.uint64).reshape(400, 10)
    ids[3, 9] = np.uint64(0xFFFFFFFFFFFFFFFF)
    d = np.linspace(0, 1, 400 * 10, dtype=np.float32).reshape(400, 10)
    n = np.full(400, 10, np.int32)
    bench.dump_outputs(str(tmp_path / "a"), ids=ids, dists=d, counts=n)
    got = {k: np.load(tmp_path / "a" / (k + ".npy")) for k in ("ids", "dists", "counts")}
    assert got["ids"].dtype == np.float64 and got["counts"].dtype == np.float64 and got["dists"].dtype == np.float32
    assert np.array_equal(got["ids"][:3].astype(np.uint64), ids[:3]) and got["ids"][3, 9] == 2.0 ** 64
    assert np.array_equal(got["dists"], d) and not (tmp_path / "a" / "rows.npy").exists()
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 100 * (10 * 8 + 10 * 4 + 8 + 8))
    for sub in ("b", "c"):
        bench.dump_outputs(str(tmp_path / sub), ids=ids, dists=d, counts=n)
    rows = np.load(tmp_path / "b" / "rows.npy").astype(np.int64)
    assert len(rows) == 100 and np.array_equal(rows, np.load(tmp_path / "c" / "rows.npy").astype(np.int64))
    assert np.array_equal(np.load(tmp_path / "b" / "dists.npy"), d[rows])
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 100 * 136 + 4 * 128


@pytest.mark.gpu
def test_bench_plain_run_is_lean_and_dumps_its_last_step(tmp_path):
    """A plain run prints the headline line without the --full legs, times
    exactly --steps steps, and --dump-outputs holds what the exact path
    returned: the restatement's flatSearch ids and distance bits on the same
    counter-based inputs."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import pyoracle as O
    from bench import counter_uniform
    n, d, nq, k = 20000, 64, 200, 10
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "3", "--warmup", "1", "--rows",
           str(n), "--dim", str(d), "--nq", str(nq), "--dump-outputs", str(tmp_path / "out")]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=110)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["steps"] == 3 and r["ms_per_step"] > 0 and r["unit"] == "queries/s" and r["higher_is_better"] is True
    assert abs(r["value"] - nq / (r["ms_per_step"] * 1e-3)) <= 0.01 * r["value"]
    for key in ("cpu_baseline", "parity_sample", "wide_k", "hnsw_c1", "hnsw_c3", "exact_c4", "hnsw_c5_sharded"):
        assert key not in r, key
    ids = np.load(tmp_path / "out" / "ids.npy")
    dists = np.load(tmp_path / "out" / "dists.npy")
    counts = np.load(tmp_path / "out" / "counts.npy")
    assert ids.dtype == np.float64 and dists.dtype == np.float32 and ids.shape == dists.shape == (nq, k)
    oi, od, on = O.flat_scan(O.L2, counter_uniform(1, 0, n, d), counter_uniform(2, 0, nq, d), k)
    assert np.array_equal(ids.astype(np.uint64), oi)
    assert np.array_equal(dists.view(np.uint32), od.view(np.uint32))
    assert np.array_equal(counts.astype(np.int64), np.asarray(on).astype(np.int64))


@pytest.mark.gpu
def test_bench_sharded_hnsw_two_ranks_equal_per_shard_restatement(tmp_path):
    """configs[4]'s layout (north_star: corpus sharded, local top-k, merge over
    RCCL): `--workload hnsw --split corpus` on 2 ranks (gloo, one GPU) -- each
    rank builds the graph of its id range on the GPU and searches the same
    batch; the merged ids must equal the restatement searching each rank's
    own graph, offset to global ids and merged by (dist, id)
    (index.go:967-1044), up to the order among equal distances."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    sys.path.insert(0, ROOT)
    import pyoracle as O
    from bench import counter_gauss
    from helpers import merge_lists, same_tie_aware
    n, d, nq, k, ef = 40000, 96, 300, 10, 64
    env = dict(os.environ)
    env.pop("WORLD_SIZE", None)
    dump = str(tmp_path / "rank%(rank)d.npz")
    cmd = [sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--workload",
           "hnsw", "--split", "corpus", "--rows", str(n), "--dim", str(d), "--nq", str(nq), "--data", "gauss",
           "--M", "16", "--efc", "64", "--ef", str(ef), "--steps", "2", "--warmup", "1", "--no-cpu-baseline",
           "--concurrency", "", "--dump-ids", dump]
    out = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=150)
    assert out.returncode == 0, out.stderr[-3000:]
    r = json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])
    assert r["n_gpus"] == 2 and r["scaling"] == "strong" and r["config"]["split"] == "corpus"
    qs = counter_gauss(2, 0, nq, d)
    parts, merged = [], None
    for rank in range(2):
        z = np.load(dump % {"rank": rank})
        lo, nl = int(z["lo"]), int(z["n_local"])
        g = {key[2:]: (z[key] if z[key].ndim else int(z[key])) for key in z.files if key.startswith("g_")}
        ref = O.Index(d, "l2-squared", 16, 64, capacity=nl, seed=1)
        ref.import_graph(counter_gauss(1, lo, nl, d), g)
        oi, od, on, _ = ref.search_batch(qs, k, ef, threads=8)
        # the rank's own shard answer is the restatement's on that graph
        for i in range(nq):
            same_tie_aware(z["shard_ids"][i] - np.uint64(lo), z["shard_dists"][i], oi[i], od[i])
        parts.append((oi + np.uint64(lo), od, on))
        merged = (z["ids"], z["dists"])
    mi, md, _ = merge_lists(parts, k)
    for i in range(nq):
        same_tie_aware(merged[0][i], merged[1][i], mi[i], md[i])
