"""Row-sharded products with the REAL HIP blocks: world_size 2 on one GPU (gloo process group,
both ranks on cuda:0), shards cut by tabmat_amd.distributed.shard(); the all-reduced results
must equal the single-rank HIP result and the oracle."""
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, device_resident, backend="gloo", ndev=1, n=30_011, rows_low=False):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(rank % ndev)
    dist.init_process_group(backend, rank=rank, world_size=world)
    try:
        import _cases as cs
        from _gpu_util import to_tm_split
        from oracle import oracle as orc
        from tabmat_amd.distributed import shard

        specs, idx = cs.mixed_specs(n, 24, 70, (11, 5, 3), seed=11)
        full = to_tm_split(specs, idx)
        if device_resident:
            full.to_device()          # shards are then cut in HBM
        blocks = [cs.to_oracle_block(s) for s in specs]
        rng = np.random.default_rng(5)
        d = rng.random(n)
        w = rng.standard_normal(n)
        v = rng.standard_normal(full.shape[1])
        rows_g = np.sort(rng.choice(n, n // 3, replace=False))
        if rows_low:                      # no selected row beyond the third shard of eight
            rows_g = np.sort(rng.choice(3 * (n // 8), n // 10, replace=False))
        sh = shard(full, always_reduce=True)     # world 1: the collective is issued all the same
        lo, hi = sh.bounds
        assert sh.local.shape[0] == hi - lo
        got = sh.sandwich_global(d)
        got_rows = sh.sandwich_global(d, rows_g)
        got_dev = sh.sandwich(torch.from_numpy(d[lo:hi]).cuda())        # device in -> device out
        got_tmv = sh.transpose_matvec_global(w)
        got_mv = sh.matvec(v)
        want = orc.split_sandwich(blocks, idx, d)
        want_rows = orc.split_sandwich(blocks, idx, d, rows_g)
        want_tmv = orc.split_transpose_matvec(blocks, idx, w)
        want_mv = orc.split_matvec(blocks, idx, v)[lo:hi]
        single = full.sandwich(d)

        def rel(a, b):
            return float(np.abs(np.asarray(a) - b).max() / max(np.abs(b).max(), 1e-300))

        errs = dict(sand=rel(got, want), rows=rel(got_rows, want_rows),
                    dev=rel(got_dev.cpu().numpy(), want), tmv=rel(got_tmv, want_tmv),
                    mv=rel(got_mv, want_mv), single=rel(got, single))
        q.put((rank, errs, (lo, hi)))
    finally:
        dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("device_resident", [False, True])
def test_world2_hip_shards_match_single_rank_and_oracle(device_resident):
    world = 2
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, device_resident)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    bounds = sorted(r[2] for r in res)
    assert bounds[0][0] == 0 and bounds[0][1] == bounds[1][0] and bounds[1][1] == 30_011
    for rank, errs, _ in res:
        for k, e in errs.items():
            assert e < 1e-10, (rank, k, e)


def _run(world, device_resident, backend, ndev):
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, device_resident, backend, ndev))
             for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=600) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    for rank, errs, _ in res:
        for k, e in errs.items():
            assert e < 1e-10, (rank, k, e)
    return res


@pytest.mark.gpu
def test_rccl_all_reduce_world1():
    """backend "nccl" (= RCCL) on one GPU: the communicator is created and the all-reduce of the
    p x p device result and of the numpy-convention result run through RCCL (world size 1 -- the
    code path that the 8-GPU job takes, minus the xGMI transfers)."""
    res = _run(1, True, "nccl", 1)
    assert res[0][2] == (0, 30_011)


@pytest.mark.gpu
def test_rccl_all_reduce_world2_two_devices():
    """Two ranks on two GPUs over RCCL, when the box has two."""
    if torch.cuda.device_count() < 2:
        pytest.skip("needs two visible GPUs (RCCL refuses two ranks on one device)")
    _run(2, True, "nccl", 2)


@pytest.mark.gpu
def test_bench_two_ranks_gloo():
    """`python bench.py --gpus 2` end to end on ONE GPU: the script spawns its own two ranks through
    torch.distributed.run, the ranks share the device over the gloo backend (TABMAT_BENCH_BACKEND=gloo; RCCL
    refuses two ranks on one device), every rank times its own shard between barriers and rank 0 prints the
    one JSON line with the whole-job value (the 8-GPU job runs the same code over RCCL)."""
    import json
    import subprocess

    env = dict(os.environ, TABMAT_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    env.pop("WORLD_SIZE", None)
    env.pop("RANK", None)
    out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rows", "200000",
                          "--steps", "3", "--warmup", "1", "--full", "--no-traffic", "--no-cpu-baseline"],
                         env=env, capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stderr[-2000:]
    line = [l for l in out.stdout.splitlines() if l.startswith("{")][-1]
    r = json.loads(line)
    assert r["n_gpus"] == 2 and r["steps"] == 3 and r["scaling"] == "weak"
    assert r["config"]["sharding"] == "rows" and r["config"]["collective"].startswith("all_reduce")
    assert r["config"]["rows_per_gpu"] == 200000
    assert np.isfinite(r["value"]) and r["value"] > 0 and r["ms_per_step"] > 0
    assert r["roofline"]["kernel_ms"] > 0


@pytest.mark.gpu
def test_world8_hip_shards_uneven_rows_and_empty_row_lists():
    """shard() at the world size of the 8-GPU job (BASELINE configs[4]) with the REAL HIP blocks: eight ranks over
    gloo on the one device, n = 20 003 rows (not divisible by 8), device-resident blocks cut in HBM, and a `rows=`
    list that leaves ranks 3..7 without a selected row (their zero partial still joins the all-reduce).  Every rank
    must hold the oracle's result afterwards."""
    world, n = 8, 20_003
    port = _free_port()
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, True, "gloo", 1, n, True)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=900) for _ in range(world)]
    for p in procs:
        p.join(timeout=120)
        assert p.exitcode == 0
    bounds = sorted(r[2] for r in res)
    assert bounds[0][0] == 0 and bounds[-1][1] == n
    assert all(bounds[i][1] == bounds[i + 1][0] for i in range(world - 1))
    assert sorted(h - l for l, h in bounds) == [2500] * 5 + [2501] * 3
    for rank, errs, _ in res:
        for k, e in errs.items():
            assert e < 1e-10, (rank, k, e)


def _bench_json(args, env, timeout=1500):
    import json
    import subprocess

    out = subprocess.run(args, env=env, capture_output=True, text=True, timeout=timeout)
    assert out.returncode == 0, out.stderr[-3000:]
    return json.loads([l for l in out.stdout.splitlines() if l.startswith("{")][-1])


@pytest.mark.gpu
def test_bench_eight_ranks_gloo():
    """`python bench.py --gpus 8` end to end, the launch of the 8-GPU scaling run minus the hardware: eight ranks
    (self-spawned through torch.distributed.run), gloo, all on the one device.  The JSON line must carry what the
    driver and the judge read off the first real 8-GPU run: n_gpus, weak scaling, the `ranks` block (backend, one
    time per rank, RCCL rank count = 0 under gloo), the collective, and the start-up costs (synth / ingest)."""
    import time

    env = dict(os.environ, TABMAT_BENCH_BACKEND="gloo", HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        env.pop(k, None)
    t0 = time.time()
    r = _bench_json([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "8", "--rows", "100000",
                     "--steps", "3", "--warmup", "1", "--full", "--no-traffic", "--no-cpu-baseline"], env)
    wall = time.time() - t0
    assert r["n_gpus"] == 8 and r["steps"] == 3 and r["scaling"] == "weak" and r["higher_is_better"] is True
    assert r["config"]["sharding"] == "rows" and r["config"]["collective"].startswith("all_reduce")
    assert r["config"]["rows_per_gpu"] == 100000
    rk = r["ranks"]
    assert rk["backend"] == "gloo" and rk["world_size"] == 8 and rk["rccl_ranks"] == 0
    assert len(rk["ms_per_step_by_rank"]) == 8 and all(t > 0 for t in rk["ms_per_step_by_rank"])
    assert rk["ms_per_step_max_rank"] == max(rk["ms_per_step_by_rank"])
    assert abs(r["ms_per_step"] - rk["ms_per_step_max_rank"]) < 1e-3        # the job's time = the slowest rank
    # whole-job value: eight shards' bytes over the slowest rank's time
    assert r["value"] > 0 and r["ingest_ms"] > 0 and r["synth_ms"] > 0 and r["resident_bytes"] > r["data_bytes"] > 0
    assert wall < 900, f"8-rank start-up + 4 steps took {wall:.0f} s"


@pytest.mark.gpu
def test_bench_one_rank_under_torchrun_matches_plain_run():
    """The driver launches N = 1 as plain `python bench.py` and N > 1 through torch.distributed.run; one rank under
    the launcher must be the same job: same keys, same workload, no collective, and the same value up to timing
    noise."""
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    common = ["--gpus", "1", "--rows", "2000000", "--steps", "10", "--warmup", "3", "--no-traffic",
              "--no-cpu-baseline"]
    plain = _bench_json([sys.executable, os.path.join(ROOT, "bench.py")] + common, env)
    launched = _bench_json([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1",
                            "--master-addr", "127.0.0.1", "--master-port", str(_free_port()),
                            os.path.join(ROOT, "bench.py")] + common, env)
    assert set(plain) == set(launched)
    for k in ("metric", "unit", "n_gpus", "steps", "warmup", "scaling", "dtype", "data", "config"):
        assert plain[k] == launched[k], k
    assert launched["config"]["collective"] == "none" and "ranks" not in launched
    assert abs(plain["value"] - launched["value"]) <= 0.1 * plain["value"], (plain["value"], launched["value"])
