"""RowShardedMatrix.sandwich_and_transpose_matvec on CPU: gloo process groups, oracle-injected local products.  The
pair (H, g) must equal the separate sharded sandwich / transpose_matvec, and each fused call must issue exactly ONE
all_reduce (H and g packed into one buffer)."""
import os
import socket
import sys

import numpy as np
import torch.distributed as dist
import torch.multiprocessing as mp

import _cases as cs

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q, rows_mode):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from oracle import oracle as orc
        from tabmat_amd.distributed import RowShardedMatrix, bucket_rows, shard_bounds

        n = 1001
        specs, idx = cs.mixed_specs(n, 8, 20, (6, 4), seed=7)
        blocks = [cs.to_oracle_block(s) for s in specs]
        rng = np.random.default_rng(0)
        d = rng.random(n)
        v = rng.standard_normal(n)
        rows_g = np.sort(rng.choice(n, 600, replace=False))
        if rows_mode == "low":            # every selected row in the first shards: the others get an empty list
            rows_g = np.sort(rng.choice(3 * (n // 8), 200, replace=False))
        cols = np.sort(rng.choice(sum(len(i) for i in idx), 17, replace=False))

        lo, hi = shard_bounds(n, world, rank)
        local_specs = []
        for s in specs:
            if s[0] == "dense":
                local_specs.append(("dense", np.ascontiguousarray(s[1][lo:hi])))
            elif s[0] == "sparse":
                local_specs.append(("sparse", s[1].tocsr()[lo:hi].tocsc()))
            else:
                local_specs.append(("cat", s[1][lo:hi], s[2], s[3]))
        lblocks = [cs.to_oracle_block(s) for s in local_specs]

        class Local:
            shape = (hi - lo, sum(len(i) for i in idx))
            dtype = np.dtype(np.float64)

        def loc_sw(dd, rows, cl):
            return orc.split_sandwich(lblocks, idx, dd, rows, cl)

        def loc_tmv(vv, rows, cl):
            return orc.split_transpose_matvec(lblocks, idx, vv, rows, cl)

        sep = RowShardedMatrix(Local(), local_sandwich=loc_sw, local_transpose_matvec=loc_tmv,
                               bounds=(lo, hi), n_global=n)
        fused = RowShardedMatrix(
            Local(), local_sandwich_and_transpose_matvec=lambda dd, vv, rows, cl: (loc_sw(dd, rows, cl),
                                                                                   loc_tmv(vv, rows, cl)),
            bounds=(lo, hi), n_global=n)

        calls = []
        real = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)

        dist.all_reduce = counting
        ok = True
        try:
            for rows, cl in [(None, None), (rows_g, None), (None, cols), (rows_g, cols)]:
                H_s = sep.sandwich_global(d, rows, cl)
                g_s = sep.transpose_matvec_global(v, rows, cl)
                before = len(calls)
                H, g = fused.sandwich_and_transpose_matvec_global(d, v, rows, cl)
                ok &= len(calls) - before == 1
                ok &= isinstance(H, np.ndarray) and isinstance(g, np.ndarray)
                ok &= H.shape == H_s.shape and g.shape == g_s.shape
                ok &= np.allclose(H, H_s, rtol=1e-12, atol=1e-12) and np.allclose(g, g_s, rtol=1e-12, atol=1e-12)
                # against the unsharded oracle as well
                ok &= np.allclose(H, orc.split_sandwich(blocks, idx, d, rows, cl), rtol=1e-12, atol=1e-12)
                ok &= np.allclose(g, orc.split_transpose_matvec(blocks, idx, v, rows, cl), rtol=1e-12, atol=1e-12)
            # the local-row form, with this shard's (possibly empty) bucket of the row list
            before = len(calls)
            H, g = fused.sandwich_and_transpose_matvec(d[lo:hi], v[lo:hi], bucket_rows(rows_g, lo, hi))
            ok &= len(calls) - before == 1
            ok &= np.allclose(H, orc.split_sandwich(blocks, idx, d, rows_g), rtol=1e-12, atol=1e-12)
            ok &= np.allclose(g, orc.split_transpose_matvec(blocks, idx, v, rows_g), rtol=1e-12, atol=1e-12)
        finally:
            dist.all_reduce = real
        q.put((rank, bool(ok), (lo, hi)))
    except Exception as e:                # reported, not left for the parent's queue timeout
        q.put((rank, False, repr(e)))
    finally:
        dist.destroy_process_group()


def _run(world, rows_mode):
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q, rows_mode)) for r in range(world)]
    for p in procs:
        p.start()
    res = [q.get(timeout=300) for _ in procs]
    for p in procs:
        p.join(timeout=60)
        assert p.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    return res


def test_fused_gloo_world2():
    _run(2, "spread")


def test_fused_gloo_world2_empty_row_lists():
    """n = 1001 rows over 2 ranks (uneven) and a row list that lies entirely in the first rank's shard: the other
    rank's partial is all zeros and still joins the one collective."""
    res = _run(2, "low")
    assert sorted(b[1] - b[0] for _, _, b in res) == [500, 501]


def test_fused_falls_back_to_injected_separate_products():
    """Only the separate products injected: the pair is made of them (world 1, no process group)."""
    from tabmat_amd.distributed import RowShardedMatrix

    class Local:
        shape = (3, 2)
        dtype = np.dtype(np.float64)

    sh = RowShardedMatrix(Local(), local_sandwich=lambda d, r, c: np.eye(2) * d.sum(),
                          local_transpose_matvec=lambda v, r, c: np.full(2, v.sum()))
    H, g = sh.sandwich_and_transpose_matvec(np.ones(3), np.arange(3.0))
    assert np.array_equal(H, 3 * np.eye(2)) and np.array_equal(g, [3.0, 3.0])
