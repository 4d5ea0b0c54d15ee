"""sandwich_diag without a GPU: argument checks before any device work, the MatrixBase default composition, and
RowShardedMatrix.sandwich_diag / _global over gloo with oracle-injected local products (one all_reduce per call)."""
import os
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import _cases as cs
import tabmat_amd as tm
from test_sandwich_matvec_host import _Stub, _free_port, _mats, no_device  # noqa: F401  (no_device: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k", range(8))
def test_error_conventions_before_any_device_work(k, no_device):  # noqa: F811
    mat = _mats()[k]
    n, m = mat.shape
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError, match="not aligned"):
            mat.sandwich_diag(np.ones(bad))
    with pytest.raises(TypeError, match="same dtype"):
        mat.astype(np.float64).sandwich_diag(np.ones(n, dtype=np.float32))
    with pytest.raises(IndexError):
        mat.sandwich_diag(np.ones(n), rows=[n + 5])
    with pytest.raises(IndexError):
        mat.sandwich_diag(np.ones(n), cols=[m])
    with pytest.raises(IndexError):
        mat.sandwich_diag(np.ones(n), rows=[0], cols=[-m - 1])


def test_standardized_checks_before_any_device_work(no_device):  # noqa: F811
    std = tm.StandardizedMatrix(tm.DenseMatrix(np.ones((4, 3))), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="not aligned"):
        std.sandwich_diag(np.ones(5))
    with pytest.raises(TypeError, match="same dtype"):
        std.sandwich_diag(np.ones(4, dtype=np.float32))
    with pytest.raises(IndexError):
        std.sandwich_diag(np.ones(4), rows=[4])
    with pytest.raises(IndexError):
        std.sandwich_diag(np.ones(4), cols=[3])


class _ColStub(_Stub):
    """_Stub with the getcol the default sandwich_diag reads its columns through."""

    def getcol(self, i):
        self.calls.append("getcol")
        return _ColStub(self.A_[:, [i]])

    def toarray(self):
        return self.A_


def test_matrix_base_default_composes():
    """MatrixBase.sandwich_diag is concrete: getcol and transpose_matvec per column, no sandwich, no device."""
    rng = np.random.default_rng(0)
    A = rng.standard_normal((40, 7))
    S = _ColStub(A)
    d = rng.standard_normal(40)
    g = S.sandwich_diag(d)
    assert isinstance(g, np.ndarray) and g.shape == (7,) and g.dtype == np.float64
    assert S.calls == ["getcol", "transpose_matvec"] * 7
    np.testing.assert_allclose(g, (A * A).T @ d, rtol=1e-12)
    rows, cols = np.array([3, 5, 5, 20]), np.array([6, 1, 6])
    g = S.sandwich_diag(d, rows, cols)
    Ar = A[rows][:, cols]
    np.testing.assert_allclose(g, (Ar * Ar).T @ d[rows], rtol=1e-12)


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
        p = sum(len(i) for i in idx)
        rng = np.random.default_rng(0)
        d = rng.standard_normal(n)
        rows_g = np.sort(rng.choice(n, 600, replace=False))
        if rows_mode == "low":            # every selected row in the first shards: the others get an empty list
            rows_g = np.sort(rng.choice(3 * (n // 8), 200, replace=False))
        cols = np.sort(rng.choice(p, 17, replace=False))

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
            shape = (hi - lo, p)
            dtype = np.dtype(np.float64)

        def loc_diag(dd, rows, cl):
            if rows is not None and len(rows) == 0:
                return np.zeros(p if cl is None else len(cl))
            return np.ascontiguousarray(orc.split_sandwich(lblocks, idx, dd, rows, cl).diagonal())

        sh = RowShardedMatrix(Local(), local_sandwich_diag=loc_diag, bounds=(lo, hi), n_global=n)

        calls = []
        real = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)

        dist.all_reduce = counting
        ok = True
        try:
            for rows, cl in [(None, None), (rows_g, None), (None, cols), (rows_g, cols)]:
                before = len(calls)
                g = sh.sandwich_diag_global(d, rows, cl)
                ok &= len(calls) - before == 1
                ok &= isinstance(g, np.ndarray) and g.shape == ((p if cl is None else len(cl)),)
                want = orc.split_sandwich(blocks, idx, d, rows, cl).diagonal()
                ok &= np.allclose(g, want, rtol=1e-11, atol=1e-11)
            # the local-row form, with this shard's (possibly empty) bucket of the row list
            before = len(calls)
            g = sh.sandwich_diag(d[lo:hi], bucket_rows(rows_g, lo, hi))
            ok &= len(calls) - before == 1
            ok &= np.allclose(g, orc.split_sandwich(blocks, idx, d, rows_g).diagonal(), rtol=1e-11, atol=1e-11)
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
    for pr in procs:
        pr.start()
    res = [q.get(timeout=300) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    return res


def test_sharded_world2():
    res = _run(2, "spread")
    assert sorted(b[1] - b[0] for _, _, b in res) == [500, 501]


def test_sharded_world2_empty_row_lists():
    _run(2, "low")


def test_sharded_world8():
    _run(8, "spread")


def test_sharded_world8_empty_row_lists():
    _run(8, "low")


def test_sharded_default_uses_local_sandwich_diag():
    """No injection: the local matrix's own sandwich_diag is the local product (world 1, no process group)."""
    from tabmat_amd.distributed import RowShardedMatrix

    class Local:
        shape = (3, 2)
        dtype = np.dtype(np.float64)

        def sandwich_diag(self, d, rows, cols):
            return np.full(2, d.sum())

    g = RowShardedMatrix(Local()).sandwich_diag(np.ones(3))
    assert np.array_equal(g, [3.0, 3.0])
