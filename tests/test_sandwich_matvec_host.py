"""sandwich_matvec without a GPU: argument checks before any device work, the MatrixBase default composition, and
RowShardedMatrix.sandwich_matvec / _global over gloo with oracle-injected local products (one all_reduce per call)."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import _cases as cs
import tabmat_amd as tm
from tabmat_amd.matrix_base import MatrixBase

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _mats():
    specs, idx = cs.complex_split_specs()
    from _gpu_util import to_tm_block, to_tm_split

    return [to_tm_block(s) for _, s in cs.unscaled_specs()] + [to_tm_split(specs, idx)]


@pytest.fixture
def no_device(monkeypatch):
    """Any device work raises: the checks must come first."""
    from tabmat_amd import _device as D

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(D, "require_gpu", boom)


@pytest.mark.parametrize("k", range(8))
def test_error_conventions_before_any_device_work(k, no_device):
    mat = _mats()[k]
    n, m = mat.shape
    for bad in (n - 1, n + 1):
        with pytest.raises(ValueError, match="not aligned"):
            mat.sandwich_matvec(np.ones(bad), np.ones(m))
    for bad in (m - 1, m + 1):
        with pytest.raises(ValueError):
            mat.sandwich_matvec(np.ones(n), np.ones(bad))
    with pytest.raises(ValueError):
        mat.sandwich_matvec(np.ones(n), np.ones(m), cols=[0])           # u must have len(cols)
    with pytest.raises(NotImplementedError, match="only implemented for 1d arrays"):
        mat.sandwich_matvec(np.ones(n), np.ones((m, 2)))
    with pytest.raises(TypeError, match="same dtype"):
        mat.astype(np.float64).sandwich_matvec(np.ones(n, dtype=np.float32), np.ones(m))
    with pytest.raises(IndexError):
        mat.sandwich_matvec(np.ones(n), np.ones(m), rows=[n + 5])


def test_standardized_checks_before_any_device_work(no_device):
    std = tm.StandardizedMatrix(tm.DenseMatrix(np.ones((4, 3))), np.zeros(3), np.ones(3))
    with pytest.raises(ValueError, match="not aligned"):
        std.sandwich_matvec(np.ones(5), np.ones(3))
    with pytest.raises(NotImplementedError, match="only implemented for 1d arrays"):
        std.sandwich_matvec(np.ones(4), np.ones((3, 1)))
    with pytest.raises(ValueError):
        std.sandwich_matvec(np.ones(4), np.ones(2))


class _Stub(MatrixBase):
    """A MatrixBase subclass with host-only products: the default sandwich_matvec composes them."""

    def __init__(self, A):
        self.A_ = np.asarray(A, dtype=np.float64)
        self.shape = self.A_.shape
        self.dtype = self.A_.dtype
        self.calls = []

    def matvec(self, v, cols=None, out=None):
        self.calls.append("matvec")
        v = np.asarray(v)
        A = self.A_ if cols is None else self.A_[:, cols]
        return A @ (v if cols is None else v[cols])

    def transpose_matvec(self, v, rows=None, cols=None, out=None):
        self.calls.append("transpose_matvec")
        v = np.asarray(v)
        r = np.arange(self.shape[0]) if rows is None else np.asarray(rows)
        A = self.A_[r] if cols is None else self.A_[r][:, cols]
        return A.T @ v[r]

    def sandwich(self, d, rows=None, cols=None):
        raise AssertionError("the default sandwich_matvec must not form the sandwich")

    getcol = toarray = astype = __getitem__ = _get_col_stds = None


def test_matrix_base_default_composes(monkeypatch):
    """MatrixBase.sandwich_matvec is concrete: matvec then transpose_matvec, nothing else."""
    from tabmat_amd import _device as D
    from tabmat_amd import matrix_base as mb

    # host-only stand-ins for the device helpers the default uses
    monkeypatch.setattr(mb._SmvArgs, "u_full", lambda self, tdt: _u_full_host(self))
    monkeypatch.setattr(mb._SmvArgs, "finish", lambda self, g: np.asarray(g).astype(self.out_dtype))
    monkeypatch.setattr(D, "to_dev", lambda x, dtype=None: np.asarray(x))
    rng = np.random.default_rng(0)
    A = rng.standard_normal((40, 7))
    S = _Stub(A)
    d, u = rng.random(40), rng.standard_normal(7)
    g = S.sandwich_matvec(d, u)
    assert S.calls == ["matvec", "transpose_matvec"]
    np.testing.assert_allclose(g, A.T @ (d * (A @ u)), rtol=1e-12)
    rows, cols = np.array([3, 5, 5, 20]), np.array([6, 1])
    g = S.sandwich_matvec(d, u[:2], rows, cols)
    Ar = A[rows][:, cols]
    np.testing.assert_allclose(g, Ar.T @ (d[rows] * (Ar @ u[:2])), rtol=1e-12)
    assert S.calls == ["matvec", "transpose_matvec"] * 2


def _u_full_host(a):
    if a.cols is None:
        return np.asarray(a.u, dtype=np.float64)
    full = np.zeros(a.p)
    np.add.at(full, a.cols, a.u)
    return full


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
        p = sum(len(i) for i in idx)
        rng = np.random.default_rng(0)
        d = rng.random(n)
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

        def loc_smv(dd, uu, rows, cl):
            if rows is not None and len(rows) == 0:
                return np.zeros(len(uu))
            return orc.split_sandwich(lblocks, idx, dd, rows, cl) @ uu

        sh = RowShardedMatrix(Local(), local_sandwich_matvec=loc_smv, bounds=(lo, hi), n_global=n)

        calls = []
        real = dist.all_reduce

        def counting(*a, **k):
            calls.append(1)
            return real(*a, **k)

        dist.all_reduce = counting
        ok = True
        try:
            for rows, cl in [(None, None), (rows_g, None), (None, cols), (rows_g, cols)]:
                u = np.random.default_rng(1).standard_normal(p if cl is None else len(cl))
                before = len(calls)
                g = sh.sandwich_matvec_global(d, u, rows, cl)
                ok &= len(calls) - before == 1
                ok &= isinstance(g, np.ndarray) and g.shape == u.shape
                want = orc.split_sandwich(blocks, idx, d, rows, cl) @ u
                ok &= np.allclose(g, want, rtol=1e-11, atol=1e-11)
            # the local-row form, with this shard's (possibly empty) bucket of the row list
            u = np.random.default_rng(2).standard_normal(p)
            before = len(calls)
            g = sh.sandwich_matvec(d[lo:hi], u, bucket_rows(rows_g, lo, hi))
            ok &= len(calls) - before == 1
            ok &= np.allclose(g, orc.split_sandwich(blocks, idx, d, rows_g) @ u, rtol=1e-11, atol=1e-11)
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


def test_sharded_default_uses_local_sandwich_matvec():
    """No injection: the local matrix's own sandwich_matvec is the local product (world 1, no process group)."""
    from tabmat_amd.distributed import RowShardedMatrix

    class Local:
        shape = (3, 2)
        dtype = np.dtype(np.float64)

        def sandwich_matvec(self, d, u, rows, cols):
            return np.full(2, d.sum() * u.sum())

    g = RowShardedMatrix(Local()).sandwich_matvec(np.ones(3), np.array([1.0, 2.0]))
    assert np.array_equal(g, [9.0, 9.0])
