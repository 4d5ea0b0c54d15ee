"""glm_loss_grad without a GPU: argument checks before any device work on every matrix class, and
RowShardedMatrix.glm_loss_grad / _global over gloo with a NumPy local product (ONE all_reduce of [grad, loss])."""
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import _cases as cs
import tabmat_amd as tm

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


def _check_errors(mat):
    n, m = mat.shape
    ok = dict(family="poisson", beta=np.ones(m), y=np.ones(n))
    for name in ("y", "weights", "offset"):
        for bad in (n - 1, n + 1):
            with pytest.raises(ValueError, match=name):
                mat.glm_loss_grad(**{**ok, name: np.ones(bad)})
        with pytest.raises(ValueError, match=name):
            mat.glm_loss_grad(**{**ok, name: np.ones((n, 1))})
    for bad in (m - 1, m + 1):
        with pytest.raises(ValueError, match="beta"):
            mat.glm_loss_grad(**{**ok, "beta": np.ones(bad)})
    with pytest.raises(NotImplementedError, match="glm_loss_grad is only implemented for 1d arrays."):
        mat.glm_loss_grad(**{**ok, "beta": np.ones((m, 2))})
    for fam in ("tweedie", "Poisson", None, 1):
        with pytest.raises(ValueError, match="family"):
            mat.glm_loss_grad(**{**ok, "family": fam})


@pytest.mark.parametrize("k", range(8))
def test_error_conventions_before_any_device_work(k, no_device):
    _check_errors(_mats()[k])


def test_standardized_checks_before_any_device_work(no_device):
    _check_errors(tm.StandardizedMatrix(tm.DenseMatrix(np.ones((4, 3))), np.zeros(3), np.ones(3)))


def test_family_codes_match_the_header():
    """The Python family table and the TM_GLM_* enum of include/tabmat_hip.h are one list."""
    import re

    from tabmat_amd import _lib
    from tabmat_amd.ext.dense import GLM_FAMILIES

    src = open(_lib.HEADER).read()
    codes = {m.group(1).lower(): int(m.group(2)) for m in re.finditer(r"TM_GLM_(\w+)\s*=\s*(\d+)", src)}
    assert codes == GLM_FAMILIES
    for sym in ("tm_dense_glm_loss_grad_f32", "tm_dense_glm_loss_grad_f64", "tm_glm_rowfn_f32", "tm_glm_rowfn_f64"):
        assert sym in _lib.prototypes()


def _np_glm(A, family, beta, y, w, off):
    """float64 NumPy (loss, grad, eta, d) of the issue's table."""
    n = A.shape[0]
    w = np.ones(n) if w is None else w
    eta = A @ beta + (0.0 if off is None else off)
    with np.errstate(divide="ignore", invalid="ignore"):
        ylogy = np.where(y > 0, y * np.log(np.where(y > 0, y, 1.0)), 0.0)
        if family == "gaussian":
            l, r, h = (y - eta) ** 2 / 2, eta - y, np.ones(n)
        elif family == "poisson":
            mu = np.exp(eta)
            l, r, h = ylogy - y * eta - (y - mu), mu - y, mu
        elif family == "binomial":
            mu = 1 / (1 + np.exp(-eta))
            z = 1 - y
            zlogz = np.where(z > 0, z * np.log(np.where(z > 0, z, 1.0)), 0.0)
            l = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta))) - y * eta + ylogy + zlogz
            r, h = mu - y, mu * (1 - mu)
        else:
            em = np.exp(-eta)
            l, r, h = y * em - 1 - np.log(y) + eta, 1 - y * em, np.ones(n)
    return float((w * l).sum()), A.T @ (w * r), eta, w * h


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tabmat_amd.distributed import RowShardedMatrix, shard_bounds

        n, p = 1001, 13
        rng = np.random.default_rng(0)
        A = rng.standard_normal((n, p))
        beta = 0.1 * rng.standard_normal(p)
        w = rng.random(n)
        w[::7] = 0.0
        off = 0.1 * rng.standard_normal(n)
        lo, hi = shard_bounds(n, world, rank)

        class Local:
            shape = (hi - lo, p)
            dtype = np.dtype(np.float64)

        def loc(family, b, y, weights, offset):
            return _np_glm(A[lo:hi], family, b, y, weights, offset)

        sh = RowShardedMatrix(Local(), local_glm_loss_grad=loc, bounds=(lo, hi), n_global=n)
        calls = []
        real = dist.all_reduce

        def counting(t, *a, **k):
            calls.append(tuple(t.shape))
            return real(t, *a, **k)

        dist.all_reduce = counting
        ok = True
        try:
            for family in ("gaussian", "poisson", "binomial", "gamma"):
                eta_t = A @ beta + off
                y = {"gaussian": eta_t + 1.0, "poisson": np.floor(np.exp(eta_t) + 0.5),
                     "binomial": (eta_t > 0).astype(np.float64), "gamma": np.exp(eta_t) + 0.5}[family]
                for ww, oo in ((None, None), (w, off)):
                    want = _np_glm(A, family, beta, y, ww, oo)
                    before = len(calls)
                    loss, g, eta, d = sh.glm_loss_grad_global(family, beta, y, ww, oo)
                    ok &= len(calls) - before == 1 and calls[-1] == (p + 1,)     # ONE collective: [grad, loss]
                    ok &= isinstance(loss, float) and isinstance(g, np.ndarray) and g.shape == (p,)
                    ok &= bool(np.isclose(loss, want[0], rtol=1e-12, atol=1e-12))
                    ok &= bool(np.allclose(g, want[1], rtol=1e-11, atol=1e-11))
                    # eta and d stay local
                    ok &= eta.shape == (hi - lo,) and bool(np.allclose(eta, want[2][lo:hi], rtol=1e-13, atol=1e-13))
                    ok &= d.shape == (hi - lo,) and bool(np.allclose(d, want[3][lo:hi], rtol=1e-12, atol=1e-13))
            # the local-slice form
            y = np.floor(np.exp(A @ beta) + 0.5)
            before = len(calls)
            loss, g, _, _ = sh.glm_loss_grad("poisson", beta, y[lo:hi], w[lo:hi])
            ok &= len(calls) - before == 1
            want = _np_glm(A, "poisson", beta, y, w, None)
            ok &= bool(np.isclose(loss, want[0], rtol=1e-12)) and bool(np.allclose(g, want[1], rtol=1e-11, atol=1e-11))
        finally:
            dist.all_reduce = real
        q.put((rank, bool(ok), (lo, hi)))
    except Exception as e:                # reported, not left for the parent's queue timeout
        q.put((rank, False, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_world2_one_all_reduce():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=300) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    assert sorted(b[1] - b[0] for _, _, b in res) == [500, 501]


def test_sharded_default_uses_local_glm_loss_grad():
    """No injection: the local matrix's own glm_loss_grad is the local product (world 1, no process group)."""
    from tabmat_amd.distributed import RowShardedMatrix

    class Local:
        shape = (3, 2)
        dtype = np.dtype(np.float64)

        def glm_loss_grad(self, family, beta, y, weights, offset):
            return 1.5, np.full(2, y.sum()), y * 2, y * 3

    loss, g, eta, d = RowShardedMatrix(Local()).glm_loss_grad("poisson", np.zeros(2), np.ones(3))
    assert loss == 1.5 and np.array_equal(g, [3.0, 3.0]) and np.array_equal(eta, [2.0] * 3)
