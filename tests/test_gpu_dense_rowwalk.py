"""The dense row walk K8 (tm_dense_sandwich_matvec_*), K8d (tm_dense_sandwich_diag_*) and K9 (tm_dense_glm_loss_grad_*)
share (csrc/dense_rowwalk.hpp), through the tabmat_amd.ext.dense wrappers and with every optional input: each
(lanes per row, loads per lane) rung of the ladder, both load forms (odd widths read one element per load), fewer
rows than one wave step, a partial step, and several workgroups with a ragged tail.  Compared with long-double
numpy at the natural scales of test_gpu_sandwich_matvec / test_gpu_sandwich_diag / test_gpu_glm_loss_grad; K8's w
at dm = 1 and K9's eta are the same chain of operations and must agree bit for bit."""
import functools

import numpy as np
import pytest
import torch

from test_gpu_glm_loss_grad import TINY, _errors, _problem, _reference
from test_gpu_sandwich_matvec import LD, TOL, _host

pytestmark = pytest.mark.gpu

WIDTHS = (1, 3, 10, 17, 64, 127, 256, 512)
WIDEST = {np.float64: 1024, np.float32: 2048}
GRID = [(dt, w, n) for dt in (np.float64, np.float32) for w in WIDTHS + (WIDEST[dt],) for n in (1, 63, 5003)]
grid = pytest.mark.parametrize("dtype,width,n", GRID, ids=[f"{dt.__name__}-{w}-{n}" for dt, w, n in GRID])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(got, want, scale):
    got = np.asarray(_host(got), dtype=LD)
    return float((np.abs(got - want) / np.maximum(scale, TINY)).max())


@functools.lru_cache(maxsize=None)
def _case(dtype, width, n):
    """Inputs on the device and the long-double references of the three kernels, built once per grid point (the
    references keep vectors only)."""
    from tabmat_amd.ext import dense as xd
    from tabmat_amd.ext._types import DenseDev

    rng = np.random.default_rng(width * 11 + n)
    X = rng.standard_normal((n, width)).astype(dtype)
    c = (0.5 * rng.standard_normal(width)).astype(dtype)
    shift = np.asarray([0.3], dtype=dtype)
    Ac = X.astype(LD) - c.astype(LD)[None, :]                         # the centred block the kernels work on
    # poisson problem at the centred block: u, y, weights with zeros, and the offset that goes in as t_add
    u, y, wt, t_add = _problem(Ac.astype(np.float64), "poisson", dtype, "random", "given", width + 3 * n)
    dm = (rng.random(n) * rng.choice([-1.0, 1.0], n)).astype(dtype)
    off = t_add.astype(LD) + shift.astype(LD)[0]

    Aa, ul, dl = np.abs(Ac), u.astype(LD), dm.astype(LD)
    t = Ac @ ul + off
    t_s = Aa @ np.abs(ul) + np.abs(off)
    smv = dict(w=dl * t, w_s=np.abs(dl) * t_s, g=Ac.T @ (dl * t), g_s=Aa.T @ (np.abs(dl) * t_s))
    A2 = Ac * Ac
    diag = dict(out=dl @ A2, s=np.abs(dl) @ A2)
    glm = _reference(Ac, "poisson", u, y, wt, off)
    blk = DenseDev.from_tensor(_dev(X))
    assert xd.sandwich_matvec_supported(blk)
    dev = {k: _dev(v) for k, v in dict(u=u, y=y, wt=wt, t_add=t_add, dm=dm, center=c, shift=shift).items()}
    return dict(blk=blk, dev=dev, smv=smv, diag=diag, glm=glm)


@grid
def test_sandwich_matvec(dtype, width, n):
    from tabmat_amd.ext import dense as xd

    cse = _case(dtype, width, n)
    v, ref = cse["dev"], cse["smv"]
    g, w = xd.dense_sandwich_matvec(cse["blk"], v["u"], v["dm"], t_add=v["t_add"], center=v["center"],
                                    shift=v["shift"], want_w=True)
    assert _host(g).dtype == dtype and tuple(g.shape) == (width,) and tuple(w.shape) == (n,)
    errs = dict(g=_rel(g, ref["g"], ref["g_s"]), w=_rel(w, ref["w"], ref["w_s"]))
    print(f"K8 {dtype.__name__} width={width} n={n}: " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL[dtype], f"{k}: {e:.2e}"


@grid
def test_sandwich_diag(dtype, width, n):
    from tabmat_amd.ext import dense as xd

    cse = _case(dtype, width, n)
    v, ref = cse["dev"], cse["diag"]
    out = xd.dense_sandwich_diag(cse["blk"], v["dm"], center=v["center"])
    assert _host(out).dtype == dtype and tuple(out.shape) == (width,)
    err = _rel(out, ref["out"], ref["s"])
    print(f"K8d {dtype.__name__} width={width} n={n}: {err:.2e}")
    assert err <= TOL[dtype], f"{err:.2e}"


@grid
def test_glm_loss_grad(dtype, width, n):
    from tabmat_amd.ext import dense as xd

    cse = _case(dtype, width, n)
    v = cse["dev"]
    loss, g, eta, r, d = xd.dense_glm_loss_grad(cse["blk"], v["u"], xd.GLM_FAMILIES["poisson"], v["y"], v["wt"],
                                                t_add=v["t_add"], center=v["center"], shift=v["shift"])
    assert _host(g).dtype == dtype and tuple(g.shape) == (width,)
    assert all(tuple(x.shape) == (n,) for x in (eta, r, d)) and loss.dtype == torch.float64
    errs = _errors(cse["glm"], loss, g, eta, d, r)
    print(f"K9 {dtype.__name__} width={width} n={n}: " + " ".join(f"{k}={e:.2e}" for k, e in errs.items()))
    for k, e in errs.items():
        assert e <= TOL[dtype], f"{k}: {e:.2e}"


@grid
def test_matvec_w_is_glm_eta(dtype, width, n):
    """dm = 1: K8's w = 1 * t and K9's eta are both segment_allreduce(p) + shift + t_add[r] with the same fma chain
    for p -- bit for bit the same vector."""
    from tabmat_amd.ext import dense as xd

    cse = _case(dtype, width, n)
    v = cse["dev"]
    _, w = xd.dense_sandwich_matvec(cse["blk"], v["u"], torch.ones_like(v["dm"]), t_add=v["t_add"],
                                    center=v["center"], shift=v["shift"], want_w=True)
    eta = xd.dense_glm_loss_grad(cse["blk"], v["u"], xd.GLM_FAMILIES["poisson"], v["y"], v["wt"], t_add=v["t_add"],
                                 center=v["center"], shift=v["shift"])[2]
    assert torch.equal(w, eta)
