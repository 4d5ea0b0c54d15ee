"""glm_loss_grad: loss, gradient, eta and Hessian weights of a GLM from one call.  Compared with long-double numpy from
toarray() at the natural scales
    t_s = |A| |beta| + |offset|                       (eta)
    r_s = w (|y| + mu (1 + t_s))                      (r and a non-constant d; gaussian: w (|y| + t_s);
                                                       gamma: |y| -> 1 and mu -> y / mu)
    (|A|' r_s)_j                                      (grad_j)
    sum |w l| + sum r_s t_s                           (loss)
at the tolerances of test_gpu_sandwich_matvec.py; the ABI spy proves which kernel ran (tm_dense_glm_loss_grad_* in one
pass over the dense block, tm_glm_rowfn_* where no dense block takes it)."""
import zlib

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import _cases as cs
from _gpu_util import to_tm_block, to_tm_split

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = {np.float64: 1e-12, np.float32: 1e-4}
FAMILIES = ["gaussian", "poisson", "binomial", "gamma"]
TINY = np.finfo(np.float64).tiny


def _spy():
    from conftest import ABI_CALLS

    return dict(ABI_CALLS)


def _called(before, after, name):
    return after.get(name, 0) > before.get(name, 0)


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _dense(M):
    A = M.toarray()
    return A.toarray() if sps.issparse(A) else np.asarray(A)


def _xlogx(v):
    pos = v > 0
    return np.where(pos, v * np.log(np.where(pos, v, LD(1))), LD(0))


def _reference(A, family, beta, y, w, off):
    """Long-double (loss, grad, eta, r, d) and the natural scales of their errors."""
    A = np.asarray(A, dtype=LD)
    beta = np.asarray(beta, dtype=LD)
    y = np.asarray(y, dtype=LD)
    n = A.shape[0]
    w = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=LD)
    off = np.zeros(n, dtype=LD) if off is None else np.asarray(off, dtype=LD)
    eta = A @ beta + off
    t_s = np.abs(A) @ np.abs(beta) + np.abs(off)
    if family == "gaussian":
        mu = eta
        l, r, h = (y - mu) ** 2 / 2, mu - y, np.ones(n, dtype=LD)
        r_s = w * (np.abs(y) + t_s)
    elif family == "poisson":
        mu = np.exp(eta)
        l, r, h = _xlogx(y) - y * eta - (y - mu), mu - y, mu
        r_s = w * (np.abs(y) + mu * (1 + t_s))
    elif family == "binomial":
        mu = 1 / (1 + np.exp(-eta))
        sp = np.maximum(eta, 0) + np.log1p(np.exp(-np.abs(eta)))
        l, r, h = sp - y * eta + _xlogx(y) + _xlogx(1 - y), mu - y, mu * (1 - mu)
        r_s = w * (np.abs(y) + mu * (1 + t_s))
    else:
        em = np.exp(-eta)
        l, r, h = y * em - 1 - np.log(y) + eta, 1 - y * em, np.ones(n, dtype=LD)
        r_s = w * (1 + y * em * (1 + t_s))
    return dict(loss=(w * l).sum(), grad=A.T @ (w * r), eta=eta, r=w * r, d=w * h, t_s=t_s, r_s=r_s,
                g_s=np.abs(A).T @ r_s, l_s=np.abs(w * l).sum() + (r_s * t_s).sum(), const_d=family in ("gaussian", "gamma"),
                w=w)


def _errors(ref, loss, grad, eta, d, r=None):
    """The four (five with r) errors at their natural scales; a constant d (gaussian, gamma: d = w) must be exact."""
    def rel(got, want, scale):
        got = np.asarray(_host(got), dtype=LD)
        return float((np.abs(got - want) / np.maximum(scale, TINY)).max()) if got.size else 0.0

    out = dict(eta=rel(eta, ref["eta"], ref["t_s"]), grad=rel(grad, ref["grad"], ref["g_s"]),
               loss=float(abs(LD(float(loss)) - ref["loss"]) / max(ref["l_s"], TINY)))
    dh = _host(d)
    if ref["const_d"]:
        out["d"] = 0.0 if np.array_equal(dh, np.asarray(ref["w"]).astype(dh.dtype)) else np.inf
    else:
        out["d"] = rel(d, ref["d"], ref["r_s"])
    if r is not None:
        out["r"] = rel(r, ref["r"], ref["r_s"])
    return out


def _draw_y(rng, family, eta):
    if family == "gaussian":
        return eta + rng.standard_normal(eta.shape[0])
    if family == "poisson":
        return rng.poisson(np.exp(eta)).astype(np.float64)
    if family == "binomial":
        y = (rng.random(eta.shape[0]) < 1 / (1 + np.exp(-eta))).astype(np.float64)
        k = min(50, y.shape[0])
        y[rng.choice(y.shape[0], k, replace=False)] = rng.random(k)      # fractional responses
        return y
    return rng.gamma(2.0, np.exp(eta) / 2.0) + 1e-3


def _problem(A, family, dtype, wkind, okind, seed):
    """(beta, y, weights or None, offset or None) in `dtype`: beta ~ 0.3 N(0, 1) / sqrt(p), y drawn from the family
    at the true eta, weights random with 10 % zeros."""
    rng = np.random.default_rng(seed)
    n, p = A.shape
    beta = (0.3 * rng.standard_normal(p) / np.sqrt(max(p, 1))).astype(dtype)
    off = (0.2 * rng.standard_normal(n)).astype(dtype) if okind == "given" else None
    eta = np.asarray(A, dtype=np.float64) @ beta.astype(np.float64) + (0.0 if off is None else off.astype(np.float64))
    y = _draw_y(rng, family, eta).astype(dtype)
    w = None
    if wkind == "random":
        w = (rng.random(n) + 0.1).astype(dtype)
        w[rng.random(n) < 0.1] = 0
    return beta, y, w, off


def _dev(x):
    return None if x is None else torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _class_cases():
    rng = np.random.default_rng(7)
    n = 3000
    X = rng.standard_normal((n, 40))
    codes = rng.integers(0, 25, n).astype(np.int32)
    codes_m = codes.copy()
    codes_m[rng.random(n) < 0.1] = -1
    S = sps.random(n, 30, density=0.1, format="csc", random_state=rng)
    mixed = cs.mixed_specs(n, 96, 64, (20, 7, 3), seed=11)
    return {
        "dense_C": lambda dt: to_tm_block(("dense", np.ascontiguousarray(X)), dt),
        "dense_F": lambda dt: to_tm_block(("dense", np.asfortranarray(X)), dt),
        "sparse": lambda dt: to_tm_block(("sparse", S), dt),
        "cat_drop_first": lambda dt: to_tm_block(("cat", codes, 25, True), dt),
        "cat_missing_zero": lambda dt: to_tm_block(("cat", codes_m, 25, False), dt),
        "split_mixed": lambda dt: to_tm_split(*mixed, dtype=dt),
        "split_complex": lambda dt: to_tm_split(*cs.complex_split_specs(), dtype=dt),
    }


CASES = _class_cases()
_BUILT = {}
_REFS = {}


def _mat(name, dtype):
    key = (name, dtype)
    if key not in _BUILT:
        M = CASES[name](dtype)
        _BUILT[key] = (M, _dense(M))
    return _BUILT[key]


def _setup(name, dtype, family, wkind, okind):
    """The matrix, its dense form, the problem and its long-double reference: built once, shared by both sides."""
    key = (name, dtype, family, wkind, okind)
    if key not in _REFS:
        M, A = _mat(name, dtype)
        args = _problem(A, family, dtype, wkind, okind, zlib.crc32("/".join(map(str, key)).encode()))
        _REFS[key] = (args, _reference(A, family, *args))
    return _mat(name, dtype) + _REFS[key]


@pytest.mark.parametrize("side", ["numpy", "device"])
@pytest.mark.parametrize("okind", ["none", "given"])
@pytest.mark.parametrize("wkind", ["none", "random"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", FAMILIES)
def test_parity(family, dtype, name, wkind, okind, side):
    M, A, (beta, y, w, off), ref = _setup(name, dtype, family, wkind, okind)
    n, p = M.shape
    if side == "device":
        loss, grad, eta, d = M.glm_loss_grad(family, _dev(beta), _dev(y), _dev(w), _dev(off))
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (loss, grad, eta, d))
        assert loss.ndim == 0 and loss.dtype == torch.float64
    else:
        loss, grad, eta, d = M.glm_loss_grad(family, beta, y, w, off)
        assert isinstance(loss, float) and all(isinstance(x, np.ndarray) for x in (grad, eta, d))
    assert tuple(grad.shape) == (p,) and tuple(eta.shape) == (n,) and tuple(d.shape) == (n,)
    for x in (grad, eta, d):
        assert _host(x).dtype == dtype
    errs = _errors(ref, loss, grad, eta, d)
    print(f"{family} {dtype.__name__} {name} w={wkind} off={okind} {side}: "
          + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL[dtype], f"{k}: {v:.2e}"
    # d is ready for the Hessian-vector product
    s = np.random.default_rng(p).standard_normal(p).astype(dtype)
    hv = M.sandwich_matvec(d, _dev(s) if side == "device" else s)
    Al, sl = np.asarray(A, dtype=LD), s.astype(LD)
    want = Al.T @ (ref["d"] * (Al @ sl))
    scale = np.abs(Al).T @ (np.abs(ref["d"]) * (np.abs(Al) @ np.abs(sl)))
    err = float((np.abs(np.asarray(_host(hv), dtype=LD) - want) / np.maximum(scale, TINY)).max())
    assert err <= 10 * TOL[dtype], f"sandwich_matvec(d, s): {err:.2e}"


@pytest.mark.parametrize("n", [1, 63, 5003])
@pytest.mark.parametrize("width", [1, 3, 10, 17, 64, 127, 256, 513, 1024])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_kernel_layouts(dtype, width, n):
    """Every lane layout of K9 (8 .. 64 lanes per row, 1 .. 8 loads per lane, aligned or not) at one partial wave
    step, fewer rows than a step and several workgroups with a ragged tail.  513 columns are rows off the 16-byte
    grid and more than the 512 the one-element form takes: the one width of the list that runs matvec,
    tm_glm_rowfn_* and transpose_matvec."""
    import tabmat_amd as tm

    rng = np.random.default_rng(width * 7 + n)
    X = rng.standard_normal((n, width)).astype(dtype)
    beta, y, w, off = _problem(X, "poisson", dtype, "random", "given", width + n)
    suf = "f64" if dtype == np.float64 else "f32"
    before = _spy()
    loss, grad, eta, d = tm.DenseMatrix(X).glm_loss_grad("poisson", beta, y, w, off)
    after = _spy()
    assert _called(before, after, f"tm_dense_glm_loss_grad_{suf}") == (width != 513)
    assert _called(before, after, f"tm_glm_rowfn_{suf}") == (width == 513)
    errs = _errors(_reference(X, "poisson", beta, y, w, off), loss, grad, eta, d)
    print(f"{dtype.__name__} width={width} n={n}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL[dtype], f"{k}: {v:.2e}"


def _path_mats(dtype):
    import tabmat_amd as tm

    rng = np.random.default_rng(12)
    n = 4000
    X = rng.standard_normal((n, 24)).astype(dtype)
    specs, idx = cs.mixed_specs(20_000, 128, 64, (30, 5), seed=3)
    fused = {"dense": tm.DenseMatrix(np.ascontiguousarray(X)), "dense_F_twin": tm.DenseMatrix(np.asfortranarray(X)),
             "mixed": to_tm_split(specs, idx, dtype=dtype)}
    rowfn = {"sparse_only": tm.SparseMatrix(sps.random(n, 20, density=0.1, format="csc", random_state=rng).astype(dtype)),
             "cat_only": tm.CategoricalMatrix(rng.integers(0, 12, n), dtype=dtype)}
    if dtype == np.float64:
        rowfn["dense_1100"] = tm.DenseMatrix(rng.standard_normal((600, 1100)))
    return fused, rowfn


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_path_taken(dtype):
    suf = "f64" if dtype == np.float64 else "f32"
    fused, rowfn = _path_mats(dtype)
    for name, M in fused.items():
        A = _dense(M)
        beta, y, w, off = _problem(A, "poisson", dtype, "random", "given", 5)
        before = _spy()
        res = M.glm_loss_grad("poisson", beta, y, w, off)
        after = _spy()
        assert _called(before, after, f"tm_dense_glm_loss_grad_{suf}"), name
        # the dense block is read once: no separate matvec / transpose_matvec over it, no second row function
        for sym in (f"tm_dense_matvec_{suf}", f"tm_dense_rmatvec_{suf}", f"tm_glm_rowfn_{suf}"):
            assert not _called(before, after, sym), (name, sym)
        for k, v in _errors(_reference(A, "poisson", beta, y, w, off), *res).items():
            assert v <= TOL[dtype], f"{name} {k}: {v:.2e}"
    for name, M in rowfn.items():
        A = _dense(M)
        beta, y, w, off = _problem(A, "poisson", dtype, "random", "given", 6)
        before = _spy()
        res = M.glm_loss_grad("poisson", beta, y, w, off)
        after = _spy()
        assert _called(before, after, f"tm_glm_rowfn_{suf}"), name
        assert not _called(before, after, f"tm_dense_glm_loss_grad_{suf}"), name
        for k, v in _errors(_reference(A, "poisson", beta, y, w, off), *res).items():
            assert v <= TOL[dtype], f"{name} {k}: {v:.2e}"


@pytest.mark.parametrize("kind", ["dense", "sparse"])
@pytest.mark.parametrize("family", ["poisson", "gamma"])
def test_zero_weights_mask_overflowing_rows(family, kind):
    """Rows whose eta overflows exp carry weight 0: they contribute exactly nothing (the zero is selected, 0 * inf
    would be NaN), through the public call and in r of both kernels."""
    import tabmat_amd as tm
    from tabmat_amd.ext import dense as xd

    rng = np.random.default_rng(31)
    n = 2500
    if kind == "dense":
        A = rng.standard_normal((n, 33))
        M = tm.DenseMatrix(A)
    else:
        S = sps.random(n, 33, density=0.2, format="csc", random_state=rng)
        A, M = S.toarray(), tm.SparseMatrix(S)
    beta, y, w, off = _problem(A, family, np.float64, "random", "given", 8)
    bad = rng.choice(n, 200, replace=False)
    off[bad] = 800.0
    w[bad] = 0.0
    w[(bad[:5] + 1) % n] = 0.0                    # zero weights on ordinary rows too
    loss, grad, eta, d = M.glm_loss_grad(family, beta, y, w, off)
    assert np.isfinite(loss) and np.isfinite(grad).all() and np.isfinite(d).all()
    assert np.array_equal(d[w == 0], np.zeros(int((w == 0).sum())))
    keep = w != 0
    ref = _reference(A[keep], family, beta, y[keep], w[keep], off[keep])
    errs = _errors(ref, loss, grad, eta[keep], d[keep])
    for k, v in errs.items():
        assert v <= 1e-12, f"{k}: {v:.2e}"
    assert np.array_equal(eta[bad] > 700.0, np.ones(len(bad), dtype=bool))       # eta is still written
    # r is not part of the public result: ask the kernels
    fam = xd.GLM_FAMILIES[family]
    if kind == "dense":
        r = xd.dense_glm_loss_grad(M._smv_block(), _dev(beta), fam, _dev(y), _dev(w), t_add=_dev(off))[3]
    else:
        r = xd.glm_rowfn(fam, _dev(eta), _dev(y), _dev(w))[1]
    r = _host(r)
    assert np.array_equal(r[w == 0], np.zeros(int((w == 0).sum()))) and np.isfinite(r).all()
    assert float((np.abs(r[keep].astype(LD) - ref["r"]) / np.maximum(ref["r_s"], TINY)).max()) <= 1e-12


def test_dense_reproducible():
    import tabmat_amd as tm

    rng = np.random.default_rng(5)
    n = 200_000
    X = rng.standard_normal((n, 128))
    M = tm.DenseMatrix(X)
    beta, y, w, off = (_dev(v) for v in _problem(X, "poisson", np.float64, "random", "given", 3))
    a = M.glm_loss_grad("poisson", beta, y, w, off)
    b = M.glm_loss_grad("poisson", beta, y, w, off)
    for x, z in zip(a[1:], b[1:]):
        assert torch.equal(x, z)
    assert float(a[0]) == float(b[0])


def test_rowfn_reproducible_and_unaligned():
    """The streaming kernel alone: a fixed-order loss, and vectors that start off a 16-byte boundary (its
    one-element form) -- what a row part's slice of y / weights looks like."""
    from tabmat_amd.ext import dense as xd

    rng = np.random.default_rng(6)
    n = 300_001
    for dtype in (np.float64, np.float32):
        eta = (0.5 * rng.standard_normal(n + 1)).astype(dtype)
        y = rng.poisson(np.exp(eta.astype(np.float64))).astype(dtype)
        w = rng.random(n + 1).astype(dtype)
        a = xd.glm_rowfn(1, _dev(eta), _dev(y), _dev(w))
        b = xd.glm_rowfn(1, _dev(eta), _dev(y), _dev(w))
        assert float(a[0]) == float(b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2])
        loss, r, d = xd.glm_rowfn(1, *(_dev(v)[1:] for v in (eta, y, w)))       # element 1 on: not 16-byte aligned
        # (eta as the offset of a matrix without columns: t_s = |eta|)
        ref = _reference(np.zeros((n, 0)), "poisson", np.zeros(0), y[1:], w[1:], eta[1:])
        for k, v in _errors(ref, loss, np.zeros(0), eta[1:], d, r).items():
            assert v <= TOL[dtype], f"{dtype.__name__} {k}: {v:.2e}"


def _std_split(rng, n):
    import tabmat_amd as tm

    stds = np.array([(1.0, 5.0, 0.02, 300.0)[(j // 4) % 4] for j in range(48)])
    means = np.array([(0.0, 10.0, 400.0, 1e4)[j % 4] for j in range(48)]) * stds
    means[1::8] *= -1.0
    Xd = means[None, :] + stds[None, :] * rng.standard_normal((n, 48))
    Xs = sps.random(n, 16, density=0.05, format="csc", random_state=rng)
    c1 = rng.integers(0, 20, n)
    c2 = rng.integers(0, 7, n)
    mat = tm.SplitMatrix([tm.DenseMatrix(Xd), tm.SparseMatrix(Xs), tm.CategoricalMatrix(c1),
                          tm.CategoricalMatrix(c2, drop_first=True)])
    w = rng.random(n)
    w /= w.sum()
    return mat.standardize(w, True, True)[0]


_STD = {}


def _std():
    if not _STD:
        std = _std_split(np.random.default_rng(50), 20_000)
        X = std.mat.toarray().astype(LD)
        _STD["v"] = (std, X * std.mult.astype(LD)[None, :] + std.shift.astype(LD)[None, :])
    return _STD["v"]


@pytest.mark.parametrize("family", FAMILIES)
def test_standardized(family):
    std, Z = _std()
    beta, y, w, off = _problem(np.asarray(Z, dtype=np.float64), family, np.float64, "random", "given", 77)
    ref = _reference(Z, family, beta, y, w, off)
    before = _spy()
    res = std.glm_loss_grad(family, beta, y, w, off)
    assert _called(before, _spy(), "tm_dense_glm_loss_grad_f64")
    errs = _errors(ref, *res)
    print(f"standardized {family}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= 1e-10, f"{k}: {v:.2e}"
    resd = std.glm_loss_grad(family, _dev(beta), _dev(y), _dev(w), _dev(off))
    for k, v in _errors(ref, *resd).items():
        assert v <= 1e-10, f"device {k}: {v:.2e}"


@pytest.mark.parametrize("family", FAMILIES)
def test_row_parts(monkeypatch, family):
    import tabmat_amd.sparse_matrix as spm

    monkeypatch.setattr(spm, "PART_NNZ", 30_000)
    specs, idx = cs.mixed_specs(12_000, 48, 160, (40, 700), seed=21)      # ~96k nonzeros: 4+ parts
    X = to_tm_split(specs, idx)
    assert X._parts() is not None and len(X._parts()) >= 4
    A = _dense(X)
    beta, y, w, off = _problem(A, family, np.float64, "random", "given", 9)
    before = _spy()
    res = X.glm_loss_grad(family, beta, y, w, off)
    assert _called(before, _spy(), "tm_glm_rowfn_f64")
    for k, v in _errors(_reference(A, family, beta, y, w, off), *res).items():
        assert v <= TOL[np.float64], f"{k}: {v:.2e}"
