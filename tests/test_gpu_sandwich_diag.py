"""sandwich_diag: dg[q] = sum_{i in rows} d_i a_{i, cols[q]}^2, the diagonal of sandwich(d, rows, cols), without forming it.
Compared with long-double numpy at the natural scale s_q = sum_i |d_i| a_iq^2 (an entry with s_q = 0 must be exactly
0) and with sandwich(d, rows, cols).diagonal(); the ABI spy proves that the one-pass kernels
(tm_dense_sandwich_diag_*, tm_csr_sandwich_diag_*) run."""
import os
import sys
import zlib

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import _cases as cs
from _gpu_util import to_tm_split
from test_gpu_sandwich_matvec import DET, LD, TOL, _called, _class_cases, _cols, _host, _rows, _spy
from test_gpu_standardized_centered import _dense_cols, _standardized_ld

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

CASES = _class_cases()
_BUILT = {}


def _mat(name, dtype):
    key = (name, dtype)
    if key not in _BUILT:
        _BUILT[key] = CASES[name](dtype)
    return _BUILT[key]


def _dense_of(M):
    A = M.toarray()
    return A.toarray() if sps.issparse(A) else np.asarray(A)


def _ref(A, d, rows, cols):
    """(long-double diagonal, natural scale s) of A[rows][:, cols]' diag(d[rows]) A[rows][:, cols]."""
    A = np.asarray(A, dtype=LD)
    d = np.asarray(d, dtype=LD)
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64)
        A, d = A[r], d[r]
    if cols is not None:
        A = A[:, np.asarray(cols, dtype=np.int64)]
    A2 = A * A
    return d @ A2, np.abs(d) @ A2


def _err(got, ref, s, what=""):
    """Largest error at the natural scale; entries of scale 0 must be exactly 0."""
    got = np.asarray(_host(got), dtype=LD)
    if got.size == 0:
        return 0.0
    zero = s == 0
    assert np.all(got[zero] == 0), f"{what}: an entry of natural scale 0 is not exactly 0"
    if zero.all():
        return 0.0
    return float((np.abs(got - ref)[~zero] / s[~zero]).max())


def _weights(rng, n, dtype, signed):
    d = rng.random(n)
    if signed:
        d = d * rng.choice([-1.0, 1.0], n)
    return d.astype(dtype)


@pytest.mark.parametrize("side", ["numpy", "device"])
@pytest.mark.parametrize("cols_kind", ["none", "subset", "empty"])
@pytest.mark.parametrize("rows_kind", ["none", "sorted", "repeats", "empty"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_parity(name, dtype, rows_kind, cols_kind, side):
    M = _mat(name, dtype)
    n, p = M.shape
    seed = zlib.crc32(f"{name}/{rows_kind}/{cols_kind}".encode())
    rng = np.random.default_rng(seed)
    A = _dense_of(M)
    rows = _rows(rows_kind, n, rng)
    cols = _cols(cols_kind, p, rng)
    k = p if cols is None else len(cols)
    d = _weights(rng, n, dtype, signed=bool(seed & 1) ^ (side == "device"))     # mixed signs in half of the cases
    if side == "device":
        g = M.sandwich_diag(torch.from_numpy(d).cuda(), rows, cols)
        assert isinstance(g, torch.Tensor) and g.is_cuda
    else:
        g = M.sandwich_diag(d, rows, cols)
        assert isinstance(g, np.ndarray)
    assert tuple(g.shape) == (k,)
    ref, s = _ref(A, d, rows, cols)
    what = f"{name} {dtype.__name__} rows={rows_kind} cols={cols_kind}"
    err = _err(g, ref, s, what)
    print(f"{what} {side}: {err:.2e}")
    assert err <= TOL[dtype], f"{what}: {err:.2e}"
    if rows_kind != "repeats" and side == "numpy":
        H = M.sandwich(d, rows, cols)
        assert g.dtype == H.dtype


def _std_variants(M, rng):
    import tabmat_amd as tm

    w = rng.random(M.shape[0])
    w /= w.sum()
    return {"centred+scaled": M.standardize(w, True, True)[0], "scaled": M.standardize(w, False, True)[0],
            "neither": tm.StandardizedMatrix(M, np.zeros(M.shape[1]), None)}


@pytest.mark.parametrize("restrict", ["none", "rows", "cols", "both"])
@pytest.mark.parametrize("name", list(CASES))
def test_equals_the_sandwich(name, restrict):
    """Every class and StandardizedMatrix over it: the diagonal of sandwich() on the float64 units."""
    import tabmat_amd as tm

    M = _mat(name, np.float64)
    n, p = M.shape
    rng = np.random.default_rng(zlib.crc32(f"eq/{name}/{restrict}".encode()))
    rows = np.sort(rng.choice(n, n // 2, replace=False)) if restrict in ("rows", "both") else None
    cols = np.sort(rng.choice(p, max(1, p // 3), replace=False)) if restrict in ("cols", "both") else None
    d = rng.random(n)
    mats = {"plain": M}
    mats.update(_std_variants(M, rng))
    old = tm.set_strict_f64(True)
    try:
        for label, X in mats.items():
            H = X.sandwich(d, rows, cols)
            H = H.toarray() if sps.issparse(H) else _host(H)
            want = np.asarray(H.diagonal(), dtype=LD)
            for dd in (d, torch.from_numpy(d).cuda()):
                got = np.asarray(_host(X.sandwich_diag(dd, rows, cols)), dtype=LD)
                assert got.shape == want.shape
                scale = np.maximum(np.abs(want), np.finfo(np.float64).tiny)      # d >= 0: |H_jj| is the natural scale
                err = float((np.abs(got - want) / scale).max())
                print(f"{name} {label} {restrict}: {err:.2e}")
                assert err <= 1e-10, f"{name} {label} {restrict}: {err:.2e}"
    finally:
        tm.set_strict_f64(old)


@pytest.fixture(scope="module")
def std_case():
    import tabmat_amd as tm

    rng = np.random.default_rng(50)
    n = 32768
    Xd = _dense_cols(rng, n, 72)
    Xs = sps.random(n, 24, density=0.05, format="csc", random_state=rng)
    c1 = rng.integers(0, 20, n)
    c2 = rng.integers(0, 7, n)
    mat = tm.SplitMatrix([tm.DenseMatrix(Xd), tm.SparseMatrix(Xs), tm.CategoricalMatrix(c1),
                          tm.CategoricalMatrix(c2, drop_first=True)])
    w = rng.random(n)
    w /= w.sum()
    split = mat.standardize(w, True, True)[0]
    dense = tm.DenseMatrix(_dense_cols(rng, n, 40, order="F")).standardize(w, True, True)[0]
    return dict(split=(split, _standardized_ld(split)), dense=(dense, _standardized_ld(dense)), n=n)


@pytest.mark.parametrize("restrict", ["none", "rows", "cols", "both"])
@pytest.mark.parametrize("which", ["split", "dense"])
def test_standardized_uncentred_columns(std_case, which, restrict):
    """Dense columns with mean / std up to 1e4: the long-double diagonal of the STANDARDIZED columns, 1e-10 at
    every mean / std."""
    std, Z = std_case[which]
    n, p = std.shape
    assert np.abs(std.shift).max() > 5e3
    rng = np.random.default_rng(zlib.crc32(f"std/{which}/{restrict}".encode()))
    rows = np.sort(rng.choice(n, n // 2, replace=False)) if restrict in ("rows", "both") else None
    cols = np.sort(rng.choice(p, p // 3, replace=False)) if restrict in ("cols", "both") else None
    d = rng.random(n)
    ref, s = _ref(Z, d, rows, cols)
    for dd in (d, torch.from_numpy(d).cuda()):
        got = std.sandwich_diag(dd, rows, cols)
        assert _host(got).dtype == np.float64
        err = _err(got, ref, s)
        print(f"standardized {which} {restrict}: {err:.2e}")
        assert err <= 1e-10, f"standardized {which} {restrict}: {err:.2e}"


@pytest.mark.parametrize("dtype,suf", [(np.float64, "f64"), (np.float32, "f32")])
def test_dense_kernel_reached(dtype, suf):
    import tabmat_amd as tm

    rng = np.random.default_rng(1)
    n = 20_000
    X = rng.standard_normal((n, 96)).astype(dtype)
    d = _weights(rng, n, dtype, True)
    M = tm.DenseMatrix(X)
    before = _spy()
    g = M.sandwich_diag(d)
    after = _spy()
    assert _called(before, after, f"tm_dense_sandwich_diag_{suf}")
    assert not _called(before, after, f"tm_dense_col_sq_dev_{suf}")
    assert not _called(before, after, f"tm_dense_sandwich_{suf}")
    ref, s = _ref(X, d, None, None)
    assert _err(g, ref, s) <= TOL[dtype]
    # inside a split, and centred inside the kernel for a standardized matrix
    specs, idx = cs.mixed_specs(n, 128, 64, (30, 5), seed=3)
    S = to_tm_split(specs, idx, dtype=dtype)
    before = _spy()
    S.sandwich_diag(rng.random(n).astype(dtype))
    assert _called(before, _spy(), f"tm_dense_sandwich_diag_{suf}")


@pytest.mark.parametrize("dtype,suf", [(np.float64, "f64"), (np.float32, "f32")])
def test_sparse_kernels_reached(dtype, suf):
    """A block that holds the 16-bit column twin after to_device() runs on it and widens nothing; a small block runs
    the int32-column form.  Both moments (StandardizedMatrix) and the second one alone."""
    import tabmat_amd as tm
    from tabmat_amd.ext import _types as ty
    from tabmat_amd.ext import sparse as xs

    rng = np.random.default_rng(2)
    n, m = 200_000, 128
    S = sps.random(n, m, density=0.05, format="csc", random_state=rng, dtype=dtype)
    assert S.nnz >= xs.CSR_U16_MIN_NNZ
    M = tm.SparseMatrix(S).to_device()
    A = M._dev()
    assert A._ind32 is None and A._ind16 is not None, "the block must be compacted to its 16-bit columns"
    ty.release_index_scratch()
    d = _weights(rng, n, dtype, True)
    d_dev = torch.from_numpy(d).cuda()
    w = rng.random(n)
    std = M.standardize(w / w.sum(), True, True)[0]
    Z = _standardized_ld(std)
    ty.release_index_scratch()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    before = _spy()
    g = M.sandwich_diag(d_dev)
    gs = std.sandwich_diag(d_dev)
    torch.cuda.synchronize()
    after = _spy()
    grow = torch.cuda.max_memory_allocated() - base
    assert after.get(f"tm_csr_sandwich_diag_u16_{suf}", 0) - before.get(f"tm_csr_sandwich_diag_u16_{suf}", 0) == 2
    assert not _called(before, after, f"tm_csr_col_sq_{suf}")
    assert not _called(before, after, f"tm_csr_sandwich_diag_{suf}")
    assert grow < S.nnz * 4, f"peak growth {grow} bytes: an nnz-sized widening scratch was allocated"
    assert A._ind32 is None and not ty._WIDE
    Ad = S.toarray()
    ref, s = _ref(Ad, d, None, None)
    assert _err(g, ref, s) <= TOL[dtype]
    ref, s = _ref(Z, d, None, None)
    assert _err(gs, ref, s) <= (1e-10 if dtype == np.float64 else 1e-4)

    small = sps.random(3000, 30, density=0.1, format="csc", random_state=rng, dtype=dtype)
    Ms = tm.SparseMatrix(small).to_device()
    assert Ms._dev()._ind32 is not None
    ds = _weights(rng, 3000, dtype, True)
    ws = rng.random(3000)
    before = _spy()
    g = Ms.sandwich_diag(ds)
    gs = Ms.standardize(ws / ws.sum(), True, True)[0].sandwich_diag(ds)
    after = _spy()
    assert after.get(f"tm_csr_sandwich_diag_{suf}", 0) - before.get(f"tm_csr_sandwich_diag_{suf}", 0) == 2
    ref, s = _ref(small.toarray(), ds, None, None)
    assert _err(g, ref, s) <= TOL[dtype]


def test_sparse_wider_than_the_bins():
    """More columns than two LDS bin arrays hold: the two single-moment launches, same answer."""
    import tabmat_amd as tm

    rng = np.random.default_rng(4)
    n, m = 4000, 7000
    S = sps.random(n, m, density=0.002, format="csc", random_state=rng)
    M = tm.SparseMatrix(S)
    w = rng.random(n)
    std = M.standardize(w / w.sum(), True, True)[0]
    d = _weights(rng, n, np.float64, True)
    before = _spy()
    gs = std.sandwich_diag(d)
    after = _spy()
    assert _called(before, after, "tm_csr_col_sq_f64") and not _called(before, after, "tm_csr_sandwich_diag_f64")
    ref, s = _ref(_standardized_ld(std), d, None, None)
    assert _err(gs, ref, s) <= 1e-10
    ref, s = _ref(S.toarray(), d, None, None)
    assert _err(M.sandwich_diag(d), ref, s) <= 1e-12


@pytest.mark.parametrize("width,dtype", [(w, dt) for dt in (np.float64, np.float32)
                                         for w in (1, 7, 8, 63, 130, 512)]
                         + [(1024, np.float64), (1025, np.float64), (2048, np.float32), (2049, np.float32)])
def test_dense_widths(width, dtype):
    """Every lane layout of the kernel, its widest block, and one column more (the column-square kernel)."""
    import tabmat_amd as tm

    rng = np.random.default_rng(width)
    n = 5003
    X = rng.standard_normal((n, width)).astype(dtype)
    d = _weights(rng, n, dtype, width % 2 == 0)
    suf = "f64" if dtype == np.float64 else "f32"
    before = _spy()
    g = tm.DenseMatrix(X).sandwich_diag(d)
    after = _spy()
    limit = 1024 if dtype == np.float64 else 2048
    assert _called(before, after, f"tm_dense_sandwich_diag_{suf}") == (width <= limit)
    assert _called(before, after, f"tm_dense_col_sq_dev_{suf}") == (width > limit)
    assert g.dtype == dtype and g.shape == (width,)
    ref, s = _ref(X, d, None, None)
    err = _err(g, ref, s)
    print(f"width {width} {suf}: {err:.2e}")
    assert err <= TOL[dtype]


def test_reproducible():
    import tabmat_amd as tm

    rng = np.random.default_rng(5)
    n = 200_000
    M = tm.DenseMatrix(rng.standard_normal((n, 128)))
    d = torch.from_numpy(rng.random(n)).cuda()
    assert torch.equal(M.sandwich_diag(d), M.sandwich_diag(d))
    specs, idx = cs.mixed_specs(100_000, 128, 64, (50, 7), seed=4)
    S = to_tm_split(specs, idx)
    d = torch.from_numpy(rng.random(S.shape[0])).cuda()
    a, b = S.sandwich_diag(d), S.sandwich_diag(d)
    dense_cols = torch.from_numpy(np.asarray(idx[0], dtype=np.int64)).cuda()
    assert torch.equal(a[dense_cols], b[dense_cols])
    if DET:
        cat_cols = torch.from_numpy(np.concatenate([np.asarray(i, dtype=np.int64) for i in idx[2:]])).cuda()
        assert torch.equal(a[cat_cols], b[cat_cols])


@pytest.mark.parametrize("kind", ["dense", "split", "standardized"])
def test_non_finite(kind):
    """inf / nan in an excluded row and in an unselected column leave the selected entries finite and right."""
    import tabmat_amd as tm

    rng = np.random.default_rng(9)
    n = 4000
    X = rng.standard_normal((n, 70))
    X[17, 5] = np.inf
    X[30, 6] = np.nan
    X[2000, 1] = np.inf          # in a selected column, in a row the row list leaves out
    Sx = sps.random(n, 12, density=0.1, format="csc", random_state=rng).tolil()
    Sx[2001, 3] = np.inf
    if kind == "dense":
        M = tm.DenseMatrix(X)
        cols = np.array([0, 1, 2, 40, 69])
    else:
        M = tm.SplitMatrix([tm.DenseMatrix(X), tm.SparseMatrix(Sx.tocsc()), tm.CategoricalMatrix(rng.integers(0, 9, n))])
        cols = np.array([0, 1, 2, 40, 69, 73, 75, 84])
    A = _dense_of(M)
    if kind == "standardized":
        shift, mult = rng.standard_normal(M.shape[1]), 0.5 + rng.random(M.shape[1])
        M = tm.StandardizedMatrix(M, shift, mult)
        A = A * mult[None, :] + shift[None, :]
    d = rng.random(n)
    rows = np.arange(100, 900)
    for dd in (d, torch.from_numpy(d).cuda()):
        g = _host(M.sandwich_diag(dd, rows, cols))
        with np.errstate(invalid="ignore"):
            ref, s = _ref(A, d, rows, cols)
        assert np.isfinite(g).all() and _err(g, ref, s) <= 1e-12
    cols2 = np.array([0, 2, 40, 69])           # the column holding the inf of row 2000 is left out
    g = _host(M.sandwich_diag(d, cols=cols2))
    with np.errstate(invalid="ignore"):
        ref, s = _ref(A, d, None, cols2)
    assert np.isfinite(g).all() and _err(g, ref, s) <= 1e-12


def test_scale_sandwich_cannot_reach():
    """1M rows, 8 dense columns and one categorical of 400 000 levels: the (p, p) float64 sandwich would be
    1.28 TB; its diagonal needs device vectors only."""
    import tabmat_amd as tm

    n, k, L = 1_000_000, 8, 400_000
    rng = np.random.default_rng(400)
    X = rng.standard_normal((n, k))
    codes = rng.integers(0, L, n).astype(np.int32)
    M = tm.SplitMatrix([tm.DenseMatrix(X), tm.CategoricalMatrix(codes, categories=np.arange(L))])
    M.to_device()
    d = rng.random(n)
    d_dev = torch.from_numpy(d).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    g = M.sandwich_diag(d_dev)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    assert grow < (1 << 28), f"peak growth {grow / 2**20:.0f} MiB"
    assert g.shape == (k + L,)
    want = torch.bincount(torch.from_numpy(codes.astype(np.int64)).cuda(), weights=d_dev, minlength=L)
    gc = g[k:]
    rel = float(((gc - want).abs() / want.clamp_min(1e-300)).max())
    assert rel <= 1e-12, rel
    assert bool((gc[want == 0] == 0).all())
    ref, s = _ref(X, d, None, None)
    assert _err(g[:k], ref, s) <= 1e-12


def _zipf_design(n, levels, seed):
    import tabmat_amd as tm

    rng = np.random.default_rng(seed)
    Xd = rng.random((n, 16))
    Xs = sps.random(n, 64, density=0.05, format="csc", random_state=rng, data_rvs=rng.random)
    pr = 1.0 / np.arange(1, levels + 1)
    codes = rng.choice(levels, size=n, p=pr / pr.sum()).astype(np.int32)
    X = tm.SplitMatrix([tm.DenseMatrix(Xd), tm.SparseMatrix(Xs),
                        tm.CategoricalMatrix(codes, categories=np.arange(levels))]).to_device()
    E_eta = lambda b: Xd @ b[:16] + Xs @ b[16:80] + b[80:][codes]      # noqa: E731
    truth = 0.02 * rng.standard_normal(80 + levels)
    y = rng.poisson(np.exp(E_eta(truth))).astype(np.float64)
    return X, torch.from_numpy(y).cuda()


def test_preconditioned_newton_cg():
    """Zipf-distributed categorical next to dense and sparse columns: Jacobi-preconditioned CG reaches the
    coefficients of plain CG in at most half of its steps (the same design on the CPU: 9-10x fewer)."""
    import glm_newton_cg

    X, y = _zipf_design(20_000, 2_000, 21)
    steps = {}
    betas = {}
    for pre in (False, True):
        ks = []
        betas[pre] = glm_newton_cg.fit_poisson_newton_cg(
            X, y, alpha=1.0, iters=6, cg_rtol=1e-6, cg_maxiter=2000, tol=0.0, precondition=pre,
            callback=lambda it, beta, step, k, dev: ks.append(k))
        steps[pre] = ks
    print("CG steps per Newton iteration: plain", steps[False], "Jacobi", steps[True])
    rel = float((betas[True] - betas[False]).norm() / betas[False].norm())
    assert rel <= 1e-6, rel
    assert 2 * sum(steps[True]) <= sum(steps[False]), (steps[True], steps[False])
