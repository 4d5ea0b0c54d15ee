"""sandwich_matvec: g = X[rows][:, cols]' (d[rows] * (X[rows][:, cols] u)) without forming the sandwich.  Compared with
long-double numpy at the natural scale s_j = sum_i |d_i| |a_ij| sum_k |a_ik| |u_k| and with sandwich(d, rows, cols) @ u;
the ABI spy proves that the one-pass dense kernel (tm_dense_sandwich_matvec_*) runs."""
import os
import zlib

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import _cases as cs
from _gpu_util import to_tm_block, to_tm_split

pytestmark = pytest.mark.gpu

DET = os.environ.get("TABMAT_AMD_DETERMINISTIC", "0") == "1"
LD = np.longdouble
TOL = {np.float64: 1e-12, np.float32: 1e-4}


def _spy():
    from conftest import ABI_CALLS

    return dict(ABI_CALLS)


def _called(before, after, name):
    return after.get(name, 0) > before.get(name, 0)


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


def _ref(A, d, u, rows, cols):
    """(long-double g, natural scale s) of A[rows][:, cols]' (d[rows] * (A[rows][:, cols] u))."""
    A = np.asarray(A, dtype=LD)
    d = np.asarray(d, dtype=LD)
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64)
        A, d = A[r], d[r]
    if cols is not None:
        A = A[:, np.asarray(cols, dtype=np.int64)]
    u = np.asarray(u, dtype=LD)
    g = A.T @ (d * (A @ u))
    Aa = np.abs(A)
    s = Aa.T @ (np.abs(d) * (Aa @ np.abs(u)))
    return g, s


def _err(got, g_ref, s):
    got = np.asarray(_host(got), dtype=LD)
    if got.size == 0:
        return 0.0
    scale = np.maximum(s, np.finfo(np.float64).tiny)
    return float((np.abs(got - g_ref) / scale).max())


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


def _mat(name, dtype):
    key = (name, dtype)
    if key not in _BUILT:
        _BUILT[key] = CASES[name](dtype)
    return _BUILT[key]


def _rows(kind, n, rng):
    if kind == "none":
        return None
    if kind == "sorted":
        return np.sort(rng.choice(n, size=max(1, (2 * n) // 3), replace=False))
    if kind == "repeats":
        r = rng.choice(n, size=max(1, n // 2), replace=True)
        return np.concatenate([r, r[: max(1, len(r) // 4)]])[::-1]
    return np.array([], dtype=np.int64)


def _cols(kind, p, rng):
    if kind == "none":
        return None
    if kind == "subset":
        return np.sort(rng.choice(p, size=max(1, p // 2), replace=False))
    return np.array([], dtype=np.int64)


@pytest.mark.parametrize("side", ["numpy", "device"])
@pytest.mark.parametrize("cols_kind", ["none", "subset", "empty"])
@pytest.mark.parametrize("rows_kind", ["none", "sorted", "repeats", "empty"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", list(CASES))
def test_parity(name, dtype, rows_kind, cols_kind, side):
    M = _mat(name, dtype)
    n, p = M.shape
    rng = np.random.default_rng(zlib.crc32(f"{name}/{rows_kind}/{cols_kind}".encode()))
    A = M.toarray()
    A = A.toarray() if sps.issparse(A) else np.asarray(A)
    rows = _rows(rows_kind, n, rng)
    cols = _cols(cols_kind, p, rng)
    k = p if cols is None else len(cols)
    d = rng.random(n).astype(dtype)
    u = rng.standard_normal(k).astype(dtype)
    if side == "device":
        g = M.sandwich_matvec(torch.from_numpy(d).cuda(), torch.from_numpy(u).cuda(), rows, cols)
        assert isinstance(g, torch.Tensor) and g.is_cuda
    else:
        g = M.sandwich_matvec(d, u, rows, cols)
        assert isinstance(g, np.ndarray)
    assert tuple(g.shape) == (k,)
    g_ref, s = _ref(A, d, u, rows, cols)
    err = _err(g, g_ref, s)
    assert err <= TOL[dtype], f"{name} {dtype.__name__} rows={rows_kind} cols={cols_kind}: {err:.2e}"
    if rows_kind != "repeats":
        H = M.sandwich(d, rows, cols)
        H = H.toarray() if sps.issparse(H) else _host(H)
        want = H @ u
        if side == "numpy":
            assert g.dtype == want.dtype
        assert _err(g, np.asarray(want, dtype=LD), s) <= 10 * TOL[dtype]


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


@pytest.mark.parametrize("restrict", ["none", "rows", "cols"])
def test_standardized_uncentred_columns(restrict):
    rng = np.random.default_rng(50)
    n = 20_000
    std = _std_split(rng, n)
    X = std.mat.toarray().astype(LD)
    Z = X * std.mult.astype(LD)[None, :] + std.shift.astype(LD)[None, :]
    p = std.shape[1]
    rows = np.sort(rng.choice(n, n // 2, replace=False)) if restrict == "rows" else None
    cols = np.sort(rng.choice(p, p // 3, replace=False)) if restrict == "cols" else None
    d = rng.random(n)
    u = rng.standard_normal(p if cols is None else len(cols))
    before = _spy()
    g = std.sandwich_matvec(d, u, rows, cols)
    assert _called(before, _spy(), "tm_dense_sandwich_matvec_f64")
    g_ref, s = _ref(Z, d, u, rows, cols)
    assert _err(g, g_ref, s) <= 1e-10
    gd = std.sandwich_matvec(torch.from_numpy(d).cuda(), torch.from_numpy(u).cuda(), rows, cols)
    assert _err(gd, g_ref, s) <= 1e-10


@pytest.mark.parametrize("dtype,sym", [(np.float64, "tm_dense_sandwich_matvec_f64"),
                                       (np.float32, "tm_dense_sandwich_matvec_f32")])
def test_fused_path_taken(dtype, sym):
    specs, idx = cs.mixed_specs(20_000, 128, 64, (30, 5), seed=3)
    M = to_tm_split(specs, idx, dtype=dtype)
    rng = np.random.default_rng(0)
    d = rng.random(M.shape[0]).astype(dtype)
    u = rng.standard_normal(M.shape[1]).astype(dtype)
    before = _spy()
    g = M.sandwich_matvec(d, u)
    after = _spy()
    assert _called(before, after, sym)
    # the dense block is not read by a separate matvec / transpose_matvec
    suf = "f64" if dtype == np.float64 else "f32"
    assert not _called(before, after, f"tm_dense_matvec_{suf}")
    assert not _called(before, after, f"tm_dense_rmatvec_{suf}")
    g_ref, s = _ref(M.toarray(), d, u, None, None)
    assert _err(g, g_ref, s) <= TOL[dtype]


@pytest.mark.parametrize("width", [1, 3, 10, 17, 64, 127, 256, 513, 1024])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_dense_widths(width, dtype):
    """Every lane layout of the kernel (8 .. 64 lanes per row, 1 .. 8 loads per lane, aligned or not)."""
    import tabmat_amd as tm

    rng = np.random.default_rng(width)
    n = 5003
    X = rng.standard_normal((n, width)).astype(dtype)
    d = rng.random(n).astype(dtype)
    u = rng.standard_normal(width).astype(dtype)
    M = tm.DenseMatrix(X)
    g = M.sandwich_matvec(d, u)
    g_ref, s = _ref(X, d, u, None, None)
    assert g.dtype == dtype
    assert _err(g, g_ref, s) <= TOL[dtype]


def test_dense_reproducible():
    import tabmat_amd as tm

    rng = np.random.default_rng(5)
    n = 200_000
    M = tm.DenseMatrix(rng.standard_normal((n, 128)))
    d = torch.from_numpy(rng.random(n)).cuda()
    u = torch.from_numpy(rng.standard_normal(128)).cuda()
    a = M.sandwich_matvec(d, u)
    b = M.sandwich_matvec(d, u)
    assert torch.equal(a, b)


def test_split_reproducible():
    if not DET:
        pytest.skip("the categorical transpose_matvec uses atomics outside TABMAT_AMD_DETERMINISTIC=1")
    # (dense + categoricals: the sparse rmatvec has no fixed-order form in any mode)
    specs, idx = cs.mixed_specs(100_000, 128, 0, (50, 7), seed=4)
    M = to_tm_split(specs, idx)
    rng = np.random.default_rng(2)
    d = torch.from_numpy(rng.random(M.shape[0])).cuda()
    u = torch.from_numpy(rng.standard_normal(M.shape[1])).cuda()
    assert torch.equal(M.sandwich_matvec(d, u), M.sandwich_matvec(d, u))


@pytest.mark.parametrize("kind", ["dense", "split"])
def test_inf_in_unselected_column(kind):
    import tabmat_amd as tm

    rng = np.random.default_rng(9)
    n = 4000
    X = rng.standard_normal((n, 70))
    X[17, 5] = np.inf
    X[30, 6] = np.nan
    if kind == "dense":
        M = tm.DenseMatrix(X)
    else:
        M = tm.SplitMatrix([tm.DenseMatrix(X), tm.CategoricalMatrix(rng.integers(0, 9, n))])
    cols = np.array([0, 1, 2, 40, 69] + ([72] if kind == "split" else []))
    d = rng.random(n)
    u = rng.standard_normal(len(cols))
    g = M.sandwich_matvec(d, u, cols=cols)
    assert np.isfinite(g).all()
    A = M.toarray()
    g_ref, s = _ref(A, d, u, None, cols)
    assert _err(g, g_ref, s) <= 1e-12
    rows = np.arange(100, 900)
    g = M.sandwich_matvec(d, u, rows, cols)
    g_ref, s = _ref(A, d, u, rows, cols)
    assert np.isfinite(g).all() and _err(g, g_ref, s) <= 1e-12


def test_scale_sandwich_cannot_reach():
    """4M rows, 16 dense columns and one categorical of 400 000 levels: the (p, p) float64 sandwich would be
    1.28 TB; sandwich_matvec needs device vectors only."""
    import tabmat_amd as tm

    n, k, L = 4_000_000, 16, 400_000
    rng = np.random.default_rng(400)
    X = rng.standard_normal((n, k))
    codes = rng.integers(0, L, n).astype(np.int32)
    M = tm.SplitMatrix([tm.DenseMatrix(X), tm.CategoricalMatrix(codes, categories=np.arange(L))])
    M.to_device()
    p = k + L
    d = rng.random(n)
    u = rng.standard_normal(p)
    d_dev, u_dev = torch.from_numpy(d).cuda(), torch.from_numpy(u).cuda()
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    g = M.sandwich_matvec(d_dev, u_dev)
    torch.cuda.synchronize()
    grow = torch.cuda.max_memory_allocated() - base
    assert grow < (1 << 30), f"peak growth {grow / 2**30:.2f} GiB"
    g = g.cpu().numpy()
    # host reference from the codes: t = X u_dense + u_cat[code], w = d t
    t = X @ u[:k] + u[k:][codes]
    w = d * t
    gd_ref = X.T @ w
    scale_d = np.abs(X).T @ (d * (np.abs(X) @ np.abs(u[:k]) + np.abs(u[k:][codes])))
    assert float((np.abs(g[:k] - gd_ref) / scale_d).max()) <= 1e-11
    lv = rng.choice(L, 300, replace=False)
    sel = np.isin(codes, lv)
    want = np.zeros(L, dtype=LD)
    np.add.at(want, codes[sel], w[sel].astype(LD))
    scale_c = np.zeros(L)
    np.add.at(scale_c, codes[sel], (d * (np.abs(X) @ np.abs(u[:k]) + np.abs(u[k:][codes])))[sel])
    got = g[k:][lv].astype(LD)
    assert float((np.abs(got - want[lv]) / np.maximum(scale_c[lv], 1e-300)).max()) <= 1e-12
