"""sandwich_and_transpose_matvec: (H, g) = (sandwich(d, rows, cols), transpose_matvec(v, rows, cols)) from one call,
the dense block's syrk carrying v through its own pass (tm_dense_sandwich_*_xtv_f64).  Compared with the two
separate calls, with long-double numpy and with the oracle; the ABI spy proves that the dense block is read once."""
import os

import numpy as np
import pytest
import torch

import _cases as cs
from _gpu_util import nat_err, rel_err, to_tm_split

pytestmark = pytest.mark.gpu

DET = os.environ.get("TABMAT_AMD_DETERMINISTIC", "0") == "1"


def _ld_ref(X, d, v, rows=None):
    """(X[rows]' diag(d[rows]) X[rows], X[rows]' v[rows]) in long double (repeated rows count per occurrence)."""
    X = np.asarray(X, dtype=np.longdouble)
    d = np.asarray(d, dtype=np.longdouble)
    v = np.asarray(v, dtype=np.longdouble)
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64)
        X, d, v = X[r], d[r], v[r]
    return (X.T * d) @ X, X.T @ v


def _g_err(g, ref, X, v, rows=None):
    """max |g - ref| relative to X' |v| (the scale of the sum)."""
    Xa = np.abs(np.asarray(X, dtype=np.float64))
    va = np.abs(np.asarray(v, dtype=np.float64))
    if rows is not None:
        r = np.asarray(rows, dtype=np.int64)
        Xa, va = Xa[r], va[r]
    scale = max(float((Xa.T @ va).max()), 1e-300)
    return float(np.abs(np.asarray(g, dtype=np.float64) - np.asarray(ref, dtype=np.float64)).max() / scale)


def _spy():
    from conftest import ABI_CALLS

    return dict(ABI_CALLS)


def _called(before, after, prefix):
    return sorted(k for k in after if k.startswith(prefix) and after[k] > before.get(k, 0))


@pytest.mark.parametrize("width", [2, 64, 97, 128, 256])
def test_dense_widths(width):
    import tabmat_amd as tm

    rng = np.random.default_rng(width)
    n = 20_000
    X = rng.standard_normal((n, width))
    d = rng.random(n)
    v = rng.standard_normal(n)
    M = tm.DenseMatrix(X)
    H, g = M.sandwich_and_transpose_matvec(d, v)
    assert isinstance(H, np.ndarray) and isinstance(g, np.ndarray)
    assert H.dtype == np.float64 and g.dtype == np.float64 and H.shape == (width, width) and g.shape == (width,)
    Hr, gr = _ld_ref(X, d, v)
    assert nat_err(H, Hr) < 1e-10
    assert _g_err(g, gr, X, v) < 1e-12
    assert nat_err(H, M.sandwich(d)) < 1e-10
    assert _g_err(g, M.transpose_matvec(v), X, v) < 1e-12


def test_dense_one_pass_spy():
    """An unrestricted float64 block of <= 128 columns: H and g without any dense transpose_matvec launch."""
    import tabmat_amd as tm

    if DET:
        pytest.skip("deterministic mode keeps the two passes")
    rng = np.random.default_rng(1)
    n = 30_000
    X = rng.standard_normal((n, 128))
    d, v = rng.random(n), rng.standard_normal(n)
    M = tm.DenseMatrix(X)
    M.to_device()
    dd, vd = torch.tensor(d, device="cuda"), torch.tensor(v, device="cuda")
    b = _spy()
    H, g = M.sandwich_and_transpose_matvec(dd, vd)
    torch.cuda.synchronize()
    a = _spy()
    assert _called(b, a, "tm_dense_rmatvec") == []
    assert _called(b, a, "tm_dense_sandwich_i8_xtv_f64") == ["tm_dense_sandwich_i8_xtv_f64"]
    assert H.is_cuda and g.is_cuda and g.dtype == torch.float64
    Hr, gr = _ld_ref(X, d, v)
    assert nat_err(H.cpu().numpy(), Hr) < 1e-10
    assert _g_err(g.cpu().numpy(), gr, X, v) < 1e-12


def test_dense_outside_envelope():
    """A column scaled by 1e6 and a negative weight: K1e hands the call to K1c on the device, which must write g."""
    import tabmat_amd as tm

    rng = np.random.default_rng(2)
    n = 20_000
    X = rng.standard_normal((n, 100))
    X[:, 7] *= 1e6
    d = rng.random(n)
    d[123] = -0.5
    v = rng.standard_normal(n)
    M = tm.DenseMatrix(X)
    H, g = M.sandwich_and_transpose_matvec(d, v)
    Hr, gr = _ld_ref(X, d, v)
    assert rel_err(H, Hr) < 1e-12
    assert _g_err(g, gr, X, v) < 1e-12
    # and inside the envelope again on the same matrix (the history of the int8 kernel)
    d2 = rng.random(n)
    X2 = X.copy()
    H2, g2 = M.sandwich_and_transpose_matvec(d2, v)
    Hr2, gr2 = _ld_ref(X2, d2, v)
    assert nat_err(H2, Hr2) < 1e-10 and _g_err(g2, gr2, X, v) < 1e-12


def test_dense_strict_f64_k1c():
    """strict float64 (no int8 syrk): the K1c form carries v."""
    import tabmat_amd as tm
    from tabmat_amd import dense_matrix as dm

    rng = np.random.default_rng(3)
    n = 10_000
    X = rng.standard_normal((n, 97))
    d, v = rng.random(n), rng.standard_normal(n)
    old = dm.set_strict_f64(True)
    try:
        H, g = tm.DenseMatrix(X).sandwich_and_transpose_matvec(d, v)
    finally:
        dm.set_strict_f64(old)
    Hr, gr = _ld_ref(X, d, v)
    assert nat_err(H, Hr) < 1e-12 and _g_err(g, gr, X, v) < 1e-12


@pytest.mark.parametrize("order,dtype", [("F", np.float64), ("C", np.float32), ("F", np.float32)])
def test_dense_order_dtype(order, dtype):
    import tabmat_amd as tm

    rng = np.random.default_rng(4)
    n = 8_000
    X = rng.standard_normal((n, 96)).astype(dtype)
    X = np.asfortranarray(X) if order == "F" else X
    d, v = rng.random(n).astype(dtype), rng.standard_normal(n).astype(dtype)
    M = tm.DenseMatrix(X)
    H, g = M.sandwich_and_transpose_matvec(d, v)
    gs = M.transpose_matvec(v)
    assert g.dtype == gs.dtype and H.dtype == M.sandwich(d).dtype
    tol = 1e-10 if dtype == np.float64 else 1e-5
    Hr, gr = _ld_ref(X, d, v)
    assert nat_err(H, Hr) < tol and _g_err(g, gr, X, v) < tol


@pytest.mark.parametrize("dense_kind", ["c", "f"])
def test_rows_cols_and_repeats(dense_kind):
    import tabmat_amd as tm

    rng = np.random.default_rng(5)
    n = 16_000
    X = rng.standard_normal((n, 120))
    if dense_kind == "f":
        X = np.asfortranarray(X)
    d, v = rng.random(n), rng.standard_normal(n)
    M = tm.DenseMatrix(X)
    rows_big = np.sort(rng.choice(n, n // 2, replace=False))
    rows_big = np.concatenate([rows_big, rows_big[:50]])          # repeated ids (masked weights count them twice)
    rows_small = rng.choice(n, 300, replace=True)
    cols = np.sort(rng.choice(120, 40, replace=False))
    for rows, cl in [(rows_big, None), (rows_small, None), (None, cols), (rows_big, cols), (rows_small, cols)]:
        H, g = M.sandwich_and_transpose_matvec(d, v, rows, cl)
        Hs, gs = M.sandwich(d, rows, cl), M.transpose_matvec(v, rows, cl)
        assert H.shape == Hs.shape and g.shape == gs.shape
        assert nat_err(H, Hs) < 1e-10
        Xc = X if cl is None else X[:, cl]
        assert _g_err(g, gs, Xc, v, rows) < 1e-12
        Hr, gr = _ld_ref(Xc, d, v, rows)
        assert nat_err(H, Hr) < 1e-10 and _g_err(g, gr, Xc, v, rows) < 1e-12


def test_zero_weights_and_vectors():
    import tabmat_amd as tm

    rng = np.random.default_rng(6)
    n = 12_000
    X = rng.standard_normal((n, 80))
    M = tm.DenseMatrix(X)
    d = rng.random(n)
    v = rng.standard_normal(n)
    dz = d.copy()
    dz[: n // 2] = 0.0                    # d = 0 where v != 0
    vz = v.copy()
    vz[n // 2:] = 0.0                     # v = 0 where d != 0 (in the other half)
    for dd, vv in [(dz, v), (d, vz), (dz, vz), (np.zeros(n), v), (d, np.zeros(n))]:
        H, g = M.sandwich_and_transpose_matvec(dd, vv)
        Hr, gr = _ld_ref(X, dd, vv)
        assert nat_err(H, Hr) < 1e-10
        assert _g_err(g, gr, X, vv if np.any(vv) else np.ones(n)) < 1e-12
    H, g = M.sandwich_and_transpose_matvec(d, d)              # v is d
    Hr, gr = _ld_ref(X, d, d)
    assert nat_err(H, Hr) < 1e-10 and _g_err(g, gr, X, d) < 1e-12


def test_errors():
    import tabmat_amd as tm

    rng = np.random.default_rng(7)
    n = 500
    M = tm.DenseMatrix(rng.standard_normal((n, 10)))
    d, v = rng.random(n), rng.standard_normal(n)
    with pytest.raises(NotImplementedError):
        M.sandwich_and_transpose_matvec(d, np.ones((n, 2)))
    for bad_d, bad_v in [(d[:-1], v), (d, v[:-1])]:
        with pytest.raises(ValueError):
            M.sandwich_and_transpose_matvec(bad_d, bad_v)
    specs, idx = cs.mixed_specs(n, 4, 6, (5, 3), seed=1)
    S = to_tm_split(specs, idx)
    with pytest.raises(NotImplementedError):
        S.sandwich_and_transpose_matvec(d, np.ones((n, 2)))
    with pytest.raises(ValueError):
        S.sandwich_and_transpose_matvec(d, v[:-1])


@pytest.mark.parametrize("missing,drop_first,cats", [(False, False, (40, 12, 6)), (True, False, (40, 12)),
                                                     (False, True, (30,)), (True, True, (9, 7))])
def test_split_mixed_oracle(missing, drop_first, cats):
    from oracle import oracle as orc

    n = 20_000
    specs, idx = cs.mixed_specs(n, 128, 64, cats, seed=11, missing=missing, drop_first=drop_first)
    mat = to_tm_split(specs, idx)
    blocks = [cs.to_oracle_block(s) for s in specs]
    rng = np.random.default_rng(8)
    d, v = rng.random(n), rng.standard_normal(n)
    b = _spy()
    H, g = mat.sandwich_and_transpose_matvec(d, v)
    a = _spy()
    assert nat_err(H, orc.split_sandwich(blocks, idx, d)) < 1e-10
    assert rel_err(g, orc.split_transpose_matvec(blocks, idx, v)) < 1e-12
    assert nat_err(H, mat.sandwich(d)) < 1e-10
    assert rel_err(g, mat.transpose_matvec(v)) < 1e-12
    if not DET:
        assert _called(b, a, "tm_dense_rmatvec_f64") == []
        if len(cats) >= 2:                # (one histogram launch for every categorical block)
            assert _called(b, a, "tm_cat_transpose_matvec_f64") == []


def test_split_rows_cols_oracle():
    from oracle import oracle as orc

    n = 12_000
    specs, idx = cs.mixed_specs(n, 96, 40, (20, 6), seed=12, missing=True)
    mat = to_tm_split(specs, idx)
    blocks = [cs.to_oracle_block(s) for s in specs]
    p = mat.shape[1]
    rng = np.random.default_rng(9)
    d, v = rng.random(n), rng.standard_normal(n)
    rows_big = np.sort(rng.choice(n, 2 * n // 3, replace=False)).astype(np.int32)
    rows_rep = np.concatenate([rows_big, rows_big[:40]])
    cols_wide = np.sort(rng.choice(p, int(0.8 * p), replace=False))
    cols_narrow = np.sort(rng.choice(p, 30, replace=False))
    for rows, cols in [(rows_big, None), (rows_rep, None), (None, cols_wide), (rows_big, cols_wide),
                       (None, cols_narrow), (rows_big[:200], cols_narrow)]:
        H, g = mat.sandwich_and_transpose_matvec(d, v, rows, cols)
        Hs, gs = mat.sandwich(d, rows, cols), mat.transpose_matvec(v, rows, cols)
        assert nat_err(H, Hs) < 1e-10 and rel_err(g, gs) < 1e-12
        if rows is rows_rep:
            continue                      # (the oracle's row lists are sets here)
        assert nat_err(H, orc.split_sandwich(blocks, idx, d, rows, cols)) < 1e-10
        assert rel_err(g, orc.split_transpose_matvec(blocks, idx, v, rows, cols)) < 1e-12


def test_split_sparse_and_cats_alone():
    """Blocks without a one-pass kernel (sparse on the entry twin / lane-group kernels, lone categoricals) keep the
    separate transpose_matvec launch: g stays complete."""
    from oracle import oracle as orc

    n = 15_000
    for k_dense, k_sparse, cats in [(0, 64, ()), (0, 0, (50,)), (32, 200, (17,)), (128, 300, ())]:
        specs, idx = cs.mixed_specs(n, k_dense, k_sparse, cats, seed=13, missing=bool(cats))
        mat = to_tm_split(specs, idx)
        blocks = [cs.to_oracle_block(s) for s in specs]
        rng = np.random.default_rng(10)
        d, v = rng.random(n), rng.standard_normal(n)
        H, g = mat.sandwich_and_transpose_matvec(d, v)
        assert nat_err(H, orc.split_sandwich(blocks, idx, d)) < 1e-10
        assert rel_err(g, orc.split_transpose_matvec(blocks, idx, v)) < 1e-12
    for spec in [cs.mixed_specs(n, 0, 64, (), seed=14)[0][0], ("cat", np.arange(n, dtype=np.int32) % 33, 33, True)]:
        from _gpu_util import to_tm_block

        blk = to_tm_block(spec)
        rng = np.random.default_rng(11)
        d, v = rng.random(n), rng.standard_normal(n)
        H, g = blk.sandwich_and_transpose_matvec(d, v)
        Hs = blk.sandwich(d)
        assert type(H) is type(Hs)            # (a lone categorical's sandwich is a scipy.sparse diagonal, as in tabmat)
        H, Hs = (x.toarray() if hasattr(x, "toarray") else x for x in (H, Hs))
        assert nat_err(H, Hs) < 1e-12 and rel_err(g, blk.transpose_matvec(v)) < 1e-12


def test_split_f32_and_device_inputs():
    n = 10_000
    specs, idx = cs.mixed_specs(n, 96, 40, (12, 5), seed=15)
    rng = np.random.default_rng(12)
    d, v = rng.random(n), rng.standard_normal(n)
    m32 = to_tm_split(specs, idx, dtype=np.float32)
    H, g = m32.sandwich_and_transpose_matvec(d.astype(np.float32), v.astype(np.float32))
    gs = m32.transpose_matvec(v.astype(np.float32))
    assert g.dtype == gs.dtype and rel_err(g, gs) < 1e-5
    assert rel_err(H, m32.sandwich(d.astype(np.float32))) < 1e-5
    mat = to_tm_split(specs, idx)
    dd, vd = torch.tensor(d, device="cuda"), torch.tensor(v, device="cuda")
    H1, g1 = mat.sandwich_and_transpose_matvec(dd, v)          # device d, numpy v: H on the device, g on the host
    assert H1.is_cuda and isinstance(g1, np.ndarray)
    H2, g2 = mat.sandwich_and_transpose_matvec(d, vd)
    assert isinstance(H2, np.ndarray) and g2.is_cuda
    assert nat_err(H1.cpu().numpy(), H2) < 1e-10 and rel_err(g1, g2.cpu().numpy()) < 1e-12


def test_configs3_shaped_mixed():
    """BASELINE configs[3] shape (dense 128 + sparse 512 @ 5 % + categoricals 256 / 96 / 32) at 200k rows."""
    from tabmat_amd import synth

    n = 200_000
    mat = synth.mixed_split(n)
    mat.to_device()
    g_ = torch.Generator(device="cuda").manual_seed(0)
    d = torch.rand(n, dtype=torch.float64, device="cuda", generator=g_)
    v = torch.randn(n, dtype=torch.float64, device="cuda", generator=g_)
    b = _spy()
    H, g = mat.sandwich_and_transpose_matvec(d, v)
    torch.cuda.synchronize()
    a = _spy()
    Hs, gs = mat.sandwich(d), mat.transpose_matvec(v)
    assert nat_err(H.cpu().numpy(), Hs.cpu().numpy()) < 1e-10
    assert rel_err(g.cpu().numpy(), gs.cpu().numpy()) < 1e-12
    if not DET:
        assert _called(b, a, "tm_dense_rmatvec_f64") == []
        assert _called(b, a, "tm_cat_transpose_matvec_f64") == []
        assert _called(b, a, "tm_dense_sandwich_i8_xtv_f64") == ["tm_dense_sandwich_i8_xtv_f64"]


@pytest.mark.parametrize("center,scale", [(True, True), (True, False), (False, True)])
def test_standardized(center, scale):
    n = 12_000
    specs, idx = cs.mixed_specs(n, 96, 30, (10,), seed=16)
    specs[0] = ("dense", specs[0][1] * 3.0 + 50.0)
    mat = to_tm_split(specs, idx)
    rng = np.random.default_rng(13)
    w = rng.random(n)
    w /= w.sum()
    sm, _, _ = mat.standardize(w, center, scale)
    d, v = rng.random(n), rng.standard_normal(n)
    rows = np.sort(rng.choice(n, n // 2, replace=False))
    for r in (None, rows):
        H, g = sm.sandwich_and_transpose_matvec(d, v, r)
        assert nat_err(H, sm.sandwich(d, r)) < 1e-12
        assert rel_err(g, sm.transpose_matvec(v, r)) < 1e-12
        A = sm.toarray()
        _, gr = _ld_ref(A, d, v, r)
        assert _g_err(g, gr, A, v, r) < 1e-10


@pytest.mark.parametrize("width,kind", [(128, "i8"), (97, "i8"), (128, "co"), (97, "co"), (256, "i8_wide")])
def test_centered_kernels_direct(width, kind):
    """The centred forms of the entry points: (X - 1 c)' D (X - 1 c), X' d (K1c) and (X - 1 c)' v."""
    from tabmat_amd import _device as D
    from tabmat_amd.ext import dense as xd
    from tabmat_amd.ext._types import DenseDev

    rng = np.random.default_rng(width)
    n = 9_000
    X = rng.standard_normal((n, width)) + 10.0
    c = X.mean(axis=0)
    d, v = rng.random(n), rng.standard_normal(n)
    blk = DenseDev.from_host(np.ascontiguousarray(X))
    cd = D.to_dev(c, torch.float64).contiguous()
    dd, vd = D.to_dev(d, torch.float64), D.to_dev(v, torch.float64)
    cmax = torch.tensor(np.abs(X - c).max(axis=0), device="cuda").contiguous()
    hist = None
    if kind == "i8":
        from tabmat_amd._lib import lib

        hist = torch.zeros(int(lib().tm_dense_sandwich_i8_history_words()), dtype=torch.int32, device="cuda")
    out, cs_, xtv = xd.dense_sandwich_xtv(blk, dd, vd, kind, None if kind == "co" else cmax, history=hist,
                                          center=cd, want_colsum=kind == "co")
    Hr, gr = _ld_ref(X - c, d, v)
    assert nat_err(out.cpu().numpy(), Hr) < 1e-10
    assert _g_err(xtv.cpu().numpy(), gr, X - c, v) < 1e-12
    if kind == "co":
        _, dr = _ld_ref(X - c, d, d)
        assert _g_err(cs_.cpu().numpy(), dr, X - c, d) < 1e-12
    else:
        assert cs_ is None
