"""The launchers' ROW CUTS, swept: every kernel that walks a range of rows per workgroup (or per wave) against its oracle
with the range forced long (knob 0 / the smallest legal value: ONE workgroup or slot over all rows), at the default, and
cut several times finer (4 rounds); the `*_waves` knobs at their legal extremes.  At the default launch a workgroup of
these tests' matrices sees a handful of slabs: whatever depends on the position inside a long range -- a running index,
double-buffer parity, look-ahead past the end of a stream, 32-bit offsets from the range start -- is otherwise only
exercised by the 10M-row tests on uniform data.  n = 20 011: 313 slabs of 64 rows with a ragged tail of 43.

Knobs that select an ALGORITHM (syrk_*, k2_slots, catsparse_staged) are not cuts and stay as they are.  The tolerances
are those of the comparisons these cases were taken from (named in each test)."""
import numpy as np
import pytest
import torch
from scipy import sparse as sps

from _gpu_util import cross_err, nat_err, rel_err, to_tm_block
from test_ent_stream_ranges import tune  # noqa: F401  (fixture: tm_tune_set, reset afterwards)

pytestmark = pytest.mark.gpu
N = 20_011
ROUNDS = [0, None, 4]          # one workgroup over all rows / the default / four rounds of workgroups over the chip


def _orc():
    from oracle import oracle as orc

    return orc


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("lg_rounds", ROUNDS)
def test_lg_rounds(lg_rounds, compact, dtype, tune):
    """K3's lane-group fallback (csrc/sparse_lg.hip), padded and compact stream; tests/test_lg_twin.py
    test_lg_kernel_matches_oracle: 1e-10 / 2e-4 of max|ref|."""
    import tabmat_amd as tm
    from tabmat_amd import _device as D
    from tabmat_amd.ext import sparse as xs
    from tabmat_amd.ext._types import SlabLg

    n, m, k = N, 300, 136
    rng = np.random.default_rng(n + m + k)
    S = sps.random(n, m, density=0.05, format="csc", random_state=rng, dtype=np.float64)
    S.data -= 0.5
    S = S.astype(dtype)
    B = rng.standard_normal((n, k)).astype(dtype)
    d = rng.random(n).astype(dtype)
    d[rng.integers(0, n, n // 7)] = 0
    B[d == 0] = np.inf
    sm, dm = tm.SparseMatrix(S), tm.DenseMatrix(B)
    tw = SlabLg.from_csr(sm._dev(), max_pad=None, max_extra=None)
    if compact:
        tw.compact_()
    tune(lg_rounds=lg_rounds)
    got, cs = xs.csr_dense_sandwich_lg(tw, dm._dev_c(), D.to_dev(d), want_colsum=True)
    got, cs = D.to_host(got), D.to_host(cs)
    Bz = B.copy()
    Bz[d == 0] = 0
    want = _orc().csr_dense_sandwich(sps.csr_matrix(S), Bz, d, None, None, None)
    tol = 1e-10 if dtype == np.float64 else 2e-4
    assert np.abs(got - want).max() / max(np.abs(want).max(), 1e-30) < tol
    cref = sps.csr_matrix(S).astype(np.float64).T @ d.astype(np.float64)
    assert np.abs(cs - cref).max() / np.abs(cref).max() < tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("waves", [4, 16])
@pytest.mark.parametrize("rounds", ROUNDS)
def test_catdense_rounds_and_waves(rounds, waves, dtype, tune):
    """tm_multi_cat_dense_sandwich_* on its wide-load path (csrc/cat_multi.hip multi_cat_dense_wide_kernel);
    tests/test_gpu_kernels.py test_multi_cat_dense_wide_kernel: cross_err < 1e-10 / 1e-4."""
    import tabmat_amd as tm
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit

    n, k, ncats = N, 132, (11, 3, 40)
    rng = np.random.default_rng(n + k)
    X = rng.standard_normal((n, k)).astype(dtype)
    d = rng.random(n).astype(dtype)
    d[::5] = 0
    X[::5, 0] = np.inf
    dm = tm.DenseMatrix(X)
    cats, blocks = [], []
    for ci, nc in enumerate(ncats):
        codes = rng.integers(0, nc, n).astype(np.int32)
        codes[rng.random(n) < 0.05] = -1
        drop = bool(ci % 2)
        cm = to_tm_block(("cat", codes, nc, drop), dtype)
        blocks.append((codes, cm.shape[1], drop))
        cats.append((cm._dev(), cm.shape[1], drop))
    assert xsplit.multi_cat_dense_wide_ok(cats, dm._dev())
    tune(catdense_rounds=rounds, catdense_waves=waves)
    res = D.to_host(xsplit.multi_cat_dense_sandwich(cats, D.to_dev(d), dm._dev()))
    Xc = X.astype(np.float64).copy()
    Xc[::5, 0] = 0.0
    off = 0
    tol = 1e-10 if dtype == np.float64 else 1e-4
    for codes, ncol, drop in blocks:
        ref = _orc().sandwich_cat_dense(codes, ncol, d.astype(np.float64), Xc, None, None, drop)
        assert cross_err(res[off:off + ncol], ref, d, ("cat", codes, ncol, drop), Xc) < tol
        off += ncol
    assert off == res.shape[0]


def _cat_sparse_case(dtype, m):
    rng = np.random.default_rng(m + 77)
    S = sps.random(N, m, density=0.07, format="csc", random_state=rng, dtype=np.float64)
    S.data -= 0.4
    S = S.astype(dtype)
    d = rng.random(N).astype(dtype)
    d[rng.integers(0, N, N // 8)] = 0
    levels, drops = (13, 40, 5), (False, True, False)
    codes = [rng.integers(0, L, N).astype(np.int32) for L in levels]
    codes[2][rng.integers(0, N, N // 10)] = -1
    return S, d, levels, drops, codes


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("waves", [4, 16])
@pytest.mark.parametrize("rounds", ROUNDS)
def test_catsparse_rounds_and_waves_slab_form(rounds, waves, dtype, tune):
    """tm_multi_cat_sparse_sandwich_slab_* (csrc/cat_multi.hip run_multi_cat_sparse); tolerance of
    tests/test_gpu_row_list.py test_cat_sparse_row_list_kernel (the same reduction): 1e-10 / 3e-4 of max|ref|."""
    import tabmat_amd as tm
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit

    S, d, levels, drops, codes = _cat_sparse_case(dtype, 300)
    cats = [(D.to_dev(c), L - int(dr), dr) for c, L, dr in zip(codes, levels, drops)]
    sm = tm.SparseMatrix(S)
    tune(catsparse_rounds=rounds, catsparse_waves=waves)
    got = D.to_host(xsplit.multi_cat_sparse_sandwich(cats, D.to_dev(d), sm._slab()))
    want = np.vstack([_orc().sandwich_cat_sparse(c, L - int(dr), d.astype(np.float64),
                                                 sps.csr_matrix(S).astype(np.float64), None, None, None, dr)
                      for c, L, dr in zip(codes, levels, drops)])
    tol = 1e-10 if dtype == np.float64 else 3e-4
    assert got.shape == want.shape
    assert np.abs(got - want).max() / max(np.abs(want).max(), 1e-300) < tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("rounds", ROUNDS)
def test_catsparse_rounds_row_list_form(rounds, dtype, tune):
    """tm_multi_cat_sparse_sandwich_rows_* (csrc/cat_multi.hip run_multi_cat_sparse_rows), 12 000 selected rows with repeats;
    tests/test_gpu_row_list.py test_cat_sparse_row_list_kernel: 1e-10 / 3e-4 of max|ref|."""
    import tabmat_amd as tm
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit

    S, d, levels, drops, codes = _cat_sparse_case(dtype, 300)
    rng = np.random.default_rng(8)
    rows = rng.choice(N, 10_000, replace=False)
    rows = np.concatenate([rows, rows[:2_000]])
    cats = [(D.to_dev(c), L - int(dr), dr) for c, L, dr in zip(codes, levels, drops)]
    sm = tm.SparseMatrix(S)
    tune(catsparse_rounds=rounds)
    got = D.to_host(xsplit.multi_cat_sparse_sandwich_rows(cats, D.to_dev(d), sm._dev(), D.idx_dev(rows)))
    want = np.vstack([_orc().sandwich_cat_sparse(c, L - int(dr), d.astype(np.float64),
                                                 sps.csr_matrix(S).astype(np.float64), rows.astype(np.int32), None,
                                                 None, dr)
                      for c, L, dr in zip(codes, levels, drops)])
    tol = 1e-10 if dtype == np.float64 else 3e-4
    assert np.abs(got - want).max() / max(np.abs(want).max(), 1e-300) < tol


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("waves", [1, 16])
@pytest.mark.parametrize("rounds", ROUNDS)
def test_k2p_rounds_and_waves(rounds, waves, dtype, tune):
    """K2e, the pair-stream sparse self sandwich (csrc/sparse_pairs.hip): k2p_rounds = 0 is ONE row segment per tile
    (the workgroups then write the assembled-tile buffer themselves), k2p_waves 1 .. 16;
    tests/test_gpu_k2_pairs.py test_pairs_kernel_matches_the_oracle: nat_err < 1e-10 / 2e-5."""
    import tabmat_amd as tm
    from tabmat_amd.ext import sparse as xs

    n, m, dens = N, 2048, 0.0125
    rng = np.random.default_rng(n + m)
    S = sps.random(n, m, density=dens, format="csc", random_state=rng)
    d = rng.random(n)
    d[::5] = 0.0
    sm = tm.SparseMatrix(S.astype(dtype))
    tune(k2p_rounds=rounds, k2p_waves=waves)
    got = xs.sparse_sandwich_pairs(sm._dev(), torch.from_numpy(d.astype(dtype)).cuda()).cpu().numpy()
    S64 = S.astype(dtype).astype(np.float64)
    ref = _orc().sparse_sandwich(sps.csc_matrix(S64), sps.csr_matrix(S64), d.astype(dtype).astype(np.float64), None,
                                 None)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    assert got.shape == (m, m) and nat_err(got, ref) < tol
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("waves", [8, 12, 16])
def test_k2_waves(waves, dtype, tune):
    """K2, the chunked sparse self sandwich with 8 slots per row and chunk (csrc/sparse.hip; the knob only applies
    there: more than 4.5 nonzeros per row and 128-column chunk); tests/test_gpu_k2_blocks.py
    test_blocks_sandwich_vs_oracle: 1e-10 / 3e-4 of max|ref|."""
    import tabmat_amd as tm
    from tabmat_amd import _device as D
    from tabmat_amd.ext import sparse as xs

    n, m, dens = N, 300, 0.06
    rng = np.random.default_rng(n + m)
    S = sps.random(n, m, density=dens, format="csc", random_state=rng, dtype=np.float64)
    assert S.nnz / (n * 3) > 4.5
    S.data -= 0.5
    S = S.astype(dtype)
    d = rng.random(n).astype(dtype)
    d[rng.integers(0, n, n // 7)] = 0
    A = tm.SparseMatrix(S)._dev()
    tune(k2_waves=waves)
    got = D.to_host(xs.sparse_sandwich_chunked(A, D.to_dev(d)))
    want = _orc().sparse_sandwich(sps.csc_matrix(S).astype(np.float64), sps.csr_matrix(S).astype(np.float64),
                                  d.astype(np.float64), None, None)
    tol = 1e-10 if dtype == np.float64 else 3e-4
    assert rel_err(got, want) < tol
    assert np.array_equal(got, got.T)


@pytest.mark.parametrize("m", [128, 101])
@pytest.mark.parametrize("n", [N, 131_075])
@pytest.mark.parametrize("grid", [1, 3, 256, 0])
def test_i8_grid(grid, n, m, tune):
    """K1e, the float64 syrk on the int8 matrix cores (csrc/syrk_i8.hip): one workgroup over all 2048-row items, three,
    and one per CU; a knob below 1 is clamped to one workgroup (a grid of 0 cannot be launched).
    tests/test_gpu_syrk_i8.py test_i8_vs_oracle / test_i8_column_sums_from_the_same_pass: 1e-10 of max|ref| and of
    every entry's natural scale."""
    from tabmat_amd.ext import dense as xd
    from tabmat_amd.ext._types import DenseDev

    rng = np.random.default_rng(n * 3 + m)
    X = rng.standard_normal((n, m)) * rng.lognormal(0, 3, m)
    d = rng.random(n)
    d[::7] = 0.0
    cmax = torch.from_numpy(np.abs(X).max(axis=0)).cuda()
    tune(i8_grid=grid)
    out, cs = xd.dense_sandwich_i8(DenseDev.from_host(X), torch.from_numpy(d).cuda(), cmax, True)
    out, cs = out.cpu().numpy(), cs.cpu().numpy()
    ref = _orc().dense_sandwich(X, d, None, None)
    assert rel_err(out, ref) < 1e-10
    assert np.array_equal(out, out.T)
    scale = np.sqrt(np.outer(np.diag(ref), np.diag(ref))) + 1e-300
    assert float((np.abs(out - ref) / scale).max()) < 1e-10
    assert rel_err(cs, X.T @ d) < 1e-10
