"""The fused categorical cross terms (csrc/cat_multi.hip), launcher by launcher and rung by rung: the five ext.split
wrappers called directly at the smallest shapes at which each template rung, each kernel and each launcher condition
is reached (derived from the launchers' own conditions; named at every case).

Every case compares against a float64 numpy reference, onehot(cats)' diag(d) X, with the measure and the tolerances
of tests/test_gpu_kernels.py test_multi_cat_dense_wide_kernel (cross_err < 1e-10 for f64, < 1e-4 for f32), and is run
once more with integer-valued inputs (d in {0..3}, values in {-4..4}, at most 10 000 rows): every partial sum is then
an integer below 2^24, exact in both dtypes, and the result must EQUAL the reference whatever order the LDS atomics
land in.  Missing codes (-1), drop_first on every second categorical and rows with d == 0 throughout; those rows hold
inf wherever the kernel masks them (all but the two narrow dense kernels, which multiply d == 0 into the operand as the
reference loop does and so get finite values there).

The cases are small (the whole module takes a few seconds) and many, so they run as loops inside two tests -- one per
kernel the `_catsparse_kernel` fixture forces for the entry twin -- and every failing case is reported by name."""
import functools

import numpy as np
import pytest
from scipy import sparse as sps

from _gpu_util import cross_err
from test_k3_ent import _catsparse_kernel  # noqa: F401  (fixture: forces the staged / the gather kernel)

pytestmark = pytest.mark.gpu
F64_TOL = 1e-10
DTYPES = [np.float64, np.float32]
TM_EINVAL, TM_EUNSUPPORTED = -1, -3


def _split(total, k):
    """k column counts that add up to `total` (unequal where they can be)."""
    base = [total // k] * k
    for i in range(total - sum(base)):
        base[i] += 1
    if k > 1 and base[0] > 1 and total % 2 == 0:
        base[0] -= 1
        base[-1] += 1
    return base


def _inputs(seed, n, ncols, integer, dtype):
    """d and the categoricals [(codes, n_cols, drop_first)]: 5 % missing codes, every second one drops its first level,
    a fifth of the rows (at least) with d == 0."""
    rng = np.random.default_rng(seed)
    d = (rng.integers(0, 4, n) if integer else rng.random(n)).astype(dtype)
    d[::5] = 0
    cats = []
    for ci, ncol in enumerate(ncols):
        drop = bool(ci % 2)
        codes = rng.integers(0, ncol + int(drop), n).astype(np.int32)
        codes[rng.random(n) < 0.05] = -1
        cats.append((codes, ncol, drop))
    return rng, d, cats


def _dense(rng, n, m, d, integer, dtype, inf_rows):
    """(operand, with inf in the rows of zero weight if `inf_rows`; the same with those rows zeroed in float64)."""
    X = (rng.integers(-4, 5, (n, m)) if integer else rng.standard_normal((n, m))).astype(dtype)
    Xc = X.astype(np.float64)
    Xc[d == 0] = 0.0
    if inf_rows:
        X[d == 0, 0] = np.inf
    return X, Xc


@functools.lru_cache(maxsize=None)
def _pattern(n, m, density, seed):
    S = sps.random(n, m, density=density, format="csr", random_state=np.random.default_rng(seed), dtype=np.float64)
    S.sort_indices()
    return S


def _sparse(rng, n, m, density, d, integer, dtype):
    """CSR operand (every entry of a row with zero weight is inf) and its float64 copy with those rows zeroed."""
    S = _pattern(n, m, density, 1000 * m + n).copy()
    nnz = S.data.shape[0]
    S.data = (rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz) if integer
              else rng.standard_normal(nnz)).astype(np.float64)
    S = S.astype(dtype)
    Sc = S.astype(np.float64)
    dead = np.repeat(d == 0, np.diff(S.indptr))
    Sc.data[dead] = 0.0
    S.data[dead] = np.inf
    return S, Sc


def _reference(cats, d, Xc, rows=None):
    """onehot(cats)' diag(d) X over the rows of the list (a repeated row counts per occurrence), float64."""
    n = d.shape[0]
    r = np.arange(n) if rows is None else np.asarray(rows, dtype=np.int64)
    dX = sps.diags(d.astype(np.float64)[r]) @ Xc[r]
    out = []
    for codes, ncol, drop in cats:
        col = codes.astype(np.int64)[r] - int(drop)
        ok = col >= 0
        oh = sps.csr_matrix((np.ones(int(ok.sum())), (np.nonzero(ok)[0], col[ok])), shape=(r.shape[0], ncol))
        ref = oh.T @ dX
        out.append(ref.toarray() if sps.issparse(ref) else np.asarray(ref))
    return out


def _check(got, cats, d, Xc, integer, dtype, rows=None):
    refs = _reference(cats, d, Xc, rows)
    assert got.shape == (sum(c[1] for c in cats), Xc.shape[1])
    off = 0
    for (codes, ncol, drop), ref in zip(cats, refs):
        blk = got[off:off + ncol]
        off += ncol
        if integer:
            assert np.abs(ref).max(initial=0.0) < 2**24
            assert np.array_equal(blk, ref)
        else:
            err = cross_err(blk, ref, d, ("cat", codes, ncol, drop), Xc, rows)
            print(f"cross_err {err:.3e}")
            assert err < (F64_TOL if dtype == np.float64 else 1e-4)


def _dev_cats(cats):
    from tabmat_amd import _device as D

    return [(D.to_dev(c), ncol, drop) for c, ncol, drop in cats]


def _row_list(rng, n, n_sel):
    rows = rng.integers(0, n, n_sel).astype(np.int32)
    rows[1::7] = rows[0]                      # repeats
    return rows


# ------------------------------------------------------------------------------------------ dense
def _run_dense(n, m, ncols, order, dtype, n_sel=None, wide=True):
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import DenseDev

    for integer in (False, True):
        rng, d, cats = _inputs(n + 31 * m + len(ncols), n, ncols, integer, dtype)
        X, Xc = _dense(rng, n, m, d, integer, dtype, inf_rows=wide)
        dm = DenseDev.from_host(np.asfortranarray(X) if order == "F" else X)
        dcats = _dev_cats(cats)
        assert xsplit.multi_cat_dense_wide_ok(dcats, dm) == wide
        rows = None if n_sel is None else _row_list(rng, n, n_sel)
        got = D.to_host(xsplit.multi_cat_dense_sandwich(dcats, D.to_dev(d), dm,
                                                        None if rows is None else D.idx_dev(rows)))
        _check(got, cats, d, Xc, integer, dtype, rows)


def _small_ncols(n_cats):
    return [3 + (5 * c) % 7 for c in range(n_cats)]


def _wide_dense(n_cats, form, n_iter, dtype):
    """multi_cat_dense_wide_kernel<F, 1..8>, plain and row-list form (rows with repeats); 33 rows are one 32-row wave
    step plus one row, 4097 rows two workgroup ranges (at least 4096 rows each); 34 columns are two 32-column parts,
    the second nearly empty."""
    if form == "rows":
        _run_dense(1500, 34, _small_ncols(n_cats), "C", dtype, n_sel=n_iter)
    else:
        _run_dense(n_iter, 34, _small_ncols(n_cats), "C", dtype)


# (m, column counts): TJ = the power of two that covers m (1 .. 64); NC = 1 .. 4 and the generic 0 (5 and 16
# categoricals).  The C-ordered operands miss the wide path through their odd width, or -- m = 2 -- through more than
# 8 categoricals.
NARROW = [(1, [4]), (2, [3] * 16), (3, [5, 3]), (5, [2, 6, 3]), (9, [4, 2, 3, 5]), (17, [3, 2, 4, 2, 5]), (33, [6]),
          (33, [2, 3] * 8)]


def _seventeen_categoricals_are_refused():
    from tabmat_amd import _device as D
    from tabmat_amd._lib import TabmatHipError
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import DenseDev

    rng, d, cats = _inputs(17, 64, [2] * 17, False, np.float64)
    dm = DenseDev.from_host(rng.standard_normal((64, 3)))
    with pytest.raises(TabmatHipError, match=rf"code {TM_EINVAL}: multi-cat call supports 1\.\.16 categoricals, got 17"):
        xsplit.multi_cat_dense_sandwich(_dev_cats(cats), D.to_dev(d), dm)


def _dense_cases():
    cases = []
    for dtype in DTYPES:
        dn = np.dtype(dtype).name
        for n_cats in range(1, 9):
            for form in ("plain", "rows"):
                for n_iter in (33, 4097):
                    cases.append((f"wide dense {n_cats} cats {form} n={n_iter} {dn}",
                                  lambda a=(n_cats, form, n_iter, dtype): _wide_dense(*a)))
        for order in ("C", "F"):
            # multi_cat_dense_c_kernel<F, TJ, NC> and multi_cat_dense_f_kernel<F, TJ>, every TJ and every NC
            for m, ncols in NARROW:
                cases.append((f"narrow dense m={m} {len(ncols)} cats {order} {dn}",
                              lambda a=(203, m, ncols, order, dtype): _run_dense(*a, wide=False)))
            # 3 000 stacked levels against 9 columns: the LDS bound gives TJ = 4 (8 B x 3 000 x 4 = 96 000 <= 128 KB
            # < x 8) and three column parts; 4097 rows are two workgroup ranges
            cases.append((f"narrow dense 3000 levels {order} {dn}",
                          lambda a=(4097, 9, [1400, 1600], order, dtype): _run_dense(*a, wide=False)))
    # 300 stacked levels in f64: a tile of 76 800 B, above the 64 KB from which the launcher takes 8 waves
    cases.append(("wide dense 300 levels float64", lambda: _run_dense(4097, 34, [149, 151], "C", np.float64)))
    cases.append(("17 categoricals are refused", _seventeen_categoricals_are_refused))
    return cases


# ------------------------------------------------------------------------------------------ slab form
def _run_slab(n, m, density, ncols, dtype):
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import CsrDev, SlabCsc

    for integer in (False, True):
        rng, d, cats = _inputs(n + 31 * m + len(ncols), n, ncols, integer, dtype)
        S, Sc = _sparse(rng, n, m, density, d, integer, dtype)
        slab = SlabCsc.from_csr(CsrDev.from_scipy(S))
        got = D.to_host(xsplit.multi_cat_sparse_sandwich(_dev_cats(cats), D.to_dev(d), slab))
        _check(got, cats, d, Sc, integer, dtype)


def _slab_tile_limit():
    """496 stacked levels are the last that fit the 128 KB tile (8 B x 496 x 33 = 130 944); 497 are refused."""
    from tabmat_amd import _device as D
    from tabmat_amd._lib import TabmatHipError
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import CsrDev, SlabCsc

    _run_slab(300, 40, 0.2, _split(496, 2), np.float64)
    rng, d, cats = _inputs(497, 300, _split(497, 2), False, np.float64)
    S, _ = _sparse(rng, 300, 40, 0.2, d, False, np.float64)
    slab = SlabCsc.from_csr(CsrDev.from_scipy(S))
    with pytest.raises(TabmatHipError,
                       match=rf"code {TM_EUNSUPPORTED}: multi_cat_sparse: 497 stacked categories exceed the LDS tile"):
        xsplit.multi_cat_sparse_sandwich(_dev_cats(cats), D.to_dev(d), slab)


# ------------------------------------------------------------------------------------------ row list
def _row_list_case(n_cats, dtype):
    """multi_cat_sparse_rows_kernel<F, uint8_t>: 2 049 selected rows with repeats are two workgroup ranges (at least
    2 048 rows each), 140 columns two 128-column chunks whose last 32-column group holds 12 columns.  (The int32-index
    entry: tests/test_gpu_abi_dark_corners.py.)"""
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import CsrDev

    n, m = 1500, 140
    for integer in (False, True):
        rng, d, cats = _inputs(n + 31 * m + n_cats, n, _small_ncols(n_cats), integer, dtype)
        S, Sc = _sparse(rng, n, m, 0.1, d, integer, dtype)
        rows = _row_list(rng, n, 2049)
        got = D.to_host(xsplit.multi_cat_sparse_sandwich_rows(_dev_cats(cats), D.to_dev(d), CsrDev.from_scipy(S),
                                                              D.idx_dev(rows)))
        _check(got, cats, d, Sc, integer, dtype, rows)


def _slab_and_row_list_cases():
    cases = []
    for dtype in DTYPES:
        dn = np.dtype(dtype).name
        # multi_cat_sparse_pf_kernel<F, 1..8>; 9 and 16 categoricals: the generic kernel, staged.  300 rows are two
        # 128-row slabs and a ragged third, 40 columns a full 32-column group and a partly filled one.
        for n_cats in list(range(1, 9)) + [9, 16]:
            cases.append((f"slab {n_cats} cats {dn}", lambda a=(300, 40, 0.2, _small_ncols(n_cats), dtype): _run_slab(*a)))
        # Three categoricals of 160 levels: the tile is 8 B x 480 x 33 = 126 720 B, staging d and the codes of 16 waves
        # would add 40 960 B (f32: 32 768 B) -- above 150 KB, so the generic kernel runs without its staging.
        cases.append((f"slab unstaged {dn}", lambda a=(300, 40, 0.2, [160, 160, 160], dtype): _run_slab(*a)))
        # One 32-column group at density 0.3: a (slab, group) block holds ~1 200 entries, beyond the 256-entry prefetch
        # window of the pf kernel.
        cases.append((f"slab long blocks {dn}", lambda a=(300, 32, 0.3, [5, 4, 6], dtype): _run_slab(*a)))
        for n_cats in (1, 16):
            cases.append((f"row list {n_cats} cats {dn}", lambda a=(n_cats, dtype): _row_list_case(*a)))
    cases.append(("slab tile limit 496 / 497 levels", _slab_tile_limit))
    return cases


# ------------------------------------------------------------------------------------------ entry twin
def _entry_twin(n_cats, packed, dtype):
    """multi_cat_sparse_ent_kernel<F, 1..8> and multi_cat_sparse_ent_staged_kernel<F, 1..8, false> / <F, 1..3, true>
    (one packed code word per row).  40 columns are three 16-column groups: the second pair of groups has no second
    group; 300 rows are four 64-row slabs and a ragged fifth."""
    from tabmat_amd import _device as D
    from tabmat_amd.ext import split as xsplit
    from tabmat_amd.ext._types import CsrDev, SlabEnt

    n, m = 300, 40
    for integer in (False, True):
        rng, d, cats = _inputs(n + 31 * m + n_cats, n, _small_ncols(n_cats), integer, dtype)
        S, Sc = _sparse(rng, n, m, 0.2, d, integer, dtype)
        tw = SlabEnt.from_csr(CsrDev.from_scipy(S))
        assert (tw.mk // 16) % 2 == 1
        dcats = _dev_cats(cats)
        pk = xsplit.pack_codes(dcats) if packed else None
        assert (pk is not None) == packed
        got = D.to_host(xsplit.multi_cat_sparse_sandwich_ent(dcats, D.to_dev(d), tw, pk))
        _check(got, cats, d, Sc, integer, dtype)


def _entry_twin_cases(kernel):
    return [(f"entry twin ({kernel}) {n_cats} cats {'packed' if packed else 'codes'} {np.dtype(dtype).name}",
             lambda a=(n_cats, packed, dtype): _entry_twin(*a))
            for dtype in DTYPES
            for n_cats, packed in [(k, False) for k in range(1, 9)] + [(k, True) for k in range(1, 4)]]


# ------------------------------------------------------------------------------------------ the two tests
def _run_cases(cases):
    from tabmat_amd._lib import TabmatHipError

    failed = []
    for name, case in cases:
        try:
            case()
        except (TabmatHipError, RuntimeError) as e:
            # a failed library or HIP call (the expected refusals are caught inside their cases): nothing more is
            # launched on this device
            raise AssertionError(f"{name}: {type(e).__name__}: {e}; stopped after {len(failed)} failing cases: "
                                 + "; ".join(failed)) from e
        except Exception as e:  # noqa: BLE001  (a wrong result: every failing case is named, not only the first)
            failed.append(f"{name}: {type(e).__name__}: {str(e)[:300]}")
    assert not failed, f"{len(failed)} of {len(cases)} cases failed:\n" + "\n".join(failed)


@pytest.mark.parametrize("_catsparse_kernel", ["staged", "gather"], indirect=True)
def test_fused_cat_launchers(_catsparse_kernel):
    """The entry-twin cases under the forced kernel; the cases that kernel choice does not touch are dealt between the
    two runs: the dense launcher with "staged", the slab-form and row-list launchers with "gather"."""
    others = _dense_cases() if _catsparse_kernel == "staged" else _slab_and_row_list_cases()
    _run_cases(_entry_twin_cases(_catsparse_kernel) + others)
