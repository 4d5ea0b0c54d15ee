"""The slab-family sparse x dense kernels (K3: csrc/sparse_slab.hip, csrc/sparse_lg.hip, csrc/sparse_ent.hip behind
the one launcher of csrc/slab_launch.hpp), kernel by kernel and launcher condition by launcher condition: the five
ext.sparse wrappers -- csr_dense_sandwich_slab, _ell narrow and wide, _lg (padded, _xtd and compact lgc entry points)
and _ent -- called directly at the smallest shapes at which each condition of the launchers is reached (named at every
case).  The slab height R is 128 for slab and ell, 64 for ellw, lg and ent; a dense part is 64 columns for slab and
ell, 128 for the other three; a wave owns 32 sparse columns (slab, ell) or 16, a workgroup 16 waves.

Every case compares against a float64 scipy reference A' diag(d) B with the measure and the tolerances of
tests/test_gpu_cat_multi.py (cross_err < 1e-10 for f64, < 1e-4 for f32; the column sums A' d the same way against a
column of ones), and is run once more with integer-valued inputs (d in {0..3}, values in {-4..4}): every partial sum
is then an integer below 2^24 (asserted on sum |A|' d |B|; the cases of more than 10 000 rows are sparse enough for
it), exact in both dtypes, and the result must EQUAL the reference.  A fifth of the rows has d == 0.  All five kernels
mask such rows -- slab on each of its four staging paths, ell, ellw, lg (padded and compact stream, overflow entries
included) and ent send their entries to an all-zero LDS row or select a zero -- so B holds inf in those rows in every
case.

The cases are small (the whole module takes a second or two) and many, so they run as one loop inside one test and
every failing case is reported by name."""
import contextlib
import functools

import numpy as np
import pytest
from scipy import sparse as sps

from _gpu_util import cross_err

pytestmark = pytest.mark.gpu
F64_TOL = 1e-10
DTYPES = [np.float64, np.float32]
TM_EINVAL, TM_EUNSUPPORTED = -1, -3
# kind -> (slab rows R, dense columns per part W, sparse columns per wave C)
GEOM = {"slab": (128, 64, 32), "ell": (128, 64, 32), "ellw": (64, 128, 16), "lg": (64, 128, 16), "ent": (64, 128, 16)}
MASKS_ZERO_WEIGHT_ROWS = {"slab": True, "ell": True, "ellw": True, "lg": True, "ent": True}


@contextlib.contextmanager
def _tuned(**knobs):
    from tabmat_amd import _lib

    try:
        for k, v in knobs.items():
            _lib.call("tm_tune_set", k.encode(), int(v))
        yield
    finally:
        for k in knobs:
            _lib.call("tm_tune_set", k.encode(), -2**63)


@functools.lru_cache(maxsize=None)
def _pattern(n, m, density, live_cols):
    """Sparsity pattern; live_cols: only the first `live_cols` columns hold entries."""
    S = sps.random(n, live_cols or m, density=density, format="csr", random_state=np.random.default_rng(7 * n + m),
                   dtype=np.float64)
    if live_cols:
        S = sps.hstack([S, sps.csr_matrix((n, m - live_cols))], format="csr")
    S.sort_indices()
    return S


def _off_grid(x, off):
    """Device copy of the contiguous array x that starts `off` elements behind a 256-byte boundary."""
    import torch

    from tabmat_amd import _device as D

    flat = torch.empty(x.size + off, dtype=D.torch_dtype(x.dtype), device="cuda")
    view = flat[off:].view(x.shape)
    view.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    assert view.data_ptr() % 16 == (off * x.itemsize) % 16
    return view


def _inputs(n, m, k, density, integer, dtype, live_cols, inf_rows):
    rng = np.random.default_rng(n + 31 * m + 977 * k)
    d = (rng.integers(0, 4, n) if integer else rng.random(n)).astype(dtype)
    d[::5] = 0
    S = _pattern(n, m, density, live_cols).copy()
    nnz = S.data.shape[0]
    S.data = (rng.integers(1, 5, nnz) * rng.choice([-1, 1], nnz) if integer else rng.standard_normal(nnz)).astype(
        np.float64)
    S = S.astype(dtype)
    B = (rng.integers(-4, 5, (n, k)) if integer else rng.standard_normal((n, k))).astype(dtype)
    Bc = B.astype(np.float64)
    Bc[d == 0] = 0.0
    if inf_rows:
        B[d == 0] = np.inf
    return d, S, B, Bc


def _twin(kind, csr, compact):
    from tabmat_amd.ext._types import SlabCsc, SlabEll, SlabEnt, SlabLg

    if kind == "slab":
        return SlabCsc.from_csr(csr)
    if kind in ("ell", "ellw"):
        return SlabEll.from_csr(csr, wide=kind == "ellw")
    if kind == "lg":
        tw = SlabLg.from_csr(csr)
        return tw.compact_() if compact else tw
    return SlabEnt.from_csr(csr)


def _run(kind, n, m, k, density, dtype, order="C", b_off=0, d_off=0, colsum=False, unc=None, compact=False,
         live_cols=0, knobs=None):
    """One case: the random pass against the tolerance, the integer-valued pass exactly."""
    from tabmat_amd import _device as D
    from tabmat_amd.ext import sparse as xs
    from tabmat_amd.ext._types import CsrDev, DenseDev

    for integer in (False, True):
        d, S, B, Bc = _inputs(n, m, k, density, integer, dtype, live_cols, MASKS_ZERO_WEIGHT_ROWS[kind])
        tw = _twin(kind, CsrDev.from_scipy(S), compact)
        assert tw is not None
        if order == "F":
            Bd = DenseDev(_off_grid(np.ascontiguousarray(B.T), b_off), n, k, 1)
        else:
            Bd = DenseDev(_off_grid(B, b_off), n, k, 0)
        dd = _off_grid(d, d_off)
        with _tuned(**(knobs or {})):
            if kind == "slab":
                res = xs.csr_dense_sandwich_slab(tw, Bd, dd)
            elif kind in ("ell", "ellw"):
                res = xs.csr_dense_sandwich_ell(tw, Bd, dd)
            elif kind == "lg":
                res = xs.csr_dense_sandwich_lg(tw, Bd, dd, unc=unc, want_colsum=colsum)
            else:
                res = xs.csr_dense_sandwich_ent(tw, Bd, dd, want_colsum=colsum)
        out, cs = (res if colsum else (res, None))
        out = D.to_host(out)
        S64, d64 = S.astype(np.float64), d.astype(np.float64)
        ref = np.asarray((S64.T @ sps.diags(d64) @ Bc))
        cref = np.asarray(S64.T @ d64).ravel()
        assert out.shape == (m, k)
        if integer:
            assert (abs(S64).T @ (d64[:, None] * np.abs(Bc))).max(initial=0.0) < 2**24
            assert np.array_equal(out, ref)
            if colsum:
                assert np.array_equal(D.to_host(cs), cref)
        else:
            tol = F64_TOL if dtype == np.float64 else 1e-4
            err = cross_err(out, ref, d, S, Bc)
            cerr = cross_err(D.to_host(cs)[:, None], cref[:, None], d, S, np.ones((n, 1))) if colsum else 0.0
            print(f"cross_err {err:.3e} colsum {cerr:.3e}")
            assert err < tol and cerr < tol


def _case(name, *args, **kw):
    return name, lambda: _run(*args, **kw)


def _common_cases(kind, dtype):
    """The conditions all five launchers share: slab counts, dense widths, sparse widths."""
    R, W, C = GEOM[kind]
    vec = 16 // np.dtype(dtype).itemsize
    dn = np.dtype(dtype).name
    cases = []
    # slabs: one slab; R - 1, R, R + 1 rows; a ragged third slab; 256 R + 1 rows with one part and one z-layer
    # (257 slabs over 256 CUs: 2 slabs per workgroup, 129 workgroups, the last one with a single slab)
    for n in (R // 2, R - 1, R, R + 1, 2 * R + 44):
        cases.append(_case(f"{kind} n={n} {dn}", kind, n, C + 8, W, 0.2, dtype))
    cases.append(_case(f"{kind} n=256R+1 {dn}", kind, 256 * R + 1, C, W, 0.01, dtype))
    # dense width: the smallest legal one, one full part (above), a ragged second part, two full parts
    for k in (vec, W + 8, 2 * W):
        cases.append(_case(f"{kind} k={k} {dn}", kind, 2 * R + 44, C + 8, k, 0.2, dtype))
    # sparse width: one column, one group, 17 groups (nz = 2: the second workgroup has one active wave of 16)
    for m in (1, C, 16 * C + 8):
        cases.append(_case(f"{kind} m={m} {dn}", kind, 2 * R + 44, m, W, 0.2 if m <= C else 0.05, dtype))
    return cases


def _slab_cases(dtype):
    """csr_dense_gather_kernel<F, ORDER_F, VEC_OK>: the four instantiations."""
    vec = 16 // np.dtype(dtype).itemsize
    dn = np.dtype(dtype).name
    n = 300
    assert n % vec == 0 and (n + 1) % vec != 0
    return [
        _case(f"slab C r=3 (unaligned rows) {dn}", "slab", n, 40, 3, 0.2, dtype),
        _case(f"slab C B off the grid {dn}", "slab", n, 40, 64, 0.2, dtype, b_off=1),
        _case(f"slab C r=1 {dn}", "slab", n, 40, 1, 0.2, dtype),
        _case(f"slab F aligned {dn}", "slab", n, 40, 72, 0.2, dtype, order="F"),
        _case(f"slab F n % VEC != 0 {dn}", "slab", n + 1, 40, 72, 0.2, dtype, order="F"),
        _case(f"slab F d off the grid {dn}", "slab", n, 40, 64, 0.2, dtype, order="F", d_off=1),
        _case(f"slab F B off the grid {dn}", "slab", n, 40, 64, 0.2, dtype, order="F", b_off=1),
        _case(f"slab F r=1 {dn}", "slab", n, 40, 1, 0.2, dtype, order="F"),
        _case(f"slab F n=256R+1 {dn}", "slab", 256 * 128 + 1, 32, 64, 0.01, dtype, order="F"),
    ]


def _lg_cases(dtype):
    dn = np.dtype(dtype).name
    cases = []
    for compact in (False, True):
        cn = "compact" if compact else "padded"
        # (density 0.2: 13 entries per column and 64-row slab, so the overflow entries beyond the 8th run too)
        for unc in (2, 4):
            for colsum in (False, True):
                cases.append(_case(f"lg {cn} unc={unc} colsum={colsum} {dn}", "lg", 172, 24, 136, 0.2, dtype,
                                   unc=unc, colsum=colsum, compact=compact))
        # 48 columns of which 10 hold entries: the density-sorted groups 1 and 2 hold none, their slots of the
        # column-sum partials keep the launcher's zero fill
        cases.append(_case(f"lg {cn} empty groups colsum {dn}", "lg", 172, 48, 128, 0.2, dtype, colsum=True,
                           compact=compact, live_cols=10))
        # 17 groups: two z-layers, with and without the soft lockstep of the column-half workgroups
        for lockstep in (1, 0):
            cases.append(_case(f"lg {cn} nz=2 lockstep={lockstep} {dn}", "lg", 172, 264, 128, 0.05, dtype,
                               colsum=True, compact=compact, knobs={"lg_lockstep": lockstep}))
        # 257 slabs: lg_rounds = 2 gives every slab a workgroup of its own (1: 129 workgroups of two slabs)
        cases.append(_case(f"lg {cn} lg_rounds=2 {dn}", "lg", 256 * 64 + 1, 16, 128, 0.01, dtype, colsum=True,
                           compact=compact, knobs={"lg_rounds": 2}))
    return cases


def _ent_cases(dtype):
    dn = np.dtype(dtype).name
    return [
        _case(f"ent colsum {dn}", "ent", 172, 24, 136, 0.2, dtype, colsum=True),
        _case(f"ent nz=2 colsum {dn}", "ent", 172, 264, 128, 0.05, dtype, colsum=True),
        _case(f"ent ent_rounds=2 {dn}", "ent", 256 * 64 + 1, 16, 128, 0.01, dtype, colsum=True,
              knobs={"ent_rounds": 2}),
        # 0.16 entries per (slab, group) pair: most pairs are empty, slabs without a batch
        _case(f"ent mostly empty {dn}", "ent", 64 * 40 + 1, 40, 128, 0.004, dtype),
        _case(f"ent mostly empty colsum {dn}", "ent", 64 * 40 + 1, 40, 128, 0.004, dtype, colsum=True),
    ]


# ------------------------------------------------------------------------------------------ early returns
def _entry_args(kind, tw, n, m, B, r, d, out, cs, dtype):
    """(entry point, argument list) of the raw ABI call; slab as C-ordered, lg as padded _xtd."""
    from tabmat_amd import _device as D

    suf = "f64" if dtype == np.float64 else "f32"
    tail = (n, m, D.p(B), r, D.p(d))
    if kind == "slab":
        return f"tm_csr_dense_sandwich_slab_{suf}", (D.p(tw.vals), D.p(tw.koff), D.p(tw.cnt), D.p(tw.gptr), n, m,
                                                     D.p(B), r, 0, D.p(d), D.p(out), D.stream_ptr())
    if kind in ("ell", "ellw"):
        return f"tm_csr_dense_sandwich_{kind}_{suf}", (D.p(tw.vals), D.p(tw.koff), D.p(tw.gptr)) + tail + (
            D.p(out), D.stream_ptr())
    if kind == "lg":
        return f"tm_csr_dense_sandwich_lg_xtd_{suf}", (D.p(tw.vals), D.p(tw.koff), D.p(tw.xptr), D.p(tw.xvals),
                                                       D.p(tw.xkoff)) + tail + (2, D.p(out), D.p(cs), D.stream_ptr())
    if kind == "lgc":
        return f"tm_csr_dense_sandwich_lgc_{suf}", (D.p(tw.cvals), D.p(tw.cmap), D.p(tw.crec), D.p(tw.xkoff)) + tail + (
            2, D.p(out), D.p(cs), D.stream_ptr())
    return f"tm_csr_dense_sandwich_ent_{suf}", (D.p(tw.vals), D.p(tw.meta), D.p(tw.bstart)) + tail + (
        D.p(out), D.p(cs), D.stream_ptr())


def _early_returns(kind, dtype):
    """Returns taken before any launch: n = 0 zero-fills out (and colsum); a B that is misaligned or whose row length
    is no multiple of the 16-byte vector is refused by all but slab; so is an m that is no multiple of the group."""
    import torch

    from tabmat_amd import _device as D
    from tabmat_amd import _lib
    from tabmat_amd.ext._types import CsrDev

    base = "lg" if kind == "lgc" else kind
    R, W, C = GEOM[base]
    vec = 16 // np.dtype(dtype).itemsize
    n, m, k = 100, 2 * C, W
    d, S, B, _ = _inputs(n, m, k, 0.2, False, dtype, 0, False)
    tw = _twin(base, CsrDev.from_scipy(S), kind == "lgc")
    Bd, dd = D.to_dev(B), D.to_dev(d)
    nan = lambda *shape: torch.full(shape, float("nan"), dtype=D.torch_dtype(dtype), device="cuda")  # noqa: E731

    out, cs = nan(m, k), nan(m)
    fn, args = _entry_args(kind, tw, 0, m, Bd, k, dd, out, cs, dtype)
    _lib.call(fn, *args)
    assert not D.to_host(out).any()
    if base in ("lg", "ent"):
        assert not D.to_host(cs).any()
    if kind == "slab":
        return
    out.fill_(float("nan"))
    name = {"lg": "tm_csr_dense_sandwich_lg", "lgc": "tm_csr_dense_sandwich_lg"}.get(
        kind, f"tm_csr_dense_sandwich_{kind}")
    refused = rf"code {TM_EUNSUPPORTED}: {name}: B must be C-ordered with 16-byte aligned rows$"
    for what, Bx, r in (("B off the grid", _off_grid(B, 1), k), ("r % VEC != 0", Bd, k - 1), ("r < VEC", Bd, vec - 1)):
        if r == 0:
            continue
        fn, args = _entry_args(kind, tw, n, m, Bx, r, dd, out, cs, dtype)
        with pytest.raises(_lib.TabmatHipError, match=refused):
            _lib.call(fn, *args)
    if kind != "ell":
        fn, args = _entry_args(kind, tw, n, m + 1, Bd, k, dd, out, cs, dtype)
        with pytest.raises(_lib.TabmatHipError,
                           match=rf"code {TM_EINVAL}: {name}: m must be a multiple of tm_{base}_group_cols\(\)$"):
            _lib.call(fn, *args)
    assert np.isnan(D.to_host(out)).all()          # nothing was launched by the refused calls


def _early_return_cases():
    return [(f"early returns {kind} {np.dtype(dtype).name}", lambda a=(kind, dtype): _early_returns(*a))
            for kind in ("slab", "ell", "ellw", "lg", "lgc", "ent") for dtype in DTYPES]


# ------------------------------------------------------------------------------------------ the test
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


def test_k3_family():
    """Every launcher: slab counts, dense widths and sparse widths; the slab kernel's four instantiations; lg's
    unconditional positions, padded and compact streams, column sums, lockstep and rounds; ent's column sums, rounds and
    mostly empty blocks; the early returns."""
    cases = []
    for kind in GEOM:
        cases += [c for dtype in DTYPES for c in _common_cases(kind, dtype)]
    cases += [c for dtype in DTYPES for c in _slab_cases(dtype) + _lg_cases(dtype) + _ent_cases(dtype)]
    _run_cases(cases + _early_return_cases())
