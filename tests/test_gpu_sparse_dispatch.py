"""-m gpu: WHICH tm_* entry points the products of ONE sparse block reach, in what order and with which scalar
arguments, pinned against tests/golden/sparse_dispatch.json -- the layer below tests/test_gpu_sandwich_dispatch.py:
SparseMatrix's choice among the self-sandwich kernels (block list, chunked, direct, pair stream, row list, narrow
selection, deterministic, row parts, generic), among the sparse x dense kernels (entry twin, lane groups, narrow / wide
ELL, slab, column-sorted, row list, generic), and which twins to_device builds for a given dense width.

The tracer, the encoding, the layout of the golden file and the recorder are those of test_gpu_sandwich_dispatch.py
(imported, see its docstring).  What to_device built is stored the same way: a call record whose "launches" are the
names of the twins that exist afterwards ("twin ent", "twin slab", ...), seen through the builders in ext/_types.py.

A case uses the public API and the module constants other tests patch; where a route cannot be reached at a small
size it overrides ONE method of the block on the instance (`_narrow_pays`, `_ent`, `_lg`) and says so in its docstring.

Re-recording (after a change that is MEANT to move launches):
    python tests/test_gpu_sparse_dispatch.py --commit <hash of the commit recorded> [--out FILE]"""
import os
import sys

import numpy as np
import pytest
from scipy import sparse as sps

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import test_gpu_sandwich_dispatch as base  # noqa: E402
from _gpu_util import cross_err  # noqa: E402
from test_gpu_sandwich_dispatch import F32_TOL, F64_TOL, _host, _sand, _sorted_choice  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "sparse_dispatch.json")
N = 3001


def _sp(m, density, seed, n=N, dtype=np.float64):
    return sps.random(n, m, density=density, format="csc", random_state=np.random.default_rng(seed)).astype(dtype)


def _tol(dtype):
    return F64_TOL if dtype == np.float64 else F32_TOL


# ---- self sandwich ---------------------------------------------------------------------------------------------
def _self_plain(t, dtype):
    import tabmat_amd as tm

    d = np.random.default_rng(20).random(N).astype(dtype)
    for tag, dens in (("0.1", 0.1), ("0.02", 0.02)):
        S = _sp(90, dens, 21, dtype=dtype)
        X = tm.SparseMatrix(S)
        t.call(f"90 @ {tag}: sandwich", lambda: X.sandwich(d), _sand(S.toarray(), d), _tol(dtype))


def case_self_f64(t):
    """3001 x 90 at 9 entries per row and chunk (block list) and at 1.8 (chunked); on the first: a short row list (row-
    list kernel), a long one (masked d), a column selection (full, then select) and the same selection with
    `_narrow_pays` overridden to True on the instance (CSC densify + syrk)."""
    import tabmat_amd as tm

    _self_plain(t, np.float64)
    rng = np.random.default_rng(22)
    S = _sp(90, 0.1, 21)
    E = S.toarray()
    X = tm.SparseMatrix(S)
    d = rng.random(N)
    rows3, rows70 = _sorted_choice(rng, N, N // 3), _sorted_choice(rng, N, int(0.7 * N))
    c17 = _sorted_choice(rng, 90, 17)
    t.call("90 @ 0.1: sandwich rows/3", lambda: X.sandwich(d, rows3), _sand(E, d, rows3))
    t.call("90 @ 0.1: sandwich rows70%", lambda: X.sandwich(d, rows70), _sand(E, d, rows70))
    t.call("90 @ 0.1: sandwich cols17", lambda: X.sandwich(d, cols=c17), _sand(E, d, None, c17))
    Xn = tm.SparseMatrix(S)
    Xn._narrow_pays = lambda w: True
    t.call("90 @ 0.1: sandwich cols17, narrow pays", lambda: Xn.sandwich(d, cols=c17), _sand(E, d, None, c17))
    t.call("90 @ 0.1: sandwich rows/3 cols17, narrow pays", lambda: Xn.sandwich(d, rows3, c17), _sand(E, d, rows3, c17))


def case_self_f32(t):
    """The two plain sandwiches of self_f64 in float32."""
    _self_plain(t, np.float32)


def case_self_wide(t):
    """Wide blocks: 2000 columns at 3 entries per row (direct), 5000 columns = more than 32 chunks with the pair
    stream switched off (the generic tm_sparse_sandwich_*), and a block without any stored entry (generic)."""
    import tabmat_amd as tm
    from tabmat_amd.ext import sparse as xs

    rng = np.random.default_rng(23)
    d = rng.random(N)
    S = _sp(2000, 0.001, 24)
    X = tm.SparseMatrix(S)
    rows = _sorted_choice(rng, N, N // 2)
    cols = _sorted_choice(rng, 2000, 300)
    t.call("2000 @ 0.001: sandwich", lambda: X.sandwich(d), _sand(S.toarray(), d))
    t.call("2000 @ 0.001: sandwich rows/2 cols300", lambda: X.sandwich(d, rows, cols), _sand(S.toarray(), d, rows, cols))
    with t.mp.context() as m:
        m.setattr(xs, "K2_PAIRS", "0")
        Sw = _sp(5000, 0.02, 25, n=500)
        Xw = tm.SparseMatrix(Sw)
        dw = rng.random(500)
        rw, cw = _sorted_choice(rng, 500, 100), _sorted_choice(rng, 5000, 50)
        t.call("500 x 5000 @ 0.02: sandwich", lambda: Xw.sandwich(dw), _sand(Sw.toarray(), dw))
        t.call("500 x 5000 @ 0.02: sandwich rows/5 cols50", lambda: Xw.sandwich(dw, rw, cw),
               _sand(Sw.toarray(), dw, rw, cw))
    Z = tm.SparseMatrix(sps.csc_matrix((N, 90)))
    t.call("no stored entry: sandwich", lambda: Z.sandwich(d), np.zeros((90, 90)))
    t.call("no stored entry: sandwich rows/2", lambda: Z.sandwich(d, rows), np.zeros((90, 90)))


def case_self_pairs(t):
    """3001 x 600 @ 0.05 with ext.sparse.K2_PAIRS = "1" (the cost model asks for about a million rows): the packed and
    the 16-byte record stream; a row list above 0.3 n stays on the stream as a masked d, a shorter one leaves it for
    the row-list kernel."""
    import tabmat_amd as tm
    from tabmat_amd.ext import sparse as xs

    rng = np.random.default_rng(26)
    S = _sp(600, 0.05, 27)
    E = S.toarray()
    d = rng.random(N)
    rows2, rows5 = _sorted_choice(rng, N, N // 2), _sorted_choice(rng, N, N // 5)
    cols = _sorted_choice(rng, 600, 200)
    with t.mp.context() as m:
        m.setattr(xs, "K2_PAIRS", "1")
        X = tm.SparseMatrix(S)
        t.call("packed: sandwich", lambda: X.sandwich(d), _sand(E, d))
        t.call("packed: sandwich rows/2", lambda: X.sandwich(d, rows2), _sand(E, d, rows2))
        t.call("packed: sandwich rows/5", lambda: X.sandwich(d, rows5), _sand(E, d, rows5))
        t.call("packed: sandwich cols200", lambda: X.sandwich(d, cols=cols), _sand(E, d, None, cols))
        m.setattr(xs, "K2_PAIRS_PACKED", False)
        Xu = tm.SparseMatrix(S)
        t.call("unpacked: sandwich", lambda: Xu.sandwich(d), _sand(E, d))
        t.call("unpacked: sandwich rows/2", lambda: Xu.sandwich(d, rows2), _sand(E, d, rows2))


def case_self_deterministic(t):
    """categorical_matrix.DETERMINISTIC: column panels written out densely, each through the entry-list kernel."""
    import tabmat_amd as tm
    import tabmat_amd.categorical_matrix as cmod

    rng = np.random.default_rng(28)
    d = rng.random(N)
    rows = _sorted_choice(rng, N, N // 3)
    c40 = _sorted_choice(rng, 90, 40)
    rep = c40.copy()
    rep[7] = rep[6]                     # (one column id twice)
    with t.mp.context() as m:
        m.setattr(cmod, "DETERMINISTIC", True)
        for tag, dens in (("0.1", 0.1), ("0.02", 0.02)):
            S = _sp(90, dens, 21)
            E = S.toarray()
            X = tm.SparseMatrix(S)
            t.call(f"90 @ {tag}: sandwich", lambda: X.sandwich(d), _sand(E, d))
            t.call(f"90 @ {tag}: sandwich rows/3", lambda: X.sandwich(d, rows), _sand(E, d, rows))
            t.call(f"90 @ {tag}: sandwich cols40", lambda: X.sandwich(d, cols=c40), _sand(E, d, None, c40))
            t.call(f"90 @ {tag}: sandwich cols40, one repeated", lambda: X.sandwich(d, cols=rep),
                   _sand(E, d, None, rep))


def case_self_row_parts(t):
    """sparse_matrix.PART_NNZ at a third of the nonzeros: sandwich and sandwich_diag as sums over row parts."""
    import tabmat_amd as tm
    import tabmat_amd.sparse_matrix as spm

    rng = np.random.default_rng(29)
    S = _sp(90, 0.1, 21)
    E = S.toarray()
    d = rng.random(N)
    first = _sorted_choice(rng, N // 5, N // 20)          # (leaves the later parts without a row)
    with t.mp.context() as m:
        m.setattr(spm, "PART_NNZ", S.nnz // 3)
        X = tm.SparseMatrix(S)
        assert X._row_parts() is not None and len(X._row_parts()) >= 3
        t.call("sandwich", lambda: X.sandwich(d), _sand(E, d))
        t.call("sandwich rows in the first part", lambda: X.sandwich(d, first), _sand(E, d, first))
        t.call("sandwich_diag", lambda: X.sandwich_diag(d))
        t.call("sandwich_diag rows in the first part", lambda: X.sandwich_diag(d, first))


# ---- sparse x dense --------------------------------------------------------------------------------------------
def _cross(t, label, sm, dm, S, B, d, rows=None, L_cols=None, R_cols=None, tol=F64_TOL):
    """Trace sm._cross_sandwich(dm, ...) twice; each result against the float64 image at the natural scale of a cross
    term (cross_err, the rectangular nat_err)."""
    S64, B64, d64 = S.astype(np.float64), np.asarray(B, dtype=np.float64), np.asarray(d, dtype=np.float64)
    r = slice(None) if rows is None else np.asarray(rows, dtype=np.int64)
    want = np.asarray((S64.tocsr()[r].T @ (d64[r, None] * B64[r])))
    if L_cols is not None:
        want = want[np.asarray(L_cols, dtype=np.int64)]
    if R_cols is not None:
        want = want[:, np.asarray(R_cols, dtype=np.int64)]

    def fn():
        res = sm._cross_sandwich(dm, d, rows, L_cols, R_cols)
        err = cross_err(_host(res), want, d64, S64, B64, rows, L_cols, R_cols)
        assert err < tol, (label, err)
        return res

    t.call(label, fn)


def case_cross_routes(t):
    """SparseMatrix._cross_sandwich with a DenseMatrix: by the operand's width and order, the block's density and the
    row list.  No override."""
    import tabmat_amd as tm
    import tabmat_amd.dense_matrix as dmod

    rng = np.random.default_rng(30)
    S = _sp(90, 0.1, 21)
    sm = tm.SparseMatrix(S)
    d = rng.random(N)
    B100, B40, B101 = (rng.standard_normal((N, k)) for k in (100, 40, 101))
    d100, d40, d101 = tm.DenseMatrix(B100), tm.DenseMatrix(B40), tm.DenseMatrix(B101)
    rows5, rows2 = _sorted_choice(rng, N, N // 5), _sorted_choice(rng, N, N // 2)
    lc, rc = _sorted_choice(rng, 90, 30), _sorted_choice(rng, 100, 25)
    _cross(t, "B 100 columns", sm, d100, S, B100, d)
    _cross(t, "B 100 columns, L_cols R_cols", sm, d100, S, B100, d, None, lc, rc)
    _cross(t, "B 100 columns, rows/5", sm, d100, S, B100, d, rows5)
    _cross(t, "B 100 columns, rows/5 L_cols R_cols", sm, d100, S, B100, d, rows5, lc, rc)
    _cross(t, "B 100 columns, rows/2", sm, d100, S, B100, d, rows2)
    _cross(t, "B 40 columns", sm, d40, S, B40, d)
    _cross(t, "B 40 columns, rows/2", sm, d40, S, B40, d, rows2)
    _cross(t, "B 101 columns", sm, d101, S, B101, d)
    Sw = _sp(1500, 0.003, 31)
    assert Sw.nnz <= 6 * N
    sw = tm.SparseMatrix(Sw)
    _cross(t, "1500 @ 0.003, B 100 columns", sw, d100, Sw, B100, d)
    _cross(t, "1500 @ 0.003, B 100 columns, rows/2 R_cols", sw, d100, Sw, B100, d, rows2, None, rc)
    _cross(t, "1500 @ 0.003, B 101 columns", sw, d101, Sw, B101, d)
    with t.mp.context() as m:
        m.setattr(dmod, "ROW_MAJOR_TWIN", False)
        BF = np.asfortranarray(B100)
        _cross(t, "B 100 columns F-ordered, no row-major twin", tm.SparseMatrix(S), tm.DenseMatrix(BF), S, BF, d)
    # one inf in a row the list leaves out: a masked d would leak inf * 0, the generic restricted kernel runs
    Si = S.tolil(copy=True)
    Si[int(np.setdiff1d(np.arange(N), rows2)[0]), 5] = np.inf
    Si = Si.tocsc()
    _cross(t, "block with one inf, rows/2", tm.SparseMatrix(Si), d100, Si, B100, d, rows2)
    _cross(t, "block with one inf, rows/2 L_cols R_cols", tm.SparseMatrix(Si), d100, Si, B100, d, rows2, lc, rc)


def case_cross_fallbacks(t):
    """What runs when the entry twin is refused (it never is below about 4M padded slots): `_ent` overridden on the
    instance to return None -> the lane-group stream (SlabLg.from_csr accepts every small block); `_lg` overridden as
    well -> the wide ELL twin (design of test_csr_dense_sandwich_wide_ell) or, where that is refused too, the slab
    stream (design of test_very_sparse_block_keeps_the_compact_stream)."""
    import tabmat_amd as tm

    rng = np.random.default_rng(32)
    S = _sp(90, 0.1, 21)
    B = rng.standard_normal((N, 100))
    d = rng.random(N)
    dm = tm.DenseMatrix(B)
    rows2 = _sorted_choice(rng, N, N // 2)
    sm = tm.SparseMatrix(S)
    sm._ent = lambda: None
    _cross(t, "no entry twin", sm, dm, S, B, d)
    _cross(t, "no entry twin, rows/2 L_cols", sm, dm, S, B, d, rows2, _sorted_choice(rng, 90, 30))
    S1 = _sp(50, 0.05, 33, n=1000)
    B1 = rng.standard_normal((1000, 128))
    s1 = tm.SparseMatrix(S1)
    s1._ent = s1._lg = lambda: None
    _cross(t, "no entry twin, no lane groups: 1000 x 50 @ 0.05, B 128 columns", s1, tm.DenseMatrix(B1), S1, B1,
           rng.random(1000))
    n2 = 400_000
    S2 = _sp(512, 0.0005, 34, n=n2)
    B2 = rng.standard_normal((n2, 128))
    s2 = tm.SparseMatrix(S2)
    s2._ent = s2._lg = lambda: None
    assert s2._ell(wide=True) is None
    _cross(t, "no entry twin, no lane groups: 400000 x 512 @ 0.0005, B 128 columns", s2, tm.DenseMatrix(B2), S2, B2,
           rng.random(n2))


def case_cross_colsum(t):
    """The forms that return the sparse block's column sums from the same pass (colsum_box), through the public API: a
    StandardizedMatrix over [dense 100 columns, sparse]; as is (entry twin) and with `_ent` overridden on the sparse
    block to return None (lane groups)."""
    import tabmat_amd as tm

    rng = np.random.default_rng(35)
    S = _sp(90, 0.1, 21)
    A = rng.standard_normal((N, 100))
    E = np.hstack([A, S.toarray()])
    d = rng.random(N)
    shift = rng.standard_normal(190)
    rows = _sorted_choice(rng, N, N // 2)
    for tag, off in (("", False), ("no entry twin: ", True)):
        sp = tm.SparseMatrix(S)
        if off:
            sp._ent = lambda: None
        Sm = tm.StandardizedMatrix(tm.SplitMatrix([tm.DenseMatrix(A), sp]), shift)
        t.call(tag + "standardized sandwich", lambda: Sm.sandwich(d), _sand(E + shift, d))
        t.call(tag + "standardized sandwich rows/2", lambda: Sm.sandwich(d, rows), _sand(E + shift, d, rows))


# ---- twins, vectors --------------------------------------------------------------------------------------------
def _twins_built(t, label, fn, csr_of):
    """Run fn() (a to_device call) and record under `label` which twins exist afterwards, as launches "twin <name>"."""
    from tabmat_amd.ext import _types as T

    built = []
    with t.mp.context() as m:
        for cls, name in ((T.SlabEnt, "ent"), (T.SlabLg, "lg"), (T.SlabEll, "ell"), (T.SlabCsc, "slab")):
            def from_csr(*a, _fn=cls.from_csr, _name=name, **kw):
                twin = _fn(*a, **kw)
                if twin is not None:
                    built.append(_name + ("w" if getattr(twin, "wide", False) else ""))
                return twin

            m.setattr(cls, "from_csr", staticmethod(from_csr))
        fn()
    A = csr_of()
    built += ["block list"] * bool(getattr(A, "_pb", None)) + ["16-bit columns"] * (A._ind16 is not None) \
        + ["int32 columns"] * (A._ind32 is not None)
    assert label not in t.calls
    t.calls[label] = [[("twin " + b, {}) for b in built]] * 2


def _to_device(t, tag):
    import tabmat_amd as tm

    rng = np.random.default_rng(36)
    v90, v1500, w = rng.standard_normal(90), rng.standard_normal(1500), rng.standard_normal(N)
    for name, S, v in (("90 @ 0.1", _sp(90, 0.1, 21), v90), ("1500 @ 0.003", _sp(1500, 0.003, 31), v1500)):
        for width in (None, 40, 100):
            X = tm.SparseMatrix(S)
            lab = f"{tag}{name}, dense_width={width}: "
            _twins_built(t, lab + "twins", lambda: X.to_device(dense_width=width), X._dev)
            t.call(lab + "matvec", lambda: X.matvec(v))
            t.call(lab + "transpose_matvec", lambda: X.transpose_matvec(w))
            t.call(lab + "sandwich_diag", lambda: X.sandwich_diag(np.abs(w)))


def case_to_device(t):
    """to_device(dense_width=None / 40 / 100) on a block of 9 entries per row and chunk and on a wide one with 3 per
    row, then one matvec, transpose_matvec and sandwich_diag; again with ext.sparse.CSR_U16_MIN_NNZ = 0 (the 16-bit
    column twin and its kernels)."""
    from tabmat_amd.ext import sparse as xs

    _to_device(t, "")
    with t.mp.context() as m:
        m.setattr(xs, "CSR_U16_MIN_NNZ", 0)
        _to_device(t, "u16: ")


def case_vectors(t):
    """sandwich_diag, matvec and transpose_matvec of one block with rows / cols, and with a 2-D operand."""
    import tabmat_amd as tm

    rng = np.random.default_rng(37)
    S = _sp(90, 0.1, 21)
    X = tm.SparseMatrix(S)
    d = rng.random(N)
    v, w = rng.standard_normal(90), rng.standard_normal(N)
    V, W = rng.standard_normal((90, 3)), rng.standard_normal((N, 3))
    rows, cols = _sorted_choice(rng, N, N // 3), _sorted_choice(rng, 90, 17)
    t.call("sandwich_diag", lambda: X.sandwich_diag(d))
    t.call("sandwich_diag rows/3 cols17", lambda: X.sandwich_diag(d, rows, cols))
    t.call("matvec", lambda: X.matvec(v))
    t.call("matvec cols17", lambda: X.matvec(v, cols))
    t.call("matvec 2-D", lambda: X.matvec(V))
    t.call("matvec 2-D cols17", lambda: X.matvec(V, cols))
    t.call("transpose_matvec", lambda: X.transpose_matvec(w))
    t.call("transpose_matvec rows/3 cols17", lambda: X.transpose_matvec(w, rows, cols))
    t.call("transpose_matvec 2-D", lambda: X.transpose_matvec(W))
    t.call("transpose_matvec 2-D rows/3 cols17", lambda: X.transpose_matvec(W, rows, cols))


CASES = {f.__name__[5:]: f for f in (
    case_self_f64, case_self_f32, case_self_wide, case_self_pairs, case_self_deterministic, case_self_row_parts,
    case_cross_routes, case_cross_fallbacks, case_cross_colsum, case_to_device, case_vectors)}
GROUPS = {"self": ["self_f64", "self_f32", "self_wide", "self_pairs", "self_deterministic", "self_row_parts"],
          "cross": ["cross_routes", "cross_fallbacks", "cross_colsum"],
          "storage": ["to_device", "vectors"]}
assert sorted(c for g in GROUPS.values() for c in g) == sorted(CASES)


@pytest.mark.parametrize("group", list(GROUPS))
def test_sparse_dispatch(group, monkeypatch):
    for case in GROUPS[group]:
        with monkeypatch.context() as mp:       # (what a case patches is undone before the next one)
            base._check_case(case, mp, CASES, GOLDEN)


# what the record must reach (f64 forms; `*`: any run of characters).  The first group is what sandwich_dispatch.json
# never reaches; the second the other kernels this layer chooses among.
REACHED = ["tm_sparse_sandwich_pairs_f64", "tm_sparse_sandwich_pairs_pk_f64", "tm_csr_dense_sandwich_ellw_f64",
           "tm_csr_dense_sandwich_lg*_f64", "tm_csr_densify_cols_f64", "tm_csr_matvec_u16_f64", "tm_csr_rmatvec_u16_f64",
           "tm_csr_sandwich_diag_u16_f64",
           "tm_sparse_sandwich_blocks_*f64", "tm_sparse_sandwich_chunked_u8_f64", "tm_sparse_sandwich_chunked_rows_u8_f64",
           "tm_sparse_sandwich_direct_f64", "tm_sparse_sandwich_f64", "tm_csc_densify_cols_f64",
           "tm_csr_dense_sandwich_ent_f64", "tm_csr_dense_sandwich_ell_f64", "tm_csr_dense_sandwich_slab_f64",
           "tm_csc_dense_sandwich_sorted_f64", "tm_csr_dense_sandwich_rows_u8_f64", "tm_csr_dense_sandwich_f64",
           "tm_csr_sandwich_diag_f64", "tm_csr_matvec_f64", "tm_csr_rmatvec_f64", "tm_csr_matvec_multi_f64",
           "tm_csr_rmatvec_multi_f64"]


def test_the_record_reaches_every_sparse_entry_point():
    """From the golden file alone: every entry point of REACHED occurs in some recorded case (and the file holds
    every case), so a route that silently stops being reachable fails here when the file is recorded again."""
    import fnmatch

    gold = base._load(GOLDEN)
    assert sorted(gold["cases"]) == sorted(CASES)
    used = {i for labels in gold["cases"].values() for seqs in labels.values() for seq in seqs for i in seq}
    names = {gold["launches"][i].split(" ")[0] for i in used}
    assert len(names) > len(REACHED) // 2
    missing = [pat for pat in REACHED if not fnmatch.filter(names, pat)]
    assert not missing, missing


if __name__ == "__main__":
    base.main(sys.argv[1:], CASES, GOLDEN)
