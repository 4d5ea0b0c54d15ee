"""-m gpu: the solver-facing products -- sandwich_matvec, sandwich_diag, sandwich_and_transpose_matvec, glm_loss_grad,
their StandardizedMatrix, to_device() and row-part forms, and matvec / transpose_matvec of 2-D operands -- over the
seeded random designs of test_gpu_fuzz.py (_random_split): a net under the host composition in split_matrix.py
(which dense block the fused pass reads, the fused multi-categorical plan, the CSR column form after to_device(),
column selections as zeros in u, row parts), whose pieces depend on shapes.

Designs.  Seed s draws from default_rng(BASE + s) with n from N_ROWS; a draw with n * p > NP_CAP draws a second
design with n from (129, 1000) on the same rng (one fixed rule, no loop; the second draw is taken as it comes, at
most 1000 rows).  Every fourth seed is float32.  With
BASE = 3000 none of the 24 default seeds is degenerate (no seed skips).  Row parts run on the seeds with
seed % 6 == PARTS_RESIDUE that are a SplitMatrix holding a sparse block of at least 3000 entries: seeds 5 and 23.

References.  All long double, from the dense float64 image E of the blocks' own values (exact for float32 blocks),
in column chunks of at most CHUNK columns (row slabs of the same size for the per-row part of glm_loss_grad), so
the peak stays far below E in long double.  They are the expressions of the products' own tests, evaluated
piecewise:
    sandwich_matvec   _ref of test_gpu_sandwich_matvec.py: t = A u one column after the other (the order in which
                      the long-double matmul sums), then A' (d t) and the scale |A|' (|d| |A| |u|) chunk by chunk
    sandwich_diag     _ref of test_gpu_sandwich_diag.py chunk by chunk
    glm_loss_grad     _reference of test_gpu_glm_loss_grad.py / reference of _glm_families_ref.py called on row slabs
                      (eta, r, d and the scales t_s, r_s are per row), the loss from one more call on eta alone, and
                      grad = A' r, g_s = |A|' r_s chunk by chunk
tests/test_fuzz_products_host.py proves on the CPU that these equal the unchunked helpers bit for bit (l_s, a scale
summed slab by slab, to a few long-double ulps), that the reference rounded to float64 / float32 passes every
comparator and that injected faults do not.

Tolerances (not the fuzz's own): TOL = 1e-12 float64 / 1e-4 float32 at each entry's natural scale, an entry of
scale 0 exactly 0; 10 TOL where glm_loss_grad's d feeds sandwich_matvec and for sandwich(d) @ u; H of
sandwich_and_transpose_matvec against float64 BLAS at nat_err 1e-10 / 2e-3 while p <= 1200; StandardizedMatrix
(float64 designs) 1e-10 at the natural scale of Z = E * mult + shift.  Every check prints its error.

The resident copy is a second build of the seed's arrays, ingested with ext.sparse.CSR_U16_MIN_NNZ patched to 0 (as
tests/test_gpu_compact_csr.py does): under the cap on n * p no sparse block holds the 1e6 entries from which
to_device() drops the int32 columns by itself.  Every sparse block with stored entries is asserted to hold its 16-bit
columns only; the first build keeps its int32 columns for the other checks.  to_device() at its default threshold
on the seed's own matrix is therefore not run here (it builds the same twins and leaves the columns alone)."""
import os

import numpy as np
import pytest
import scipy.sparse as sps
import torch

import _glm_families_ref as gr
import test_gpu_glm_loss_grad as gl
import test_gpu_sandwich_diag as sd
import test_gpu_sandwich_matvec as mv
from _gpu_util import nat_err
from test_gpu_fuzz import _random_split

pytestmark = pytest.mark.gpu

LD = np.longdouble
TOL = mv.TOL
BASE = 3000
N_ROWS = (1, 7, 64, 129, 1000, 4096, 5003)
NP_CAP = 1.2e7
CHUNK = 512
SLAB = CHUNK * 4096                     # entries of one row slab
PARTS_RESIDUE = 5
CASES = int(os.environ.get("TM_FUZZ_PRODUCT_CASES", "24"))
FAMILIES = ["gaussian", "poisson", "binomial", "gamma", ("tweedie", 1.5), ("negative_binomial", 1.0),
            "inverse_gaussian"]

_SEEN = set()        # tm_* entry points reached by the seeds of this module
_FACTS = {}          # seed -> facts of its design (None: a degenerate draw)


# ---------------------------------------------------------------------------------------------------------------
# long-double references in pieces
# ---------------------------------------------------------------------------------------------------------------
class Image:
    """The dense image E (float64), or Z = E * mult + shift of a standardized matrix, served as long-double blocks."""

    def __init__(self, E, mult=None, shift=None):
        self.E = E
        self.mult = None if mult is None else np.asarray(mult, dtype=LD)
        self.shift = None if shift is None else np.asarray(shift, dtype=LD)
        self.shape = E.shape

    def block(self, rows=None, cols=None):
        """Long-double E[rows][:, cols] (column-major: columns and the rows of its transpose are contiguous)."""
        E = self.E if rows is None else self.E[np.asarray(rows, dtype=np.int64)]
        if cols is not None:
            E = E[:, np.asarray(cols, dtype=np.int64)]
        A = np.asarray(E, dtype=LD, order="F")
        c = slice(None) if cols is None else np.asarray(cols, dtype=np.int64)
        if self.mult is not None:
            A = A * self.mult[c][None, :]
        if self.shift is not None:
            A = A + self.shift[c][None, :]
        return A


def _sel(img, rows, cols):
    r = None if rows is None else np.asarray(rows, dtype=np.int64)
    c = np.arange(img.shape[1]) if cols is None else np.asarray(cols, dtype=np.int64)
    return r, c, (img.shape[0] if r is None else len(r))


def _spans(k):
    return [(q, min(k, q + CHUNK)) for q in range(0, k, CHUNK)]


def _lin(img, r, c, U):
    """(A U, |A| |U|) of A = image[r][:, c], U 1-D or 2-D: column after column, the order of the matmul's own sums."""
    U = np.asarray(U, dtype=LD)
    Ua = np.abs(U)
    m = img.shape[0] if r is None else len(r)
    T = np.zeros((m,) + U.shape[1:], dtype=LD)
    Ta = np.zeros_like(T)
    for q0, q1 in _spans(len(c)):
        A = img.block(r, c[q0:q1])
        Aa = np.abs(A)
        for q in range(q1 - q0):
            if U.ndim == 1:
                T += A[:, q] * U[q0 + q]
                Ta += Aa[:, q] * Ua[q0 + q]
            else:
                T += A[:, q, None] * U[q0 + q][None, :]
                Ta += Aa[:, q, None] * Ua[q0 + q][None, :]
    return T, Ta


def _lint(img, r, c, W, Wa):
    """(A' W, |A|' Wa) of A = image[r][:, c] chunk by chunk (every entry is one sum over the rows)."""
    W = np.asarray(W, dtype=LD)
    Wa = np.asarray(Wa, dtype=LD)
    G = np.empty((len(c),) + W.shape[1:], dtype=LD)
    S = np.empty_like(G)
    for q0, q1 in _spans(len(c)):
        A = img.block(r, c[q0:q1])
        G[q0:q1] = A.T @ W
        S[q0:q1] = np.abs(A).T @ Wa
    return G, S


def smv_ref(img, d, u, rows, cols):
    """_ref of test_gpu_sandwich_matvec.py in column chunks."""
    r, c, _ = _sel(img, rows, cols)
    d = np.asarray(d, dtype=LD)
    d = d if r is None else d[r]
    t, ta = _lin(img, r, c, u)
    return _lint(img, r, c, d * t, np.abs(d) * ta)


def diag_ref(img, d, rows, cols):
    """_ref of test_gpu_sandwich_diag.py in column chunks."""
    r, c, _ = _sel(img, rows, cols)
    d = np.asarray(d, dtype=LD)
    d = d if r is None else d[r]
    ref = np.empty(len(c), dtype=LD)
    s = np.empty(len(c), dtype=LD)
    for q0, q1 in _spans(len(c)):
        A = img.block(r, c[q0:q1])
        A2 = A * A
        ref[q0:q1] = d @ A2
        s[q0:q1] = np.abs(d) @ A2
    return ref, s


def xtv_ref(img, W, rows, cols):
    """(A' W[rows], |A|' |W[rows]|) of A = image[rows][:, cols]: transpose_matvec, W 1-D or 2-D."""
    r, c, _ = _sel(img, rows, cols)
    W = np.asarray(W, dtype=LD)
    W = W if r is None else W[r]
    return _lint(img, r, c, W, np.abs(W))


def mv_ref(img, V, cols=None):
    """(A V, |A| |V|) of A = image[:, cols]: matvec, V 1-D or 2-D over the selected columns."""
    r, c, _ = _sel(img, None, cols)
    return _lin(img, r, c, V)


def glm_helper(family):
    return gl._reference if isinstance(family, str) and family in gl.FAMILIES else gr.reference


def glm_ref(img, family, beta, y, w, off):
    """The dict of _reference (test_gpu_glm_loss_grad.py) / reference (_glm_families_ref.py) from row slabs."""
    helper = glm_helper(family)
    n, p = img.shape
    step = max(1, SLAB // max(p, 1))
    parts = []
    for a in range(0, n, step):
        sl = slice(a, min(n, a + step))
        parts.append(helper(img.block(np.arange(sl.start, sl.stop)), family, beta, y[sl],
                            None if w is None else w[sl], None if off is None else off[sl]))
    out = {k: np.concatenate([pt[k] for pt in parts]) for k in ("eta", "r", "d", "t_s", "r_s", "w")}
    out["const_d"] = parts[0]["const_d"]
    out["l_s"] = sum((pt["l_s"] for pt in parts), LD(0))
    # the loss as ONE sum over all rows, as the helper forms it: eta as the offset of a matrix without columns
    out["loss"] = helper(np.zeros((n, 0)), family, np.zeros(0), y, w, out["eta"])["loss"]
    out["grad"], out["g_s"] = _lint(img, None, np.arange(p), out["r"], out["r_s"])
    return out


def lin_err(got, ref, s, what=""):
    """Largest error at the natural scale, entries of scale 0 exactly 0: _err of test_gpu_sandwich_diag.py."""
    return sd._err(np.asarray(mv._host(got)).reshape(-1), np.asarray(ref).reshape(-1), np.asarray(s).reshape(-1), what)


# ---------------------------------------------------------------------------------------------------------------
# the seed's design and operands
# ---------------------------------------------------------------------------------------------------------------
def seed_dtype(seed):
    return np.float64 if seed % 4 else np.float32


def draw_design(rng, dtype):
    """(X, E) of the seed's rng, or (None, None): _random_split with n from N_ROWS, drawn again with n from
    (129, 1000) when the dense image would exceed NP_CAP entries."""
    X, E = _random_split(rng, dtype, n_choices=N_ROWS)
    if X is not None and E.shape[0] * E.shape[1] > NP_CAP:
        X, E = _random_split(rng, dtype, n_choices=(129, 1000))
    return X, E


def design_facts(X, E):
    import tabmat_amd as tm

    mats = X.matrices if isinstance(X, tm.SplitMatrix) else [X]
    idxs = X.indices if isinstance(X, tm.SplitMatrix) else [np.arange(E.shape[1])]
    sparse = [(m, ix) for m, ix in zip(mats, idxs) if isinstance(m, tm.SparseMatrix)]
    return dict(n=E.shape[0], p=E.shape[1], split=isinstance(X, tm.SplitMatrix),
                kinds=[type(m).__name__[0] + str(m.shape[1]) for m in mats],
                n_cat=sum(isinstance(m, tm.CategoricalMatrix) for m in mats),
                widest_sparse=max([m.shape[1] for m, _ in sparse], default=0),
                max_nnz=max([int(np.count_nonzero(E[:, ix])) for _, ix in sparse], default=0))      # (stored values: never 0)


def draw_operands(rng, n, p, dtype, seed):
    o = {}
    d = rng.random(n).astype(dtype)
    d[rng.random(n) < 0.1] = 0.0
    o["d"] = d
    o["u"] = rng.standard_normal(p).astype(dtype)
    o["v"] = rng.standard_normal(n).astype(dtype)
    o["rows_sorted"] = np.sort(rng.choice(n, size=max(1, n // 2), replace=False))
    o["rows_rep"] = rng.choice(n, size=max(1, n // 2), replace=True)[::-1].copy()
    o["cols_sub"] = np.sort(rng.choice(p, size=max(1, (2 * p) // 3), replace=False))
    o["cols_few"] = np.sort(rng.choice(p, size=max(1, p // 5), replace=False))
    o["d_diag"] = sd._weights(rng, n, dtype, signed=True) if seed % 2 else d
    o["V"] = rng.standard_normal((p, 3)).astype(dtype)
    o["W"] = rng.standard_normal((n, 3)).astype(dtype)
    return o


def draw_glm(rng, A64, family, dtype, seed, scale=None):
    """(beta, y, weights or None, offset or None) as _problem of test_gpu_glm_loss_grad.py draws them: beta =
    0.3 N(0, 1) / sqrt(p) (over `scale`, the columns' magnitude, for a standardized image), y from the family at the
    true eta, weights with 10 % zeros unless seed % 3 == 0, an offset on odd seeds.  A64(beta): the float64 A beta."""
    n, p = A64.shape
    beta = 0.3 * rng.standard_normal(p) / np.sqrt(max(p, 1))
    if scale is not None:
        beta = beta / scale
    beta = beta.astype(dtype)
    off = (0.2 * rng.standard_normal(n)).astype(dtype) if seed % 2 else None
    eta = A64 @ beta.astype(np.float64) + (0.0 if off is None else off.astype(np.float64))
    if isinstance(family, str) and family in gl.FAMILIES:
        y = gl._draw_y(rng, family, eta)
    else:
        y = gr.draw_y(rng, family, eta)
    y = y.astype(dtype)
    w = None
    if seed % 3 != 0:
        w = (rng.random(n) + 0.1).astype(dtype)
        w[rng.random(n) < 0.1] = 0
    return beta, y, w, off


RESTRICTIONS = [("none", "none"), ("rows_sorted", "cols_sub"), ("rows_rep", "none"), ("none", "cols_few")]


def _pick(o, name):
    return None if name == "none" else o[name]


# ---------------------------------------------------------------------------------------------------------------
# the checks
# ---------------------------------------------------------------------------------------------------------------
class _Run:
    """One seed: the references, computed once per (product, restriction), and the printed / asserted errors."""

    def __init__(self, seed, dtype):
        self.seed, self.dtype, self.refs, self.failed = seed, dtype, {}, []

    def ref(self, key, fn):
        if key not in self.refs:
            self.refs[key] = fn()
        return self.refs[key]

    def report(self, product, residency, what, err, tol):
        ok = err <= tol
        print(f"seed={self.seed} {np.dtype(self.dtype).name} {product} [{residency}] {what}: {err:.2e}"
              + ("" if ok else f"  ABOVE {tol:.0e}"))
        if not ok:                          # (the seed goes on: one run shows every check it misses)
            self.failed.append(f"{product} [{residency}] {what}: {err:.2e} > {tol:.0e}")


def _to(x, dev):
    if x is None or not dev:
        return x
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _check_side(run, X, g, dev, k):
    """Side, shape and dtype of a sandwich_matvec / sandwich_diag result: the dtype of sandwich(d) (@ u), which is
    float64 for a SplitMatrix and a StandardizedMatrix whatever the blocks' dtype, the block's own otherwise."""
    import tabmat_amd as tm

    if dev:
        assert isinstance(g, torch.Tensor) and g.is_cuda
    else:
        assert isinstance(g, np.ndarray)
    assert tuple(g.shape) == (k,)
    assert mv._host(g).dtype == (np.float64 if isinstance(X, (tm.SplitMatrix, tm.StandardizedMatrix)) else run.dtype)


def check_smv(run, X, img, o, rn, cn, dev, residency, tol, tag="smv", H=None):
    rows, cols = _pick(o, rn), _pick(o, cn)
    u = o["u"] if cols is None else o["u"][cols]
    g = X.sandwich_matvec(_to(o["d"], dev), _to(u, dev), rows, cols)
    _check_side(run, X, g, dev, len(u))
    g_ref, s = run.ref((tag, rn, cn), lambda: smv_ref(img, o["d"], u, rows, cols))
    run.report("sandwich_matvec", residency, f"rows={rn} cols={cn}", mv._err(g, g_ref, s), tol)
    if H is not None:                       # the same product from the sandwich itself, and its dtype
        want = H @ u
        if not dev:
            assert g.dtype == want.dtype
        run.report("sandwich_matvec", residency, "against sandwich(d) @ u", mv._err(g, np.asarray(want, dtype=LD), s),
                   10 * tol)


def check_diag(run, X, img, o, rn, cn, dev, residency, tol, dname="d_diag", tag="diag", H=None):
    rows, cols = _pick(o, rn), _pick(o, cn)
    k = img.shape[1] if cols is None else len(cols)
    g = X.sandwich_diag(_to(o[dname], dev), rows, cols)
    _check_side(run, X, g, dev, k)
    if H is not None and not dev:
        assert g.dtype == H.dtype           # the dtype of the sandwich whose diagonal it is
    ref, s = run.ref((tag, rn, cn), lambda: diag_ref(img, o[dname], rows, cols))
    what = f"rows={rn} cols={cn}"
    run.report("sandwich_diag", residency, what, sd._err(g, ref, s, f"seed {run.seed} sandwich_diag {what}"), tol)


def check_glm(run, X, family, args, ref, dev, residency, tol):
    beta, y, w, off = args
    n, p = X.shape
    loss, grad, eta, d = X.glm_loss_grad(family, _to(beta, dev), _to(y, dev), _to(w, dev), _to(off, dev))
    if dev:
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (loss, grad, eta, d))
        assert loss.ndim == 0 and loss.dtype == torch.float64
    else:
        assert isinstance(loss, float) and all(isinstance(x, np.ndarray) for x in (grad, eta, d))
    assert tuple(grad.shape) == (p,) and tuple(eta.shape) == (n,) and tuple(d.shape) == (n,)
    for x in (grad, eta, d):
        assert mv._host(x).dtype == run.dtype
    for k, v in gl._errors(ref, loss, grad, eta, d).items():
        run.report("glm_loss_grad", residency, f"{family} {k}", v, tol)
    return d


def _move_dense_off_zero(rng, X, E):
    """x -> mean + x in the dense blocks and in a copy of the image, as test_random_standardized_sandwich does."""
    import tabmat_amd as tm

    E = E.copy()
    new = []
    for mb, ix in zip(X.matrices, X.indices):
        if isinstance(mb, tm.DenseMatrix):
            mu = rng.choice([0.0, 3.0, -40.0, 300.0], size=mb.shape[1])
            A = mb.toarray() + mu[None, :]
            E[:, ix] = A
            new.append(tm.DenseMatrix(A))
        else:
            new.append(mb)
    return tm.SplitMatrix(new, [np.asarray(i) for i in X.indices]), E


def _spy_names():
    from conftest import ABI_CALLS

    return dict(ABI_CALLS)


def _run_seed(seed, monkeypatch):
    import tabmat_amd as tm

    dtype = seed_dtype(seed)
    rng = np.random.default_rng(BASE + seed)
    X, E = draw_design(rng, dtype)
    if X is None:
        _FACTS[seed] = None
        pytest.skip("degenerate draw")
    facts = _FACTS[seed] = design_facts(X, E)
    n, p = E.shape
    print(f"seed={seed} design n={n} p={p} {np.dtype(dtype).name} blocks={facts['kinds']}")
    tol = TOL[dtype]
    dev = bool(seed % 2)
    side = "device" if dev else "host"
    o = draw_operands(rng, n, p, dtype, seed)
    family = FAMILIES[seed % 7]
    glm_args = draw_glm(rng, E, family, dtype, seed)
    img = Image(E)
    run = _Run(seed, dtype)
    is_split = isinstance(X, tm.SplitMatrix)

    # sandwich_and_transpose_matvec (first: its H also serves sandwich_matvec's second comparison)
    H_full = None
    for rn, cn in RESTRICTIONS[:2]:
        rows, cols = _pick(o, rn), _pick(o, cn)
        H, g = X.sandwich_and_transpose_matvec(_to(o["d"], dev), _to(o["v"], dev), rows, cols)
        g_ref, s = run.ref(("xtv", rn, cn), lambda: xtv_ref(img, o["v"], rows, cols))
        what = f"rows={rn} cols={cn}"
        run.report("sandwich_and_transpose_matvec g", side, what, lin_err(g, g_ref, s, f"seed {seed} g {what}"), tol)
        if p <= 1200:
            H = H.toarray() if sps.issparse(H) else mv._host(H)
            Er = E if rows is None else E[np.ix_(rows, cols)]
            dr = o["d"].astype(np.float64) if rows is None else o["d"].astype(np.float64)[rows]
            want = Er.T @ (dr[:, None] * Er)
            assert H.shape == want.shape
            run.report("sandwich_and_transpose_matvec H", side, what, nat_err(H, want),
                       1e-10 if dtype == np.float64 else 2e-3)
            if rows is None:
                H_full = H
    for rn, cn in RESTRICTIONS:
        check_smv(run, X, img, o, rn, cn, dev, side, tol, H=H_full if (rn, cn) == ("none", "none") else None)
    for rn, cn in RESTRICTIONS:
        check_diag(run, X, img, o, rn, cn, dev, side, tol, H=H_full if (rn, cn) == ("none", "none") else None)
    ref_glm = glm_ref(img, family, *glm_args)
    d_glm = check_glm(run, X, family, glm_args, ref_glm, dev, side, tol)
    # d is ready for the Hessian-vector product
    hv = X.sandwich_matvec(d_glm, _to(o["u"], dev))
    g_ref, s = smv_ref(img, ref_glm["d"], o["u"], None, None)
    run.report("sandwich_matvec", side, "d of glm_loss_grad", mv._err(hv, g_ref, s), 10 * tol)

    # 2-D operands
    if facts["n_cat"] == 0:
        got = X.matvec(_to(o["V"], dev))
        ref, s = mv_ref(img, o["V"])
        assert tuple(got.shape) == (n, 3)
        run.report("matvec 2-D", side, "K=3", lin_err(got, ref, s, f"seed {seed} matvec 2-D"), tol)
        rows, cols = o["rows_sorted"], o["cols_sub"]
        got = X.transpose_matvec(_to(o["W"], dev), rows, cols)
        ref, s = xtv_ref(img, o["W"], rows, cols)
        assert tuple(got.shape) == (len(cols), 3)
        run.report("transpose_matvec 2-D", side, "K=3 rows=rows_sorted cols=cols_sub",
                   lin_err(got, ref, s, f"seed {seed} transpose_matvec 2-D"), tol)

    # the resident copy, every sparse block compacted to its 16-bit columns (as tests/test_gpu_compact_csr.py forces
    # it: by default only blocks of 1e6 entries are, which the cap on n * p keeps out of reach).  A second build of
    # the same arrays: X keeps its int32 columns for the checks that follow.
    if is_split:
        from tabmat_amd.ext import sparse as xs

        with monkeypatch.context() as mp:
            mp.setattr(xs, "CSR_U16_MIN_NNZ", 0)
            Xd, Ed = draw_design(np.random.default_rng(BASE + seed), dtype)
            assert np.array_equal(Ed, E)
            Xd = Xd.to_device()
            stored = [m._dev() for m in Xd.matrices if isinstance(m, tm.SparseMatrix) and m._dev().data.numel() > 0]
            for A in stored:
                assert A._ind32 is None and A._ind16 is not None, "the block must be compacted to its 16-bit columns"
            facts["compacted"] = len(stored)
            check_smv(run, Xd, img, o, "rows_sorted", "cols_few", dev, "to_device", tol)
            check_diag(run, Xd, img, o, "rows_sorted", "cols_few", dev, "to_device", tol)
            check_glm(run, Xd, family, glm_args, ref_glm, dev, "to_device", tol)
            for A in stored:
                assert A._ind32 is None
        for m in X.matrices:
            if isinstance(m, tm.SparseMatrix) and m._dev().data.numel() > 0:
                assert m._dev()._ind32 is not None

    # the standardized view
    if is_split and dtype == np.float64:
        Xs, Es = _move_dense_off_zero(rng, X, E)
        if seed % 3 == 0:
            w = rng.random(n) + 0.1
            w /= w.sum()
            std = Xs.standardize(w, True, True)[0]
        else:
            std = tm.StandardizedMatrix(Xs, rng.standard_normal(p) * rng.choice([0.0, 1.0, 50.0], size=p),
                                        rng.uniform(0.2, 3.0, p))
        Z = Image(Es, std.mult, std.shift)
        check_smv(run, std, Z, o, "rows_sorted", "cols_sub", dev, "standardized", 1e-10, tag="std_smv")
        check_diag(run, std, Z, o, "rows_sorted", "cols_sub", dev, "standardized", 1e-10, dname="d", tag="std_diag")
        # (beta over the columns' magnitude: eta stays where every family's response can be drawn)
        Z64 = Es * (1.0 if std.mult is None else std.mult[None, :]) + std.shift[None, :]
        args_s = draw_glm(rng, Z64, family, dtype, seed, scale=np.maximum(1.0, np.sqrt((Z64 * Z64).mean(axis=0))))
        del Z64
        check_glm(run, std, family, args_s, glm_ref(Z, family, *args_s), dev, "standardized", 1e-10)

    # row parts
    if seed % 6 == PARTS_RESIDUE and is_split and facts["max_nnz"] >= 3000:
        import tabmat_amd.sparse_matrix as spm

        monkeypatch.setattr(spm, "PART_NNZ", facts["max_nnz"] // 3)
        Xp, Ep = draw_design(np.random.default_rng(BASE + seed), dtype)         # the same arrays, built again
        assert np.array_equal(Ep, E)
        parts = Xp._parts()
        assert parts is not None
        facts["row_parts"] = len(parts)
        H, g = Xp.sandwich_and_transpose_matvec(_to(o["d"], dev), _to(o["v"], dev))
        g_ref, s = run.ref(("xtv", "none", "none"), None)
        run.report("sandwich_and_transpose_matvec g", "row parts", "unrestricted",
                   lin_err(g, g_ref, s, f"seed {seed} row parts g"), tol)
        if p <= 1200:
            want = E.T @ (o["d"].astype(np.float64)[:, None] * E)
            run.report("sandwich_and_transpose_matvec H", "row parts", "unrestricted", nat_err(mv._host(H), want),
                       1e-10 if dtype == np.float64 else 2e-3)
        check_smv(run, Xp, img, o, "none", "none", dev, "row parts", tol)
        check_diag(run, Xp, img, o, "none", "none", dev, "row parts", tol)
        check_glm(run, Xp, family, glm_args, ref_glm, dev, "row parts", tol)
    assert not run.failed, f"seed {seed}: " + "; ".join(run.failed)


@pytest.mark.parametrize("seed", range(CASES))
def test_random_products(seed, monkeypatch):
    before = _spy_names()
    try:
        _run_seed(seed, monkeypatch)
    finally:
        after = _spy_names()
        _SEEN.update(k for k, v in after.items() if v > before.get(k, 0))


def test_zz_dispatch_span(request):
    """The fixed seeds land on both sides of the dispatch: the entry points below were reached by this module's own
    seeds, and the designs held several categoricals, a wide sparse block and very few rows."""
    if request.config.option.keyword or CASES < 24 or len(_FACTS) < CASES:
        pytest.skip("partial run")
    skipped = sorted(s for s, f in _FACTS.items() if f is None)
    assert len(skipped) <= 2, skipped
    facts = [f for f in _FACTS.values() if f is not None]
    print("entry points reached:", " ".join(sorted(_SEEN)))
    missing = [f"tm_{name}_{suf}" for name in ("dense_sandwich_matvec", "dense_sandwich_diag", "csr_sandwich_diag",
                                               "csr_sandwich_diag_u16")
               for suf in ("f64", "f32") if f"tm_{name}_{suf}" not in _SEEN]
    for stem in ("tm_dense_glm_loss_grad_", "tm_glm_rowfn_", "tm_glm_rowfn_p_", "tm_dense_glm_loss_grad_p_"):
        if not any(s in _SEEN for s in (stem + "f64", stem + "f32")):
            missing.append(stem + "*")
    assert not missing, f"never reached by the {CASES} seeds: {missing}"
    assert any(f["n_cat"] >= 2 for f in facts)
    assert any(f["widest_sparse"] > 512 for f in facts)
    assert any(f["n"] <= 7 for f in facts)
    assert any("row_parts" in f for f in facts), "no seed ran in row parts"
    assert any(f.get("compacted", 0) > 0 for f in facts), "no resident copy held a compacted sparse block"
