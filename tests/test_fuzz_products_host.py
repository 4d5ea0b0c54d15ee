"""The comparators of tests/test_gpu_fuzz_products.py without a GPU: they are all that stands between a subtly wrong
kernel and a green run.  No device call anywhere.  On small designs built as plain arrays:
  * the chunked long-double references equal the unchunked helpers of the products' own tests bit for bit (l_s of
    glm_loss_grad, a tolerance scale summed slab by slab, to a few long-double ulps);
  * every product's reference, rounded to float64 and to float32, passes its error function at TOL;
  * a result with one fault -- an entry off by 1e-9 (float64) / 1e-2 (float32) of its natural scale, a row counted
    twice, a selected column taken from its neighbour, a drop_first categorical shifted by one level, an entry of
    natural scale 0 set to 1e-300 -- does not, for every product the fault applies to.
The last test draws the GPU module's 24 designs (the host-side constructors of tabmat_amd, nothing on a device)."""
import numpy as np
import pytest

import test_gpu_fuzz_products as fp
import test_gpu_glm_loss_grad as gl
import test_gpu_sandwich_diag as sd
import test_gpu_sandwich_matvec as mv

LD = np.longdouble
TOL = fp.TOL
BUMP = {np.float64: 1e-9, np.float32: 1e-2}


def _onehot(codes, ncat, drop, shift=0):
    """One-hot columns of `codes` (-1: missing); drop: without the first level.  shift = 1: the faulty block that
    drops the LAST level instead (every column shows the level before its own)."""
    oh = np.zeros((len(codes), ncat))
    ok = codes >= 0
    oh[np.nonzero(ok)[0], codes[ok]] = 1.0
    if not drop:
        return oh
    return oh[:, :-1] if shift else oh[:, 1:]


def _design(name, shift=0):
    """(E, index of a column of natural scale 0): dense | sparse | categorical columns in the shapes of the fuzz.
    Values are float32 numbers, so that the float32 cases see the image of float32 blocks."""
    rng = np.random.default_rng({"mixed": 1, "tiny": 2, "wide": 3}[name])
    if name == "mixed":                 # 129 rows: dense, sparse, drop_first with an unseen level, missing codes
        n = 129
        dense = rng.standard_normal((n, 17))
        sparse = rng.standard_normal((n, 40)) * (rng.random((n, 40)) < 0.05)
        c1 = rng.integers(0, 6, n)      # level 6 of 7 never occurs: an all-zero column
        c2 = np.where(rng.random(n) < 0.1, -1, rng.integers(0, 12, n))
        parts = [dense, sparse, _onehot(c1, 7, True, shift), _onehot(c2, 12, False)]
    elif name == "tiny":                # 7 rows
        n = 7
        c1 = np.array([1, 2, 0, 1, 3, 3, 1])            # level 4 of 5 never occurs
        parts = [rng.standard_normal((n, 3)), _onehot(c1, 5, True, shift)]
    else:                               # 64 rows, more columns than one chunk, an empty sparse column
        n = 64
        sparse = rng.standard_normal((n, 600)) * (rng.random((n, 600)) < 0.04)
        sparse[:, 77] = 0.0
        c1 = rng.integers(0, 4, n)      # level 4 of 5 never occurs
        parts = [rng.standard_normal((n, 11)), sparse, _onehot(c1, 5, True, shift)]
    E = np.hstack(parts).astype(np.float32).astype(np.float64)
    zero = np.nonzero(~E.any(axis=0))[0]
    return E, (int(zero[0]) if not shift else None)


DESIGNS = ["mixed", "tiny", "wide"]
GLM_FAMILIES = ["poisson", "gamma", ("tweedie", 1.5), ("negative_binomial", 1.0)]


def _operands(E, dtype, seed=0):
    n, p = E.shape
    return fp.draw_operands(np.random.default_rng(100 + seed), n, p, dtype, seed=1)


def _restrictions(o, n, p):
    return [(None, None), (o["rows_sorted"], o["cols_sub"]), (o["rows_rep"], None), (None, o["cols_few"])]


# ---------------------------------------------------------------------------------------------------------------
# chunked == unchunked
# ---------------------------------------------------------------------------------------------------------------
def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.dtype == b.dtype == LD and a.shape == b.shape and np.array_equal(a, b)


@pytest.mark.parametrize("standardized", [False, True])
@pytest.mark.parametrize("name", DESIGNS)
def test_chunked_references_are_the_helpers(name, standardized, monkeypatch):
    E, _ = _design(name)
    n, p = E.shape
    rng = np.random.default_rng(5)
    img = fp.Image(E, rng.uniform(0.2, 3.0, p), rng.standard_normal(p)) if standardized else fp.Image(E)
    A = img.block()                     # the whole long-double image, as the helpers take it
    if name != "wide":                  # several chunks and several slabs on the small designs too
        monkeypatch.setattr(fp, "CHUNK", 5)
        monkeypatch.setattr(fp, "SLAB", 3 * p)
    else:
        monkeypatch.setattr(fp, "SLAB", 20 * p)
        assert p > fp.CHUNK
    o = _operands(E, np.float64)
    for rows, cols in _restrictions(o, n, p):
        u = o["u"] if cols is None else o["u"][cols]
        for got, want in zip(fp.smv_ref(img, o["d"], u, rows, cols), mv._ref(A, o["d"], u, rows, cols)):
            assert _same(got, want)
        for got, want in zip(fp.diag_ref(img, o["d_diag"], rows, cols), sd._ref(A, o["d_diag"], rows, cols)):
            assert _same(got, want)
        r = slice(None) if rows is None else rows
        Ar = A[r] if cols is None else A[r][:, cols]
        for W in (o["v"], o["W"]):
            g, s = fp.xtv_ref(img, W, rows, cols)
            Wl = np.asarray(W, dtype=LD)[r]
            assert _same(g, Ar.T @ Wl) and _same(s, np.abs(Ar).T @ np.abs(Wl))
    for V in (o["u"], o["V"]):
        t, ta = fp.mv_ref(img, V)
        Vl = np.asarray(V, dtype=LD)
        assert _same(t, A @ Vl) and _same(ta, np.abs(A) @ np.abs(Vl))
    for k, family in enumerate(GLM_FAMILIES + ["gaussian", "binomial", "inverse_gaussian"]):
        args = fp.draw_glm(np.random.default_rng(k), np.asarray(A, dtype=np.float64), family, np.float64, seed=k + 1,
                           scale=np.maximum(1.0, np.sqrt(np.asarray(A * A, dtype=np.float64).mean(axis=0))))
        got = fp.glm_ref(img, family, *args)
        want = fp.glm_helper(family)(A, family, *args)
        assert set(got) == set(want)
        for key in want:
            if key == "const_d":
                assert got[key] == want[key]
            elif key == "l_s":
                assert abs(got[key] - want[key]) <= 8 * np.finfo(LD).eps * want[key]
            else:
                assert _same(got[key], want[key]), (family, key)


# ---------------------------------------------------------------------------------------------------------------
# the rounded reference passes, a faulty result does not
# ---------------------------------------------------------------------------------------------------------------
def _fails(err_fn, tol):
    """True when the comparator rejects: an error above tol, or its own assertion (an entry of scale 0)."""
    try:
        return not err_fn() <= tol
    except AssertionError:
        return True


def _dup(E, rows, cols, d=None):
    """The row selection with one of its rows counted once more: the first that carries weight and holds a nonzero in
    a selected column (a row that adds nothing is no fault)."""
    r = np.arange(E.shape[0]) if rows is None else np.asarray(rows)
    Er = np.abs(E[r] if cols is None else E[r][:, cols]).sum(axis=1)
    k = int(np.nonzero(Er * (1.0 if d is None else np.abs(np.asarray(d, dtype=np.float64)[r])))[0][0])
    return np.concatenate([r, r[k:k + 1]])


def _neighbour(E, rows, cols):
    """The column selection with one column replaced by its neighbour in the matrix: the first, from the middle on,
    whose neighbour is not selected itself and differs from it on the selected rows."""
    p = E.shape[1]
    c = (np.arange(p) if cols is None else np.asarray(cols)).copy()
    Er = E if rows is None else E[np.asarray(rows)]
    for q in list(range(len(c) // 2, len(c))) + list(range(len(c) // 2)):
        for j in (c[q] + 1, c[q] - 1):
            if 0 <= j < p and (cols is None or j not in c) and not np.array_equal(Er[:, j], Er[:, c[q]]):
                c[q] = j
                return c
    raise AssertionError("no column with a different neighbour")


def _linear_products(E, Es, o, rows, cols):
    """name -> (reference, scale, {fault: faulty result in long double}, error function) of the products that are
    linear in the design's columns: sandwich_matvec, sandwich_diag, g of sandwich_and_transpose_matvec and the 2-D
    matvec / transpose_matvec.  Es: the image with the drop_first categorical shifted by one level."""
    n, p = E.shape
    img, bad = fp.Image(E), fp.Image(Es)
    u = o["u"] if cols is None else o["u"][cols]
    rd, cn = _dup(E, rows, cols, o["d"]), _neighbour(E, rows, cols)
    out = {}
    ref, s = fp.smv_ref(img, o["d"], u, rows, cols)
    out["sandwich_matvec"] = (ref, s, {"row twice": fp.smv_ref(img, o["d"], u, rd, cols)[0],
                                       "neighbour column": fp.smv_ref(img, o["d"], u, rows, cn)[0],
                                       "level shift": fp.smv_ref(bad, o["d"], u, rows, cols)[0]}, mv._err)
    ref, s = fp.diag_ref(img, o["d_diag"], rows, cols)
    out["sandwich_diag"] = (ref, s, {"row twice": fp.diag_ref(img, o["d_diag"], rd, cols)[0],
                                     "neighbour column": fp.diag_ref(img, o["d_diag"], rows, cn)[0],
                                     "level shift": fp.diag_ref(bad, o["d_diag"], rows, cols)[0]}, sd._err)
    for label, W in (("sandwich_and_transpose_matvec g", o["v"]), ("transpose_matvec 2-D", o["W"])):
        ref, s = fp.xtv_ref(img, W, rows, cols)
        out[label] = (ref, s, {"row twice": fp.xtv_ref(img, W, rd, cols)[0],
                               "neighbour column": fp.xtv_ref(img, W, rows, cn)[0],
                               "level shift": fp.xtv_ref(bad, W, rows, cols)[0]}, fp.lin_err)
    if rows is None:                    # matvec takes no row selection; a row counted twice is no fault of its own
        V = o["V"] if cols is None else o["V"][cols]
        ref, s = fp.mv_ref(img, V, cols)
        out["matvec 2-D"] = (ref, s, {"neighbour column": fp.mv_ref(img, V, cn)[0],
                                      "level shift": fp.mv_ref(bad, V, cols)[0]}, fp.lin_err)
    sub = (slice(None) if rows is None else np.asarray(rows)), (slice(None) if cols is None else np.asarray(cols))
    if np.array_equal(E[sub[0]][:, sub[1]], Es[sub[0]][:, sub[1]]):     # no column of the shifted block is selected
        assert cols is not None
        for _, _, faulty, _ in out.values():
            del faulty["level shift"]
    return out


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("name", DESIGNS)
def test_linear_products(name, dtype):
    E, zero_col = _design(name)
    Es, _ = _design(name, shift=1)
    assert E.shape == Es.shape and not np.array_equal(E, Es)
    n, p = E.shape
    o = _operands(E, dtype)
    tol = TOL[dtype]
    caught = 0
    for rows, cols in _restrictions(o, n, p):
        for label, (ref, s, faulty, err) in _linear_products(E, Es, o, rows, cols).items():
            assert err(ref.astype(dtype), ref, s) <= tol, (label, "the rounded reference")
            # one entry off by BUMP of its natural scale
            got = ref.copy()
            j = np.unravel_index(int(np.argmax(s)), s.shape)
            got[j] += BUMP[dtype] * s[j]
            assert _fails(lambda: err(got.astype(dtype), ref, s), tol), (label, "one entry off")
            for fault, got in faulty.items():
                assert got.shape == ref.shape
                assert _fails(lambda: err(got.astype(dtype), ref, s), tol), (label, fault)
                caught += 1
            # an entry of natural scale 0 (the all-zero column, when it is selected) set to 1e-300
            sel = np.arange(p) if cols is None else np.asarray(cols)
            hit = np.nonzero(sel == zero_col)[0]
            if label != "matvec 2-D" and len(hit) and dtype == np.float64:
                assert np.all(s[hit[0]] == 0)
                got = ref.astype(dtype)
                got[hit[0]] = 1e-300
                assert _fails(lambda: err(got, ref, s), tol), (label, "a zero-scale entry")
                caught += 1
    assert caught >= 40


def _glm_errs(ref, res):
    return max(gl._errors(ref, *res).values())


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", GLM_FAMILIES, ids=str)
@pytest.mark.parametrize("name", DESIGNS)
def test_glm_loss_grad(name, family, dtype):
    E, zero_col = _design(name)
    Es, _ = _design(name, shift=1)
    n, p = E.shape
    tol = TOL[dtype]
    beta, y, w, off = fp.draw_glm(np.random.default_rng(11), E, family, dtype, seed=1)
    ref = fp.glm_ref(fp.Image(E), family, beta, y, w, off)

    def result(r):
        """(loss, grad, eta, d) of a reference dict as the product returns them, in `dtype`."""
        return float(r["loss"]), r["grad"].astype(dtype), r["eta"][:n].astype(dtype), r["d"][:n].astype(dtype)

    assert _glm_errs(ref, result(ref)) <= tol, "the rounded reference"
    # one entry off by BUMP of its natural scale: in grad, in eta, in the loss
    loss, grad, eta, d = result(ref)
    g2 = ref["grad"].copy()
    j = int(np.argmax(ref["g_s"]))
    g2[j] += BUMP[dtype] * ref["g_s"][j]
    assert _fails(lambda: _glm_errs(ref, (loss, g2.astype(dtype), eta, d)), tol)
    e2 = ref["eta"].copy()
    e2[n // 2] += BUMP[dtype] * ref["t_s"][n // 2]
    assert _fails(lambda: _glm_errs(ref, (loss, grad, e2.astype(dtype), d)), tol)
    assert _fails(lambda: _glm_errs(ref, (float(ref["loss"] + BUMP[dtype] * ref["l_s"]), grad, eta, d)), tol)
    if not ref["const_d"]:
        d2 = ref["d"].copy()
        i = int(np.argmax(ref["r_s"]))
        d2[i] += BUMP[dtype] * ref["r_s"][i]
        assert _fails(lambda: _glm_errs(ref, (loss, grad, eta, d2.astype(dtype))), tol)
    # one row counted twice: the design with one row appended (loss and grad sum over it once more)
    rd = _dup(E, None, None, w)
    twice = fp.glm_ref(fp.Image(E[rd]), family, beta, y[rd], w[rd], off[rd])
    assert _fails(lambda: _glm_errs(ref, result(twice)), tol), "row twice"
    # the drop_first categorical shifted by one level
    shifted = fp.glm_ref(fp.Image(Es), family, beta, y, w, off)
    assert _fails(lambda: _glm_errs(ref, result(shifted)), tol), "level shift"
    # the gradient entry of an all-zero column set to 1e-300
    if dtype == np.float64:
        assert ref["g_s"][zero_col] == 0
        g3 = grad.copy()
        g3[zero_col] = 1e-300
        assert _fails(lambda: _glm_errs(ref, (loss, g3, eta, d)), tol), "a zero-scale entry"


def test_seed_draws_are_stable():
    """The designs the GPU module draws: no degenerate seed among the default 24, the rule of the cap as the module
    states it (a first draw above NP_CAP entries is replaced by the next draw of the same rng with n from
    (129, 1000), any other is kept), and designs on both sides of what the module's last test asks for."""
    from test_gpu_fuzz import _random_split

    facts = {}
    redrawn = []
    for seed in range(24):
        dtype = fp.seed_dtype(seed)
        X, E = fp.draw_design(np.random.default_rng(fp.BASE + seed), dtype)
        assert X is not None, seed
        facts[seed] = fp.design_facts(X, E)
        _, E1 = _random_split(np.random.default_rng(fp.BASE + seed), dtype, n_choices=fp.N_ROWS)
        if E1.shape[0] * E1.shape[1] > fp.NP_CAP:
            redrawn.append(seed)
            assert E.shape[0] in (129, 1000)
        else:
            assert np.array_equal(E, E1)
            assert E.shape[0] in fp.N_ROWS
    assert redrawn, "no seed exercises the cap"
    assert any(f["n_cat"] >= 2 for f in facts.values())
    assert any(f["widest_sparse"] > 512 for f in facts.values())
    assert any(f["n"] <= 7 for f in facts.values())
    parts = [s for s, f in facts.items() if s % 6 == fp.PARTS_RESIDUE and f["split"] and f["max_nnz"] >= 3000]
    assert parts == [5, 23]
