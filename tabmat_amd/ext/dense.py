"""Mirror of tabmat.ext.dense (reference: src/tabmat/ext/dense.pyx)."""
from __future__ import annotations

from .. import _device as D
from .._lib import call
from ._types import DenseDev


def dense_sandwich(X: DenseDev, d, rows, cols, center=None):
    """ext/dense.pyx:19-44.  rows/cols: int32 device tensors or None (= all).
    center (device tensor of the block's dtype, length X.m, or None): the product of X - 1 center'
    (tm_dense_sandwich_centered_*: the columns are centred on the way in)."""
    out_m = X.m if cols is None else D.nlen(cols)
    in_n = X.n if rows is None else D.nlen(rows)
    if in_n == 0 or out_m == 0:  # ext/dense.pyx:26-27
        return D.zeros((out_m, out_m), X.dtype)
    out = D.out_buf((out_m, out_m), X.dtype)
    D.same_float("dense_sandwich", X.buf, d)
    if center is not None:
        D.same_float("dense_sandwich", X.buf, center)
        assert center.numel() == X.m and center.is_contiguous()
        call(f"tm_dense_sandwich_centered_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, X.order_f, D.p(d), D.p(rows),
             D.nlen(rows), D.p(cols), D.nlen(cols), D.p(center), D.p(out), D.stream_ptr())
        return out
    call(f"tm_dense_sandwich_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, X.order_f, D.p(d), D.p(rows),
         D.nlen(rows), D.p(cols), D.nlen(cols), D.p(out), D.stream_ptr())
    return out


def dense_rmatvec(X: DenseDev, v, rows, cols, out=None):
    """ext/dense.pyx:48-73: X[rows, cols].T @ v[rows] (length len(cols)); accumulates into out."""
    n_cols = X.m if cols is None else D.nlen(cols)
    n_rows = X.n if rows is None else D.nlen(rows)
    if out is None:
        out = D.zeros((n_cols,), X.dtype)
    if n_rows == 0 or n_cols == 0:
        return out
    D.same_float("dense_rmatvec", X.buf, v, out)
    call(f"tm_dense_rmatvec_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, X.order_f, D.p(v), D.p(rows),
         D.nlen(rows), D.p(cols), D.nlen(cols), D.p(out), D.stream_ptr())
    return out


def dense_matvec(X: DenseDev, v, rows, cols, out=None):
    """ext/dense.pyx:76-101: X[rows, cols] @ v[cols] (length len(rows)); accumulates into out."""
    n_cols = X.m if cols is None else D.nlen(cols)
    n_rows = X.n if rows is None else D.nlen(rows)
    if out is None:
        out = D.zeros((n_rows,), X.dtype)
    if n_rows == 0 or n_cols == 0:
        return out
    D.same_float("dense_matvec", X.buf, v, out)
    call(f"tm_dense_matvec_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, X.order_f, D.p(v), D.p(rows),
         D.nlen(rows), D.p(cols), D.nlen(cols), D.p(out), D.stream_ptr())
    return out


def dense_matvec_multi(X: DenseDev, V, rows, cols, transpose):
    """2-D operand: X[rows, cols] @ V[cols] (n_rows, K) or X[rows, cols].T @ V[rows] (n_cols, K);
    the reference leaves these to NumPy BLAS (dense_matrix.py:212-217)."""
    K = int(V.shape[1])
    n_cols = X.m if cols is None else D.nlen(cols)
    n_rows = X.n if rows is None else D.nlen(rows)
    out = D.zeros((n_cols if transpose else n_rows, K), X.dtype)
    if K == 0 or n_rows == 0 or n_cols == 0:
        return out
    D.same_float("dense_matvec_multi", X.buf, V)
    Vc = V.contiguous()
    fn = "tm_dense_rmatvec_multi_" if transpose else "tm_dense_matvec_multi_"
    call(fn + D.fsuf(X.buf), D.p(X.buf), X.n, X.m, X.order_f, D.p(Vc), K, D.p(rows), D.nlen(rows),
         D.p(cols), D.nlen(cols), D.p(out), D.stream_ptr())
    return out


def transpose_square_dot_weights(X: DenseDev, weights, shift):
    """ext/dense.pyx:103-122: out[j] = sum_i w[i] * (X[i, j] - shift[j])**2."""
    out = D.zeros((X.m,), X.dtype)
    if X.n == 0 or X.m == 0:
        return out
    D.same_float("transpose_square_dot_weights", X.buf, weights, shift)
    call(f"tm_dense_col_sq_dev_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, X.order_f, D.p(weights),
         D.p(shift), D.p(out), D.stream_ptr())
    return out


def dense_gather_cols(X: DenseDev, cols, T, t0: int):
    """T[:, t0 + q] = X[:, cols[q]] (cols: int32 device tensor); T: (n, ld) row-major device tensor."""
    D.same_float("dense_gather_cols", X.buf, T)
    call(f"tm_dense_gather_cols_{D.fsuf(T)}", D.p(X.buf), X.n, X.m, int(X.order_f), D.p(cols),
         D.nlen(cols), D.p(T), T.shape[1], int(t0), D.stream_ptr())


def dense_sandwich_co(X: DenseDev, d, want_colsum=False, center=None):
    """X' diag(d) X of an unrestricted C-ordered float64 block of an even number of columns
    <= 128 with the kernel that is sized to share its compute units with a partner running on
    another stream (tm_dense_sandwich_co_f64; reference: the dense term of
    split_matrix.py:337-354).  Returns out, or (out, X' d) with want_colsum.  center (float64 device
    tensor, length X.m): product and column sums of X - 1 center' (tm_dense_sandwich_co_centered_f64)."""
    import torch

    out = D.out_buf((X.m, X.m), torch.float64)
    cs = D.out_buf((X.m,), torch.float64) if want_colsum else None
    D.same_float("dense_sandwich_co", X.buf, d, out)
    if center is not None:
        D.same_float("dense_sandwich_co", X.buf, center)
        assert center.numel() == X.m and center.is_contiguous()
        call("tm_dense_sandwich_co_centered_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(center), D.p(out), D.p(cs),
             D.stream_ptr())
        return (out, cs) if want_colsum else out
    call("tm_dense_sandwich_co_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(out), D.p(cs), D.stream_ptr())
    return (out, cs) if want_colsum else out


def co_supported(X: DenseDev, d, any_width=False) -> bool:
    """True when tm_dense_sandwich_co_f64 takes the block AND pays for it: the kernel always works on
    a 128-column panel, so blocks of <= 64 columns stay with the narrow syrk instantiations (plus a
    transpose_matvec where X'd is wanted) unless any_width is set."""
    import torch

    return (not X.order_f and X.buf.dtype == torch.float64 and d.dtype == torch.float64
            and X.m <= 128 and X.m > 0 and X.n > 0 and X.buf.data_ptr() % 16 == 0
            and (any_width or X.m > 64))


def dense_sandwich_bf16x3(X: DenseDev, d):
    """X' diag(d) X of an unrestricted C-ordered float32 block of 4 k <= 256 columns on the bf16
    matrix cores (tm_dense_sandwich_bf16x3_f32: three-piece bf16 split, f32 accumulation)."""
    import torch

    assert not X.order_f and X.buf.dtype == torch.float32 and X.m % 4 == 0 and X.m <= 256
    out = D.out_buf((X.m, X.m), torch.float32)
    D.same_float("dense_sandwich_bf16x3", X.buf, d)
    call("tm_dense_sandwich_bf16x3_f32", D.p(X.buf), X.n, X.m, D.p(d), D.p(out), D.stream_ptr())
    return out


def dense_sandwich_i8(X: DenseDev, d, colmax, want_colsum=False, history=None, center=None):
    """X' diag(d) X of an unrestricted C-ordered float64 block of an even number of columns <= 128 on
    the int8 matrix cores (tm_dense_sandwich_i8_f64: 40-bit fixed point per column, five base-256
    digits, 22 exact int8 digit-pair products).  colmax: float64 device tensor of max |x| per column.
    Weights outside the envelope (negative, non-finite, tiny exactly where a column is large) make
    the call run the f64 kernel instead (checked on the device).  want_colsum: also X' d from the
    same pass -> (out, colsum).  history: int32 device tensor of tm_dense_sandwich_i8_history_words() words
    kept per matrix (tm_dense_sandwich_i8_hist_f64: {misses in a row, calls, -, -, the previous diagonal as
    128 doubles}; after three misses in a row the int8 attempt is skipped).  center (float64 device tensor,
    length X.m): product and column sums of X - 1 center', the centre subtracted BEFORE the fixed-point
    conversion (tm_dense_sandwich_i8_centered_f64; colmax is then max |x - center| per column)."""
    import torch
    from .._lib import lib

    out = D.out_buf((X.m, X.m), torch.float64)
    D.same_float("dense_sandwich_i8", X.buf, d, colmax)
    cs = D.out_buf((X.m,), torch.float64) if want_colsum else None
    if history is not None and history.numel() < int(lib().tm_dense_sandwich_i8_history_words()):
        # (the C ABI takes no length: a short buffer would be a silent out-of-bounds device write)
        raise ValueError("history needs tm_dense_sandwich_i8_history_words() int32 words")
    if center is not None:
        D.same_float("dense_sandwich_i8", X.buf, center)
        assert center.numel() == X.m and center.is_contiguous()
        call("tm_dense_sandwich_i8_centered_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(center),
             D.p(out), D.p(cs), D.p(history), D.stream_ptr())
        return (out, cs) if want_colsum else out
    if history is not None:
        call("tm_dense_sandwich_i8_hist_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(out), D.p(cs),
             D.p(history), D.stream_ptr())
        return (out, cs) if want_colsum else out
    if want_colsum:
        call("tm_dense_sandwich_i8_xtd_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(out), D.p(cs),
             D.stream_ptr())
        return out, cs
    call("tm_dense_sandwich_i8_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(out), D.stream_ptr())
    return out


def dense_sandwich_i8_wide(X: DenseDev, d, colmax, center=None):
    """X' diag(d) X of an unrestricted C-ordered float64 block of 130 .. 512 (even) columns: the diagonal
    128-column panels on the int8 matrix cores in place, the off-diagonal panel pairs on the f64 MFMA
    (tm_dense_sandwich_i8_wide_f64; reference: the j-panels of ext/dense_helpers-tmpl.cpp:289)."""
    import torch

    out = D.out_buf((X.m, X.m), torch.float64)
    D.same_float("dense_sandwich_i8_wide", X.buf, d, colmax)
    if center is not None:
        D.same_float("dense_sandwich_i8_wide", X.buf, center)
        assert center.numel() == X.m and center.is_contiguous()
        call("tm_dense_sandwich_i8_wide_centered_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(center),
             D.p(out), D.stream_ptr())
        return out
    call("tm_dense_sandwich_i8_wide_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(colmax), D.p(out), D.stream_ptr())
    return out


def dense_sandwich_xtv(X: DenseDev, d, v, kind, colmax=None, history=None, center=None, want_colsum=False):
    """(X' diag(d) X, X' d or None, X' v) of an unrestricted C-ordered float64 block from ONE pass over it: the
    second vector v (length X.n, float64) rides in the syrk's own pass (tm_dense_sandwich_*_xtv_f64).
    kind: "i8" (K1e, <= 128 columns; calls outside its envelope are handed to K1c on the device), "i8_wide" (130 ..
    512 even columns: X' v from the diagonal 128-column panels) or "co" (K1c, <= 128 columns; want_colsum: X' d
    as well).  center (float64, length X.m): both sums are those of X - 1 center' -- the caller adds
    center * sum(v) back for X' v."""
    import torch
    from .._lib import lib

    out = D.out_buf((X.m, X.m), torch.float64)
    xtv = D.out_buf((X.m,), torch.float64)
    cs = D.out_buf((X.m,), torch.float64) if want_colsum else None
    D.same_float("dense_sandwich_xtv", X.buf, d, v, out)
    assert v.numel() == X.n and v.is_contiguous() and d.numel() == X.n
    if center is not None:
        D.same_float("dense_sandwich_xtv", X.buf, center)
        assert center.numel() == X.m and center.is_contiguous()
    if kind == "co":
        if center is not None:
            call("tm_dense_sandwich_co_centered_xtv_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(v), D.p(center),
                 D.p(out), D.p(cs), D.p(xtv), D.stream_ptr())
        else:
            call("tm_dense_sandwich_co_xtv_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(v), D.p(out), D.p(cs), D.p(xtv),
                 D.stream_ptr())
        return out, cs, xtv
    assert not want_colsum, "the int8 kernels give X' d or X' v, not both"
    D.same_float("dense_sandwich_xtv", X.buf, colmax)
    if kind == "i8_wide":
        call("tm_dense_sandwich_i8_wide_xtv_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(v), D.p(colmax), D.p(center),
             D.p(out), D.p(xtv), D.stream_ptr())
        return out, None, xtv
    assert kind == "i8"
    if history is not None and history.numel() < int(lib().tm_dense_sandwich_i8_history_words()):
        raise ValueError("history needs tm_dense_sandwich_i8_history_words() int32 words")
    if center is not None:
        call("tm_dense_sandwich_i8_centered_xtv_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(v), D.p(colmax),
             D.p(center), D.p(out), D.p(xtv), D.p(history), D.stream_ptr())
    else:
        call("tm_dense_sandwich_i8_xtv_f64", D.p(X.buf), X.n, X.m, D.p(d), D.p(v), D.p(colmax), D.p(out), D.p(xtv),
             D.p(history), D.stream_ptr())
    return out, None, xtv


# widest block the dense row walk (tm_dense_sandwich_matvec_*, tm_dense_sandwich_diag_*, tm_dense_glm_loss_grad_*)
# takes: 64 lanes x 8 loads of 16 bytes per row (rows 16-byte aligned), of one element otherwise
# (csrc/dense_rowwalk.hpp: load_form)
SANDWICH_MATVEC_MAX_BYTES = 64 * 8 * 16
SANDWICH_MATVEC_MAX_UNALIGNED = 64 * 8


def sandwich_matvec_supported(X: DenseDev) -> bool:
    """True when tm_dense_sandwich_matvec_* takes the block: C-ordered, at most 1024 (f64) / 2048 (f32) columns
    on 16-byte aligned rows, at most 512 otherwise."""
    if X.order_f or X.m == 0:
        return False
    es = X.buf.element_size()
    aligned = (X.m * es) % 16 == 0 and X.buf.data_ptr() % 16 == 0
    return X.m * es <= SANDWICH_MATVEC_MAX_BYTES if aligned else X.m <= SANDWICH_MATVEC_MAX_UNALIGNED


def dense_sandwich_matvec(X: DenseDev, u, dm, t_add=None, center=None, shift=None, want_w=False):
    """(g, w or None) with t = (X - 1 center') u + shift + t_add, w = dm * t, g = (X - 1 center)' w from ONE pass
    over a C-ordered block (tm_dense_sandwich_matvec_*).  u, center: length X.m; dm, t_add: length X.n; shift: a
    one-element device tensor; all of the block's dtype.  center / shift / t_add may be None."""
    g = D.out_buf((X.m,), X.dtype)
    w = D.out_buf((X.n,), X.dtype) if want_w else None
    D.same_float("dense_sandwich_matvec", X.buf, u, dm, t_add, center, shift)
    assert sandwich_matvec_supported(X)
    assert u.numel() == X.m and dm.numel() == X.n and u.is_contiguous() and dm.is_contiguous()
    assert t_add is None or (t_add.numel() == X.n and t_add.is_contiguous())
    assert center is None or (center.numel() == X.m and center.is_contiguous())
    assert shift is None or shift.numel() == 1
    call(f"tm_dense_sandwich_matvec_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, D.p(u), D.p(dm), D.p(t_add),
         D.p(center), D.p(shift), D.p(g), D.p(w), D.stream_ptr())
    return g, w


def dense_sandwich_diag(X: DenseDev, dm, center=None):
    """out[j] = sum_r dm[r] (X[r, j] - center[j])^2 from ONE pass over a C-ordered block (tm_dense_sandwich_diag_*:
    the diagonal of the product tm_dense_sandwich_matvec_* applies; same blocks, sandwich_matvec_supported).
    dm: length X.n, center: length X.m or None, both of the block's dtype."""
    out = D.out_buf((X.m,), X.dtype)
    D.same_float("dense_sandwich_diag", X.buf, dm, center)
    assert sandwich_matvec_supported(X)
    assert dm.numel() == X.n and dm.is_contiguous()
    assert center is None or (center.numel() == X.m and center.is_contiguous())
    call(f"tm_dense_sandwich_diag_{D.fsuf(X.buf)}", D.p(X.buf), X.n, X.m, D.p(dm), D.p(center), D.p(out),
         D.stream_ptr())
    return out


# family names of glm_loss_grad -> the TM_GLM_* codes of include/tabmat_hip.h
GLM_FAMILIES = {"gaussian": 0, "poisson": 1, "binomial": 2, "gamma": 3, "tweedie": 4, "negative_binomial": 5}
# the families that come with a parameter, ("tweedie", p) / ("negative_binomial", theta), and the parameter's name
GLM_FAMILY_PARAMS = {"tweedie": "p", "negative_binomial": "theta"}
# other spellings of a (family, parameter) pair
GLM_FAMILY_ALIASES = {"inverse_gaussian": ("tweedie", 3.0)}


def resolve_glm_family(family):
    """(code, param) of a glm_loss_grad family: a GLM_FAMILIES name, ("tweedie", p) with 1 < p < 2 or p > 2,
    ("negative_binomial", theta) with theta > 0, or "inverse_gaussian" (= ("tweedie", 3.0)).  param is 0.0 for the
    families without one.  ("tweedie", 1) and ("tweedie", 2) are poisson and gamma (the same model under the log
    link).  ValueError for anything else -- a parameterised family without its parameter included."""
    import math

    spelled = family
    if isinstance(family, str) and family in GLM_FAMILY_ALIASES:
        family = GLM_FAMILY_ALIASES[family]
    known = sorted(GLM_FAMILIES) + sorted(GLM_FAMILY_ALIASES)
    if isinstance(family, str):
        if family not in GLM_FAMILIES:
            raise ValueError(f"unknown family {spelled!r}; glm_loss_grad knows {known}")
        if family in GLM_FAMILY_PARAMS:
            pn = GLM_FAMILY_PARAMS[family]
            raise ValueError(f"family {family!r} needs its parameter {pn}: pass ({family!r}, {pn})")
        return GLM_FAMILIES[family], 0.0
    if not isinstance(family, tuple):
        raise ValueError(f"unknown family {spelled!r}; glm_loss_grad knows {known}")
    if not family or not isinstance(family[0], str) or family[0] not in GLM_FAMILIES:
        raise ValueError(f"unknown family {spelled!r}; glm_loss_grad knows {known}")
    name = family[0]
    if name not in GLM_FAMILY_PARAMS:
        raise ValueError(f"family {name!r} takes no parameter: pass {name!r}, not {spelled!r}")
    pn = GLM_FAMILY_PARAMS[name]
    if len(family) != 2:
        raise ValueError(f"family {spelled!r}: {name!r} needs exactly its parameter {pn}, as ({name!r}, {pn})")
    try:
        param = float(family[1])
    except (TypeError, ValueError):
        raise ValueError(f"family {spelled!r}: the parameter {pn} must be a number") from None
    if not math.isfinite(param):
        raise ValueError(f"family {spelled!r}: the parameter {pn} must be finite")
    if name == "tweedie":
        if param == 1.0:
            return GLM_FAMILIES["poisson"], 0.0
        if param == 2.0:
            return GLM_FAMILIES["gamma"], 0.0
        if not (1.0 < param < 2.0 or param > 2.0):
            raise ValueError(f"family {spelled!r}: glm_loss_grad serves tweedie with 1 <= p <= 2 or p > 2")
    elif not param > 0.0:
        raise ValueError(f"family {spelled!r}: theta must be > 0")
    return GLM_FAMILIES[name], param


def _glm_symbol(stem: str, family, suffix: str):
    """(symbol, leading family arguments) for a resolved family -- (code, param) or a bare code: the parameter-free
    entry point for the families without a parameter, the _p one for the others.  There param follows family as a
    HOST pointer to one double (a ctypes c_double passed by reference: it lives until the call returns)."""
    import ctypes as C

    code, param = family if isinstance(family, tuple) else (family, 0.0)
    code = int(code)
    if code in (GLM_FAMILIES[k] for k in GLM_FAMILY_PARAMS):
        return f"{stem}_p_{suffix}", (code, C.byref(C.c_double(float(param))))
    return f"{stem}_{suffix}", (code,)


def dense_glm_loss_grad(X: DenseDev, u, family, y, wt=None, t_add=None, center=None, shift=None):
    """(loss, g, eta, r, d) from ONE pass over a C-ordered block (tm_dense_glm_loss_grad_*): eta = (X - 1 center') u +
    shift + t_add, (r, d, loss) the family's weighted row function of (eta, y, wt), g = (X - 1 center')' r.  family:
    (code, param) as resolve_glm_family gives it, or a bare GLM_FAMILIES code (tweedie and negative_binomial run
    tm_dense_glm_loss_grad_p_*); u, center: length X.m; y, wt, t_add: length X.n; shift: a one-element device tensor;
    all of the block's dtype; wt / t_add / center / shift may be None.  loss: 0-dim float64 device tensor."""
    import torch

    g = D.out_buf((X.m,), X.dtype)
    eta, r, d = (D.out_buf((X.n,), X.dtype) for _ in range(3))
    loss = D.out_buf((), torch.float64)
    D.same_float("dense_glm_loss_grad", X.buf, u, y, wt, t_add, center, shift)
    assert sandwich_matvec_supported(X)
    assert u.numel() == X.m and u.is_contiguous()
    for v in (y, wt, t_add):
        assert v is None or (v.numel() == X.n and v.is_contiguous())
    assert center is None or (center.numel() == X.m and center.is_contiguous())
    assert shift is None or shift.numel() == 1
    sym, fam = _glm_symbol("tm_dense_glm_loss_grad", family, D.fsuf(X.buf))
    call(sym, D.p(X.buf), X.n, X.m, D.p(u), *fam, D.p(y), D.p(wt), D.p(t_add), D.p(center), D.p(shift), D.p(g),
         D.p(eta), D.p(r), D.p(d), D.p(loss), D.stream_ptr())
    return loss, g, eta, r, d


def glm_rowfn(family, eta, y, wt=None):
    """(loss, r, d): the family's weighted row function of an existing eta in one streaming launch
    (tm_glm_rowfn_*, tm_glm_rowfn_p_* for tweedie and negative_binomial; the device function K9 evaluates).
    family: (code, param) or a bare code, as in dense_glm_loss_grad.  eta, y, wt (or None): 1-D device tensors of
    one float dtype and length; loss: 0-dim float64 device tensor."""
    import torch

    D.same_float("glm_rowfn", eta, y, wt)
    n = eta.numel()
    assert eta.is_contiguous() and y.numel() == n and y.is_contiguous()
    assert wt is None or (wt.numel() == n and wt.is_contiguous())
    r, d = D.out_buf((n,), eta.dtype), D.out_buf((n,), eta.dtype)
    loss = D.out_buf((), torch.float64)
    sym, fam = _glm_symbol("tm_glm_rowfn", family, D.fsuf(eta))
    call(sym, *fam, D.p(eta), D.p(y), D.p(wt), n, D.p(r), D.p(d), D.p(loss), D.stream_ptr())
    return loss, r, d
