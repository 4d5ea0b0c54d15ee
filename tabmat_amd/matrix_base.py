"""Abstract interface shared by every block type (reference:
/root/reference/src/tabmat/matrix_base.py:7-258).  Same method names, argument meaning and
return conventions; results are numpy arrays for numpy inputs and torch (cuda) tensors when the
per-call vector (d / v) is already a device tensor."""
from __future__ import annotations

from abc import ABC, abstractmethod
from typing import Optional

import numpy as np


def _parts_with_rows(parts, rows):
    """(a, b, part, rows rebased to the part or None) per row part, without the parts a row list leaves empty."""
    import torch

    for a, b, part in parts:
        r = None
        if rows is not None:
            r64 = rows.to(torch.int64)
            sel = r64[(r64 >= a) & (r64 < b)]
            if sel.numel() == 0:
                continue
            r = (sel - a).to(torch.int32)
        yield a, b, part, r


class MatrixBase(ABC):
    """Base class for DenseMatrix, SparseMatrix, CategoricalMatrix and SplitMatrix."""

    ndim = 2
    shape: tuple
    dtype: np.dtype
    __array_priority__ = 11  # win over ndarray in `vec @ mat` (matrix_base.py:239-241)

    def _once(self, name, build, key=()):
        """build() the first time (per `key`, e.g. a set of categorical blocks), the same value ever after -- the
        one cache of what a block derives from its own storage: twins, cost-model verdicts, row parts.  What build()
        returned is kept whatever it is: a None (a twin that refused the block) is not built again."""
        cache = self.__dict__.setdefault(name, {})
        key = tuple(key)
        if key not in cache:
            cache[key] = build()
        return cache[key]

    @abstractmethod
    def matvec(self, other, cols=None, out=None):
        """self[:, cols] @ other[cols]; `other` has full length; with `out` the product is
        ADDED into out and out is returned (matrix_base.py:15-30)."""

    @abstractmethod
    def transpose_matvec(self, vec, rows=None, cols=None, out=None):
        """self[rows, cols].T @ vec[rows]: length len(cols) without `out`;
        with `out` (length n_cols): out[cols[i]] += ... (matrix_base.py:32-61)."""

    @abstractmethod
    def sandwich(self, d, rows=None, cols=None):
        """(self[rows, cols].T * d[rows]) @ self[rows, cols] (matrix_base.py:63-76)."""

    def sandwich_and_transpose_matvec(self, d, v, rows=None, cols=None):
        """(self.sandwich(d, rows, cols), self.transpose_matvec(v, rows, cols)) -- the two products of one IRLS
        step.  Subclasses with a one-pass kernel override it; the results follow the two calls' conventions
        (H float64 on d's side, g on v's side).  v must be 1-D."""
        _check_1d(v)
        return self.sandwich(d, rows, cols), self.transpose_matvec(v, rows, cols)

    def sandwich_matvec(self, d, u, rows=None, cols=None):
        """self[rows, cols].T @ (d[rows] * (self[rows, cols] @ u)): sandwich(d, rows, cols) @ u without forming
        the (k, k) sandwich (a Hessian-vector product; a repeated row id counts once per occurrence).  u has
        length k = len(cols) (all columns when None), and so does the result: numpy for numpy u, a device
        tensor for a device u, in numpy's dtype of sandwich(d, rows, cols) @ u.  This default composes matvec
        and transpose_matvec; classes with a one-pass path override it."""
        a = _smv_args(self, d, u, rows, cols)
        if a.trivial is not None:
            return a.finish(a.trivial)
        return a.finish(_smv_compose(self, a))

    def sandwich_diag(self, d, rows=None, cols=None):
        """The diagonal of sandwich(d, rows, cols) -- out[q] = sum_{i in rows} d[i] self[i, cols[q]]^2 -- without
        forming the (k, k) sandwich (a Jacobi preconditioner for sandwich_matvec; a repeated row id counts once
        per occurrence, a repeated column id repeats its entry).  1-D of length k = len(cols) (all columns when
        None): numpy for a numpy d, a device tensor for a device d, in the dtype of sandwich(d, rows, cols).
        This default is correct but slow (one getcol and one transpose_matvec per selected column); every class
        of the package overrides it with a one-pass path."""
        a = _sd_args(self, d, rows, cols)
        if a.trivial is not None:
            return a.finish(a.trivial)
        return _sd_compose(self, a)

    def glm_loss_grad(self, family, beta, y, weights=None, offset=None):
        """(loss, grad, eta, d) of a GLM at beta -- what a solver needs at every iterate and line-search trial.
        family: "gaussian", "poisson", "binomial" or "gamma" (links: identity, log, logit, log), or with the log link
        ("tweedie", p) for 1 <= p <= 2 or p > 2 (p = 1 / 2 are poisson / gamma), "inverse_gaussian" (= ("tweedie", 3.0))
        and ("negative_binomial", theta) with variance mu + theta mu^2, theta > 0; the bare names "tweedie" and
        "negative_binomial", a parameter outside these ranges or a malformed tuple raise ValueError.  With
        eta = self @ beta + offset, w = weights (1 when None) and the family's half unit deviance l, r = dl/deta
        and Fisher weight h per row (include/tabmat_hip.h): loss = sum w l (half the deviance, summed in float64),
        grad = self' (w r) (its gradient in beta), d = w h (ready for sandwich / sandwich_matvec /
        sandwich_diag).  A row with weight 0 contributes exactly 0 to loss and grad and has d = 0 whatever its eta
        (zero weights are a row mask); eta is not clamped; the domains of y are the caller's contract.  beta: 1-D of
        length p; y, weights, offset: 1-D of length n.  Results are on beta's side: numpy grad / eta / d and a
        Python float loss for a numpy beta, device tensors (loss 0-dim float64, no sync) for a device beta; grad,
        eta and d have the matrix dtype.  This default is matvec, one row-function launch (tm_glm_rowfn_*) and
        transpose_matvec; classes with a one-pass dense kernel override it."""
        a = _glm_args(self, family, beta, y, weights, offset)
        return a.finish(*_glm_compose(self, a))

    @abstractmethod
    def getcol(self, i: int):
        ...

    @abstractmethod
    def toarray(self) -> np.ndarray:
        ...

    @abstractmethod
    def astype(self, dtype, order="K", casting="unsafe", copy=True):
        ...

    @abstractmethod
    def __getitem__(self, item):
        ...

    @abstractmethod
    def _get_col_stds(self, weights, col_means):
        ...

    @property
    def A(self) -> np.ndarray:
        return self.toarray()

    def __matmul__(self, other):
        return self.matvec(other)

    def __rmatmul__(self, other):
        """other @ X = (X.T @ other.T).T (matrix_base.py:98-114)."""
        if not hasattr(other, "T"):
            other = np.asarray(other)
        return self.transpose_matvec(other.T).T

    def _get_col_means(self, weights):
        return self.transpose_matvec(weights)

    def standardize(self, weights, center_predictors: bool, scale_predictors: bool):
        """StandardizedMatrix + column means + column stds (matrix_base.py:126-170)."""
        from .standardized_mat import StandardizedMatrix

        means = self._get_col_means(weights)
        stds = None
        mult = None
        if scale_predictors:
            stds = self._get_col_stds(weights, means)
            mult = one_over_var_inf_to_val(stds, 1.0)
        if center_predictors:
            shifter = -means * mult if mult is not None else -means
            out_means = means
        else:
            shifter = np.zeros_like(means)
            out_means = shifter
        return StandardizedMatrix(self, shifter, mult), out_means, stds

    # --- names: a thin version of matrix_base.py:176-237 -------------------------------
    def get_names(self, type: str = "column", missing_prefix: Optional[str] = None,
                  indices=None):
        names = list(getattr(self, "_colnames" if type == "column" else "_terms",
                             [None] * self.shape[1]))
        if missing_prefix is not None:
            idx = list(range(len(names))) if indices is None else indices
            names = [f"{missing_prefix}{idx[k]}" if nm is None else nm
                     for k, nm in enumerate(names)]
        return names

    def set_names(self, names, type: str = "column"):
        if isinstance(names, str):
            names = [names]
        if len(names) != self.shape[1]:
            raise ValueError(f"Length of names must be {self.shape[1]}")
        setattr(self, "_colnames" if type == "column" else "_terms", list(names))

    @property
    def column_names(self):
        return self.get_names(type="column")

    @column_names.setter
    def column_names(self, names):
        self.set_names(names, type="column")

    @property
    def term_names(self):
        return self.get_names(type="term")

    @term_names.setter
    def term_names(self, names):
        self.set_names(names, type="term")


def one_over_var_inf_to_val(arr: np.ndarray, val: float) -> np.ndarray:
    """1/arr with (near-)zeros mapped to val (matrix_base.py:244-258)."""
    arr = np.asarray(arr)
    tiny = np.abs(arr) < 1e-7
    with np.errstate(divide="ignore"):
        out = 1 / arr
    out[tiny] = val
    return out


def _check_1d(v):
    """sandwich_and_transpose_matvec takes one vector v (as the categorical transpose_matvec does)."""
    if getattr(v, "ndim", None) is None:
        v = np.asarray(v)
    if v.ndim > 1:
        raise NotImplementedError("sandwich_and_transpose_matvec is only implemented for 1d arrays.")


class _SmvArgs:
    """The checked arguments of one sandwich_matvec call (_smv_args)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def finish(self, g):
        """g (device tensor of length k) on u's side, in the result dtype."""
        import torch

        from . import _device as D

        if self.on_dev:
            return g.to(D.torch_dtype(self.out_dtype)) if self.out_dtype in (np.float32, np.float64) else g
        return D.to_host(g).astype(self.out_dtype, copy=False)

    def u_full(self, tdt):
        """u as a device vector over ALL columns of the matrix (zeros outside `cols`; a repeated column id adds
        up, as in self[:, cols] @ u)."""
        import torch

        from . import _device as D

        u = D.to_dev(self.u, tdt)
        if self.cols is None:
            return u
        full = torch.zeros((self.p,), dtype=tdt, device=u.device)
        full.index_add_(0, D.idx_dev(self.cols, torch.int64), u)
        return full

    def d_masked(self, tdt):
        """d as a device vector with the rows outside `rows` set to 0 (a repeated id counts per occurrence)."""
        from . import _device as D

        return D.masked_d(D.to_dev(self.d, tdt), D.idx_dev(self.rows)).contiguous()


def _smv_args(mat, d, u, rows, cols, h_dtype=None):
    """Host-side checks of sandwich_matvec (no device work): d as in sandwich (check_sandwich_compatible), u 1-D
    of length len(cols) (or the number of columns).  h_dtype: the dtype sandwich() returns (default: the
    matrix dtype).  .trivial is the result (a device tensor) when rows or cols are empty, else None."""
    import torch

    from . import _device as D
    from .util import check_sandwich_compatible, normalize_index, np_dtype_of

    if not D.is_dev(d):
        d = np.asarray(d)
    on_dev = D.is_dev(u)
    if not on_dev:
        u = np.asarray(u)
    if u.ndim > 1:
        raise NotImplementedError("sandwich_matvec is only implemented for 1d arrays.")
    check_sandwich_compatible(mat, d)
    n, p = mat.shape
    rows_n = normalize_index(rows, n)
    cols_n = normalize_index(cols, p)
    k = p if cols_n is None else len(cols_n)
    if u.ndim != 1 or u.shape[0] != k:
        raise ValueError(f"u has shape {tuple(u.shape)}; sandwich_matvec needs length {k} (the selected columns)")
    out_dtype = np.result_type(np.dtype(h_dtype if h_dtype is not None else mat.dtype), np_dtype_of(u))
    trivial = None
    if k == 0 or (rows_n is not None and len(rows_n) == 0):
        tdt = D.torch_dtype(out_dtype) if out_dtype in (np.float32, np.float64) else torch.float64
        trivial = D.zeros((k,), tdt)
    return _SmvArgs(mat=mat, d=d, u=u, rows=rows_n, cols=cols_n, n=n, p=p, k=k, on_dev=on_dev,
                    out_dtype=out_dtype, trivial=trivial)


def _smv_compose(mat, a):
    """transpose_matvec(d * matvec(u), rows, cols) on the device: the two-pass form of sandwich_matvec."""
    from . import _device as D

    tdt = D.torch_dtype(mat.dtype)
    t = mat.matvec(a.u_full(tdt), cols=a.cols)
    w = D.to_dev(a.d, tdt) * t
    return mat.transpose_matvec(w, rows=a.rows, cols=a.cols)


def _sd_args(mat, d, rows, cols, h_dtype=None):
    """Host-side checks of sandwich_diag (no device work), as sandwich makes them: check_sandwich_compatible and
    normalize_index.  h_dtype: the dtype sandwich() returns (default: the matrix dtype).  .trivial is the result
    (a device tensor) when rows or cols are empty, else None."""
    from . import _device as D
    from .util import check_sandwich_compatible, normalize_index

    on_dev = D.is_dev(d)
    if not on_dev:
        d = np.asarray(d)
    check_sandwich_compatible(mat, d)
    if d.ndim != 1:
        raise ValueError("sandwich_diag needs a 1-D weight vector")
    n, p = mat.shape
    rows_n = normalize_index(rows, n)
    cols_n = normalize_index(cols, p)
    k = p if cols_n is None else len(cols_n)
    out_dtype = np.dtype(h_dtype if h_dtype is not None else mat.dtype)
    trivial = None
    if k == 0 or (rows_n is not None and len(rows_n) == 0):
        trivial = D.zeros((k,), D.torch_dtype(out_dtype))
    return _SmvArgs(mat=mat, d=d, u=None, rows=rows_n, cols=cols_n, n=n, p=p, k=k, on_dev=on_dev,
                    out_dtype=out_dtype, trivial=trivial)


def _sd_compose(mat, a):
    """sandwich_diag column by column from getcol and transpose_matvec (the MatrixBase default)."""
    from . import _device as D

    d = D.to_host(a.d) if a.on_dev else a.d
    cols = range(a.p) if a.cols is None else a.cols.tolist()
    out = np.empty(a.k, dtype=a.out_dtype)
    for q, j in enumerate(cols):
        x = np.asarray(mat.getcol(int(j)).toarray(), dtype=d.dtype).reshape(-1)
        out[q] = np.asarray(mat.transpose_matvec(d * x, rows=a.rows, cols=[int(j)])).reshape(-1)[0]
    return D.to_dev(out, D.torch_dtype(a.out_dtype)) if a.on_dev else out


class _GlmArgs:
    """The checked arguments of one glm_loss_grad call (_glm_args)."""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    def dev(self):
        """(beta, y, weights or None, offset or None) as contiguous device vectors of the matrix dtype."""
        from . import _device as D

        tdt = D.torch_dtype(self.dtype)
        return tuple(None if v is None else D.to_dev(v, tdt) for v in (self.beta, self.y, self.weights, self.offset))

    def finish(self, loss, g, eta, d):
        """(loss, grad, eta, d) on beta's side."""
        from . import _device as D

        if self.on_dev:
            return loss.reshape(()), g, eta, d
        return float(loss.item()), D.to_host(g), D.to_host(eta), D.to_host(d)


def _glm_args(mat, family, beta, y, weights, offset):
    """Host-side checks of glm_loss_grad (no device work): a known family with a valid parameter (resolved to
    (code, param): a.family), beta 1-D of length p, y / weights / offset 1-D of length n."""
    from . import _device as D
    from .ext.dense import resolve_glm_family

    family = resolve_glm_family(family)     # (code, param); ValueError for a family glm_loss_grad does not know
    n, p = mat.shape
    on_dev = D.is_dev(beta)
    if not on_dev:
        beta = np.asarray(beta)
    if beta.ndim > 1:
        raise NotImplementedError("glm_loss_grad is only implemented for 1d arrays.")
    if beta.ndim != 1 or beta.shape[0] != p:
        raise ValueError(f"beta has shape {tuple(beta.shape)}; glm_loss_grad needs length {p} (the columns)")
    vecs = {}
    for name, v in (("y", y), ("weights", weights), ("offset", offset)):
        if v is None:
            if name == "y":
                raise ValueError("glm_loss_grad needs y")
        else:
            if not D.is_dev(v):
                v = np.asarray(v)
            if v.ndim != 1 or v.shape[0] != n:
                raise ValueError(f"{name} has shape {tuple(v.shape)}; glm_loss_grad needs length {n} (the rows)")
        vecs[name] = v
    return _GlmArgs(mat=mat, family=family, beta=beta, n=n, p=p, on_dev=on_dev,
                    dtype=np.dtype(mat.dtype), **vecs)


def _glm_compose(mat, a):
    """(loss, g, eta, d) as device tensors from matvec, tm_glm_rowfn_* and transpose_matvec: the two-pass form of
    glm_loss_grad, for any object with the two products."""
    from .ext.dense import glm_rowfn

    beta, y, wt, off = a.dev()
    eta = mat.matvec(beta)
    if off is not None:
        eta = eta + off
    eta = eta.contiguous()
    loss, r, d = glm_rowfn(a.family, eta, y, wt)
    return loss, mat.transpose_matvec(r), eta, d
