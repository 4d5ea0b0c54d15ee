"""The parameterised families of glm_loss_grad on the GPU: ("tweedie", p), ("negative_binomial", theta) and
"inverse_gaussian", through tm_glm_rowfn_p_* (the row function alone), tm_dense_glm_loss_grad_p_* (K9) and the public
call on every matrix class.  Compared with the long-double reference of _glm_families_ref.py at its error scales and
the tolerances of test_gpu_glm_loss_grad.py (1e-12 float64, 1e-4 float32); the ABI spy proves which entry point ran."""
import ctypes
import functools
import zlib

import numpy as np
import pytest
import torch

import _glm_families_ref as gr
from test_gpu_glm_loss_grad import CASES, LD, TOL, _called, _dev, _errors, _host, _mat, _spy

pytestmark = pytest.mark.gpu

TWEEDIE_P = [1.01, 1.5, 1.99, 2.5, 3.0]
NB_THETA = [0.01, 1.0, 50.0]
PARAM_FAMILIES = [("tweedie", p) for p in TWEEDIE_P] + [("negative_binomial", t) for t in NB_THETA]
K9_FAMILIES = [("tweedie", 1.5), ("negative_binomial", 1.0)]
CODES = {"tweedie": 4, "negative_binomial": 5}


def _resolved(family):
    name, param = gr.family_param(family)
    return CODES[name], param


def _suf(dtype):
    return "f64" if dtype == np.float64 else "f32"


def _weights(rng, n, dtype):
    w = (rng.random(n) + 0.1).astype(dtype)
    w[rng.random(n) < 0.1] = 0
    return w


def _assert_close(errs, dtype, what):
    print(f"{what}: " + " ".join(f"{k}={v:.2e}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= TOL[dtype], f"{what} {k}: {v:.2e}"


# ---------------------------------------------------------------------------------------------------------------
# the row function alone
# ---------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _rowfn_case(family, dtype, n, scale):
    """(eta, y, w) in `dtype` and the references without / with the weights (eta as the offset of a matrix without
    columns: t_s = |eta|), built once."""
    rng = np.random.default_rng(zlib.crc32(repr((family, dtype.__name__, n, scale)).encode()))
    eta = (scale * rng.standard_normal(n)).astype(dtype)
    y = gr.draw_y(rng, family, eta.astype(np.float64)).astype(dtype)
    w = _weights(rng, n, dtype)
    A, b = np.zeros((n, 0)), np.zeros(0)
    return eta, y, w, {None: gr.reference(A, family, b, y, None, eta), "random": gr.reference(A, family, b, y, w, eta)}


@pytest.mark.parametrize("wkind", [None, "random"])
@pytest.mark.parametrize("scale", [0.5, 3.0])
@pytest.mark.parametrize("n", [1, 5, 1027, 70001])
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", PARAM_FAMILIES, ids=str)
def test_rowfn(family, dtype, n, scale, wkind):
    """The tail only (n below a vector), several workgroups, whole vectors plus a tail."""
    from tabmat_amd.ext import dense as xd

    eta, y, w, refs = _rowfn_case(family, dtype, n, scale)
    before = _spy()
    loss, r, d = xd.glm_rowfn(_resolved(family), _dev(eta), _dev(y), _dev(w) if wkind else None)
    after = _spy()
    assert _called(before, after, f"tm_glm_rowfn_p_{_suf(dtype)}") and not _called(before, after, f"tm_glm_rowfn_{_suf(dtype)}")
    assert _host(r).dtype == dtype and _host(d).dtype == dtype and loss.dtype == torch.float64
    _assert_close(_errors(refs[wkind], loss, np.zeros(0), eta, d, r), dtype, f"{family} {dtype.__name__} n={n} s={scale}")
    if wkind:
        zero = w == 0
        assert not _host(r)[zero].any() and not _host(d)[zero].any()


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", K9_FAMILIES, ids=str)
def test_rowfn_one_element_loads(family, dtype):
    """Vectors that start one element off the 16-byte grid: the one-element load form."""
    from tabmat_amd.ext import dense as xd

    eta, y, w, _ = _rowfn_case(family, dtype, 1027, 0.5)
    before = _spy()
    loss, r, d = xd.glm_rowfn(_resolved(family), *(_dev(v)[1:] for v in (eta, y, w)))
    assert _called(before, _spy(), f"tm_glm_rowfn_p_{_suf(dtype)}")
    ref = gr.reference(np.zeros((1026, 0)), family, np.zeros(0), y[1:], w[1:], eta[1:])
    _assert_close(_errors(ref, loss, np.zeros(0), eta[1:], d, r), dtype, f"{family} {dtype.__name__} offset view")


# ---------------------------------------------------------------------------------------------------------------
# K9 with every optional input: one width per rows-per-step value and both load forms
# ---------------------------------------------------------------------------------------------------------------
K9_WIDTHS = {np.float64: (16, 17, 127, 128, 256, 512, 1024), np.float32: (16, 17, 127, 256, 512, 1024, 2048)}
K9_GRID = [(dt, w, n) for dt in (np.float64, np.float32) for w in K9_WIDTHS[dt] for n in (1, 63, 5003)]


@functools.lru_cache(maxsize=None)
def _k9_block(dtype, width, n):
    """The block, centre, shift, u, weights and t_add on the device, and per family of K9_FAMILIES the response and
    the long-double reference on the centred block -- built once per grid point; the references keep vectors only."""
    from tabmat_amd.ext import dense as xd
    from tabmat_amd.ext._types import DenseDev

    rng = np.random.default_rng(width * 13 + n)
    X = rng.standard_normal((n, width)).astype(dtype)
    c = (0.5 * rng.standard_normal(width)).astype(dtype)
    shift = np.asarray([0.3], dtype=dtype)
    u = (0.3 * rng.standard_normal(width) / np.sqrt(width)).astype(dtype)
    t_add = (0.2 * rng.standard_normal(n)).astype(dtype)
    wt = _weights(rng, n, dtype)
    blk = DenseDev.from_tensor(_dev(X))
    assert xd.sandwich_matvec_supported(blk)
    dev = {k: _dev(v) for k, v in dict(u=u, wt=wt, t_add=t_add, center=c, shift=shift).items()}
    Ac = X.astype(LD) - c.astype(LD)[None, :]
    off = t_add.astype(LD) + shift.astype(LD)[0]
    eta64 = np.asarray(Ac @ u.astype(LD) + off, dtype=np.float64)
    fam = {}
    for family in K9_FAMILIES:
        y = gr.draw_y(rng, family, eta64).astype(dtype)
        fam[family] = (_dev(y), gr.reference(Ac, family, u, y, wt, off))
    return dict(blk=blk, dev=dev, fam=fam)


@pytest.mark.parametrize("dtype,width,n", K9_GRID, ids=[f"{dt.__name__}-{w}-{n}" for dt, w, n in K9_GRID])
@pytest.mark.parametrize("family", K9_FAMILIES, ids=str)
def test_k9(family, dtype, width, n):
    from tabmat_amd.ext import dense as xd

    blkc = _k9_block(dtype, width, n)
    v = blkc["dev"]
    y_dev, ref = blkc["fam"][family]
    before = _spy()
    loss, g, eta, r, d = xd.dense_glm_loss_grad(blkc["blk"], v["u"], _resolved(family), y_dev, v["wt"], t_add=v["t_add"],
                                                center=v["center"], shift=v["shift"])
    after = _spy()
    assert _called(before, after, f"tm_dense_glm_loss_grad_p_{_suf(dtype)}")
    assert not _called(before, after, f"tm_dense_glm_loss_grad_{_suf(dtype)}")
    assert _host(g).dtype == dtype and tuple(g.shape) == (width,)
    assert all(tuple(x.shape) == (n,) for x in (eta, r, d)) and loss.dtype == torch.float64
    _assert_close(_errors(ref, loss, g, eta, d, r), dtype, f"K9 {family} {dtype.__name__} width={width} n={n}")
    # the row walk is K8's: eta is K8's w at dm = 1, bit for bit
    _, w = xd.dense_sandwich_matvec(blkc["blk"], v["u"], torch.ones_like(v["wt"]), t_add=v["t_add"], center=v["center"],
                                    shift=v["shift"], want_w=True)
    assert torch.equal(w, eta)


# ---------------------------------------------------------------------------------------------------------------
# bit-identity
# ---------------------------------------------------------------------------------------------------------------
def _host_double(param):
    """const double *param of the *_p entry points: a host pointer to one double (None: NULL)."""
    return None if param is None else ctypes.byref(ctypes.c_double(float(param)))


def _rowfn_p(code, param, eta, y, wt):
    """tm_glm_rowfn_p_* called directly, whatever the code (the wrapper routes codes 0-3 to the parameter-free one)."""
    from tabmat_amd import _device as D
    from tabmat_amd._lib import call

    r, d = torch.empty_like(eta), torch.empty_like(eta)
    loss = torch.empty((), dtype=torch.float64, device=eta.device)
    call(f"tm_glm_rowfn_p_{D.fsuf(eta)}", int(code), _host_double(param), D.p(eta), D.p(y), D.p(wt), eta.numel(), D.p(r),
         D.p(d), D.p(loss), D.stream_ptr())
    return loss, r, d


def _k9_p(code, param, blk, u, y, wt, t_add, center, shift):
    """tm_dense_glm_loss_grad_p_* called directly, whatever the code."""
    from tabmat_amd import _device as D
    from tabmat_amd._lib import call

    g = torch.empty(blk.m, dtype=u.dtype, device=u.device)
    eta, r, d = (torch.empty(blk.n, dtype=u.dtype, device=u.device) for _ in range(3))
    loss = torch.empty((), dtype=torch.float64, device=u.device)
    call(f"tm_dense_glm_loss_grad_p_{D.fsuf(blk.buf)}", D.p(blk.buf), blk.n, blk.m, D.p(u), int(code), _host_double(param),
         D.p(y), D.p(wt), D.p(t_add), D.p(center), D.p(shift), D.p(g), D.p(eta), D.p(r), D.p(d), D.p(loss),
         D.stream_ptr())
    return loss, g, eta, r, d


def _same(a, b):
    return all(torch.equal(x, z) for x, z in zip(a, b))


@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("code", [0, 1, 2, 3])
def test_p_entry_points_are_the_parameter_free_ones_for_codes_0_to_3(code, dtype):
    """param is ignored for the four families without one: the same kernels, the same bits in every output."""
    from tabmat_amd.ext import dense as xd

    rng = np.random.default_rng(40 + code)
    eta = (0.5 * rng.standard_normal(1027)).astype(dtype)
    y = (0.01 + 0.98 * rng.random(1027)).astype(dtype)                    # in every family's domain
    w = _weights(rng, 1027, dtype)
    for param in (0.0, 1.5, float("nan"), None):
        assert _same(_rowfn_p(code, param, _dev(eta), _dev(y), _dev(w)), xd.glm_rowfn(code, _dev(eta), _dev(y), _dev(w)))
    for width in (17, 128):
        blkc = _k9_block(dtype, width, 5003)
        v = blkc["dev"]
        yk = _dev((0.01 + 0.98 * rng.random(5003)).astype(dtype))
        want = xd.dense_glm_loss_grad(blkc["blk"], v["u"], code, yk, v["wt"], t_add=v["t_add"], center=v["center"],
                                      shift=v["shift"])
        got = _k9_p(code, -3.25, blkc["blk"], v["u"], yk, v["wt"], v["t_add"], v["center"], v["shift"])
        assert _same(got, want)


def test_inverse_gaussian_is_tweedie_3_and_calls_repeat():
    import tabmat_amd as tm

    rng = np.random.default_rng(3)
    n = 20_000
    X = rng.standard_normal((n, 128))
    M = tm.DenseMatrix(X)
    beta = 0.3 * rng.standard_normal(128) / np.sqrt(128)
    y = gr.draw_y(rng, "inverse_gaussian", X @ beta)
    w, off = _weights(rng, n, np.float64), 0.2 * rng.standard_normal(n)
    args = tuple(_dev(v) for v in (beta, y, w, off))
    a = M.glm_loss_grad("inverse_gaussian", *args)
    b = M.glm_loss_grad(("tweedie", 3.0), *args)
    assert _same(a, b)
    for family in K9_FAMILIES:
        yk = _dev(gr.draw_y(rng, family, X @ beta))
        a = M.glm_loss_grad(family, args[0], yk, args[2], args[3])
        b = M.glm_loss_grad(family, args[0], yk, args[2], args[3])
        assert _same(a, b)                                                # fixed-order sums: several workgroups


# ---------------------------------------------------------------------------------------------------------------
# argument errors: error returns only, nothing launches
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
def test_entry_points_refuse_bad_families_and_parameters(dtype):
    from tabmat_amd import _device as D
    from tabmat_amd._lib import TabmatHipError, call
    from tabmat_amd.ext import dense as xd

    suf = _suf(dtype)
    blkc = _k9_block(dtype, 16, 63)
    v = blkc["dev"]
    y = torch.ones_like(v["wt"])
    eta = torch.zeros_like(v["wt"])
    r, d = torch.empty_like(eta), torch.empty_like(eta)
    g = torch.empty_like(v["u"])
    loss = torch.empty((), dtype=torch.float64, device=eta.device)
    # the parameter-free entry points know codes 0-3 only
    for code in (4, 5, 6, -1):
        with pytest.raises(TabmatHipError, match="family"):
            call(f"tm_glm_rowfn_{suf}", code, D.p(eta), D.p(y), None, 63, D.p(r), D.p(d), D.p(loss), D.stream_ptr())
        with pytest.raises(TabmatHipError, match="family"):
            call(f"tm_dense_glm_loss_grad_{suf}", D.p(blkc["blk"].buf), 63, 16, D.p(v["u"]), code, D.p(y), None, None,
                 None, None, D.p(g), D.p(eta), D.p(r), D.p(d), D.p(loss), D.stream_ptr())
    bad = [(4, 0.5), (4, 1.0), (4, 2.0), (4, 0.0), (4, -1.0), (4, float("nan")), (4, float("inf")),
           (5, 0.0), (5, -0.5), (5, float("nan")), (5, float("inf")), (6, 1.5), (-1, 1.5), (4, None), (5, None)]
    for fam in bad:
        with pytest.raises(TabmatHipError, match="family"):
            _rowfn_p(*fam, eta, y, None)
        with pytest.raises(TabmatHipError, match="family"):
            _k9_p(*fam, blkc["blk"], v["u"], y, None, None, None, None)
    # ... and the wrappers pass a resolved family on as it is
    with pytest.raises(TabmatHipError):
        xd.glm_rowfn((4, 0.5), eta, y)
    with pytest.raises(TabmatHipError):
        xd.dense_glm_loss_grad(blkc["blk"], v["u"], (5, 0.0), y)


# ---------------------------------------------------------------------------------------------------------------
# zero weights are a row mask; the negative binomial is finite wherever eta is
# ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kernel", ["k9", "rowfn"])
@pytest.mark.parametrize("family", [("tweedie", 1.5), ("tweedie", 3.0), ("negative_binomial", 0.01),
                                    ("negative_binomial", 1.0), ("negative_binomial", 50.0)], ids=str)
def test_zero_weights_mask_rows_at_eta_700(family, kernel):
    """Rows with wt = 0 at eta = +-700 give exactly 0 in r and d and leave the loss finite (tweedie's exp((1-p) eta)
    overflows there for p = 3).  The negative binomial also carries such rows at wt = 1: r, d and the loss are
    finite and within tolerance of the reference."""
    from tabmat_amd.ext import dense as xd
    from tabmat_amd.ext._types import DenseDev

    rng = np.random.default_rng(zlib.crc32(repr(family).encode()))
    n, m = 2500, 33
    X = rng.standard_normal((n, m))
    u = 0.3 * rng.standard_normal(m) / np.sqrt(m)
    off = 0.2 * rng.standard_normal(n)
    w = _weights(rng, n, np.float64)
    far = rng.choice(n, 200, replace=False)
    off[far[:100]], off[far[100:]] = 700.0, -700.0
    w[far] = 0.0
    nb = family[0] == "negative_binomial"
    if nb:
        w[far[::2]] = 1.0                                       # half of them count
    eta_true = X @ u + off
    y = gr.draw_y(rng, family, np.clip(eta_true, -5, 5))
    if kernel == "k9":
        loss, g, eta, r, d = xd.dense_glm_loss_grad(DenseDev.from_tensor(_dev(X)), _dev(u), _resolved(family), _dev(y),
                                                    _dev(w), t_add=_dev(off))
    else:
        eta = _dev(eta_true)
        loss, r, d = xd.glm_rowfn(_resolved(family), eta, _dev(y), _dev(w))
        g = None
    r, d, eta = _host(r), _host(d), _host(eta)
    zero = w == 0
    assert np.array_equal(r[zero], np.zeros(int(zero.sum()))) and np.array_equal(d[zero], np.zeros(int(zero.sum())))
    assert np.isfinite(float(loss)) and np.isfinite(r).all() and np.isfinite(d).all()
    assert (np.abs(eta[far]) > 690).all()                       # eta is still written
    keep = ~zero
    if kernel == "k9":
        ref = gr.reference(X[keep], family, u, y[keep], w[keep], off[keep])
        errs = _errors(ref, loss, g, eta[keep], d[keep], r[keep])
    else:
        ref = gr.reference(np.zeros((int(keep.sum()), 0)), family, np.zeros(0), y[keep], w[keep], eta_true[keep])
        errs = _errors(ref, loss, np.zeros(0), eta[keep], d[keep], r[keep])
    if nb:
        assert (w[far] == 1).sum() == 100 and np.isfinite(np.asarray(ref["r"], dtype=np.float64)).all()
    _assert_close(errs, np.float64, f"{family} {kernel}")


# ---------------------------------------------------------------------------------------------------------------
# the public call
# ---------------------------------------------------------------------------------------------------------------
_REFS = {}
FUSED = {"dense_C": True, "dense_F": True, "sparse": False, "cat_drop_first": False, "cat_missing_zero": False}


def _setup(name, dtype, family, kind):
    key = (name, dtype, family, kind)
    if key not in _REFS:
        M, A = _mat(name, dtype)
        rng = np.random.default_rng(zlib.crc32(repr((name, dtype.__name__, family, kind)).encode()))
        n, p = A.shape
        beta = (0.3 * rng.standard_normal(p) / np.sqrt(max(p, 1))).astype(dtype)
        off = (0.2 * rng.standard_normal(n)).astype(dtype) if kind == "all" else None
        eta = np.asarray(A, dtype=np.float64) @ beta.astype(np.float64) + (0.0 if off is None else off.astype(np.float64))
        y = gr.draw_y(rng, family, eta).astype(dtype)
        w = _weights(rng, n, dtype) if kind == "all" else None
        _REFS[key] = ((beta, y, w, off), gr.reference(A, family, beta, y, w, off))
    return _mat(name, dtype) + _REFS[key]


@pytest.mark.parametrize("side", ["numpy", "device"])
@pytest.mark.parametrize("kind", ["plain", "all"])
@pytest.mark.parametrize("name", list(CASES))
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("family", K9_FAMILIES + ["inverse_gaussian"], ids=str)
def test_parity(family, dtype, name, kind, side):
    """Every matrix class; kind "all": weights with zeros and an offset.  A dense block that fuses runs
    tm_dense_glm_loss_grad_p_*, everything else tm_glm_rowfn_p_*, never a parameter-free entry point."""
    M, A, (beta, y, w, off), ref = _setup(name, dtype, family, kind)
    n, p = M.shape
    suf = _suf(dtype)
    before = _spy()
    if side == "device":
        loss, grad, eta, d = M.glm_loss_grad(family, _dev(beta), _dev(y), _dev(w), _dev(off))
        assert all(isinstance(x, torch.Tensor) and x.is_cuda for x in (loss, grad, eta, d))
        assert loss.ndim == 0 and loss.dtype == torch.float64
    else:
        loss, grad, eta, d = M.glm_loss_grad(family, beta, y, w, off)
        assert isinstance(loss, float) and all(isinstance(x, np.ndarray) for x in (grad, eta, d))
    after = _spy()
    fused, rowfn = (_called(before, after, f"tm_{s}_p_{suf}") for s in ("dense_glm_loss_grad", "glm_rowfn"))
    assert fused != rowfn                                       # one of the two, once
    if name in FUSED:
        assert fused == FUSED[name]
    for sym in (f"tm_dense_glm_loss_grad_{suf}", f"tm_glm_rowfn_{suf}"):
        assert not _called(before, after, sym), sym
    assert tuple(grad.shape) == (p,) and tuple(eta.shape) == (n,) and tuple(d.shape) == (n,)
    for x in (grad, eta, d):
        assert _host(x).dtype == dtype
    _assert_close(_errors(ref, loss, grad, eta, d), dtype, f"{family} {dtype.__name__} {name} {kind} {side}")


@functools.lru_cache(maxsize=None)
def _standardized():
    """A dense block whose columns have mean = 100 standard deviations, standardized: the fused pass reads it
    centred, so eta does not cancel the means."""
    import tabmat_amd as tm

    rng = np.random.default_rng(61)
    n, m = 4000, 24
    stds = np.array([(1.0, 5.0, 0.02, 300.0)[j % 4] for j in range(m)])
    X = (100.0 * stds)[None, :] + stds[None, :] * rng.standard_normal((n, m))
    w = rng.random(n)
    w /= w.sum()
    std = tm.DenseMatrix(X).standardize(w, True, True)[0]
    Z = X.astype(LD) * std.mult.astype(LD)[None, :] + std.shift.astype(LD)[None, :]
    return std, Z


@pytest.mark.parametrize("family", K9_FAMILIES, ids=str)
def test_standardized(family):
    std, Z = _standardized()
    rng = np.random.default_rng(zlib.crc32(repr(family).encode()))
    n, p = Z.shape
    beta = 0.3 * rng.standard_normal(p) / np.sqrt(p)
    off = 0.2 * rng.standard_normal(n)
    y = gr.draw_y(rng, family, np.asarray(Z, dtype=np.float64) @ beta + off)
    w = _weights(rng, n, np.float64)
    ref = gr.reference(Z, family, beta, y, w, off)
    before = _spy()
    res = std.glm_loss_grad(family, beta, y, w, off)
    assert _called(before, _spy(), "tm_dense_glm_loss_grad_p_f64")
    _assert_close(_errors(ref, *res), np.float64, f"standardized {family} numpy")
    resd = std.glm_loss_grad(family, _dev(beta), _dev(y), _dev(w), _dev(off))
    _assert_close(_errors(ref, *resd), np.float64, f"standardized {family} device")
