"""The parameterised families of glm_loss_grad -- ("tweedie", p), ("negative_binomial", theta), "inverse_gaussian" --
without a GPU: the long-double reference of _glm_families_ref.py checked against the definitions, the family argument
resolved and refused before any device work on every matrix class, RowShardedMatrix with a tuple family over gloo, and
the header's *_p prototypes."""
import ctypes as C
import os
import socket
import sys

import numpy as np
import pytest
import torch.distributed as dist
import torch.multiprocessing as mp

import _glm_families_ref as gr
import tabmat_amd as tm
from test_glm_loss_grad_host import _mats

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LD = np.longdouble
EPS_LD = float(np.finfo(LD).eps)

TWEEDIE_P = [1.01, 1.5, 1.99, 2.5, 3.0]
NB_THETA = [0.01, 1.0, 50.0]
PARAM_FAMILIES = [("tweedie", p) for p in TWEEDIE_P] + [("negative_binomial", t) for t in NB_THETA]


# ---------------------------------------------------------------------------------------------------------------
# the reference is right
# ---------------------------------------------------------------------------------------------------------------
def _variance(family, mu):
    name, param = gr.family_param(family)
    return mu ** LD(param) if name == "tweedie" else mu + LD(param) * mu * mu


def _draw(family, scale, seed, n=1000):
    rng = np.random.default_rng(seed)
    eta = scale * rng.standard_normal(n)
    return eta, gr.draw_y(rng, family, eta)


@pytest.mark.parametrize("scale", [0.5, 3.0])
@pytest.mark.parametrize("family", PARAM_FAMILIES + ["inverse_gaussian"], ids=str)
def test_reference_matches_the_definitions(family, scale):
    """l >= 0 with l = r = 0 at mu = y, r = dl/deta (central difference in long double) and h = mu^2 / V(mu), on 1000
    random (eta, y).  Bounds: long-double rounding (eps = 1.1e-19) at the row scales of the reference, times 64; for
    the difference quotient at step 1e-6 its truncation (step^2 / 6 times the third derivative: at most c^3 times the
    r scale, c = max(1, |1-p|, |2-p|)) and rounding (eps / step times the loss scale) -- 1e-8 covers both."""
    name, param = gr.family_param(family)
    eta, y = _draw(family, scale, 17)
    l, r, h, r_s, l_s = gr.row_terms(family, eta, y)
    assert (l >= -64 * EPS_LD * l_s).all()
    mu = np.exp(np.asarray(eta, dtype=LD))
    assert (np.abs(h - mu * mu / _variance(family, mu)) <= 64 * EPS_LD * h * (1 + abs(param) * np.abs(eta))).all()
    # at mu = y (y > 0): the deviance and its slope vanish
    pos = y > 0
    eta0 = np.log(np.asarray(y[pos], dtype=LD))
    l0, r0, _, r_s0, l_s0 = gr.row_terms(family, eta0, y[pos])
    assert (np.abs(l0) <= 64 * EPS_LD * l_s0).all()
    assert (np.abs(r0) <= 64 * EPS_LD * r_s0).all()
    # r = dl / deta
    step = LD(1e-6)
    e = np.asarray(eta, dtype=LD)
    lp = gr.row_terms(family, e + step, y)[0]
    lm = gr.row_terms(family, e - step, y)[0]
    c = max(1.0, abs(1 - param), abs(2 - param)) if name == "tweedie" else 1.0
    bound = 1e-8 * (c ** 3 * r_s + l_s * 1e-5)
    assert (np.abs((lp - lm) / (2 * step) - r) <= bound).all()


def test_reference_nb_tends_to_poisson():
    """theta = 1e-8: V = mu + theta mu^2 is poisson's up to theta mu, so l, r and h are poisson's within 1e-6 of their
    scales for mu, y up to ~10 (eta ~ N(0, 0.5^2): theta (mu + y) <= 1e-6 by a wide margin)."""
    eta, y = _draw(("negative_binomial", 1.0), 0.5, 23)
    l, r, h, _, _ = gr.row_terms(("negative_binomial", 1e-8), eta, y)
    e, yl = np.asarray(eta, dtype=LD), np.asarray(y, dtype=LD)
    mu = np.exp(e)
    ylogy = np.where(yl > 0, yl * np.log(np.where(yl > 0, yl, LD(1))), LD(0))
    lp, rp, hp = ylogy - yl * e - (yl - mu), mu - yl, mu
    assert (np.abs(l - lp) <= 1e-6 * (np.abs(ylogy) + np.abs(yl * e) + yl + mu)).all()
    assert (np.abs(r - rp) <= 1e-6 * (yl + mu)).all()
    assert (np.abs(h - hp) <= 1e-6 * mu).all()


def test_reference_inverse_gaussian_is_the_textbook_deviance():
    """p = 3: the half unit deviance of the inverse Gaussian, (y - mu)^2 / (2 mu^2 y)."""
    eta, y = _draw("inverse_gaussian", 0.5, 29)
    l, _, _, _, l_s = gr.row_terms("inverse_gaussian", eta, y)
    mu, yl = np.exp(np.asarray(eta, dtype=LD)), np.asarray(y, dtype=LD)
    assert (np.abs(l - (yl - mu) ** 2 / (2 * mu * mu * yl)) <= 64 * EPS_LD * l_s).all()


# ---------------------------------------------------------------------------------------------------------------
# the family argument, before any device work
# ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Any device work raises: the checks must come first."""
    from tabmat_amd import _device as D

    def boom(*a, **k):
        raise AssertionError("device work before the argument checks")

    monkeypatch.setattr(D, "require_gpu", boom)


ACCEPTED = [
    ("gaussian", (0, 0.0)), ("poisson", (1, 0.0)), ("binomial", (2, 0.0)), ("gamma", (3, 0.0)),
    (("tweedie", 1.5), (4, 1.5)), (("tweedie", 1.01), (4, 1.01)), (("tweedie", 2.5), (4, 2.5)),
    (("tweedie", np.float32(3)), (4, 3.0)), ("inverse_gaussian", (4, 3.0)),
    (("negative_binomial", 0.5), (5, 0.5)), (("negative_binomial", 2), (5, 2.0)),
    (("tweedie", 1), (1, 0.0)), (("tweedie", 2.0), (3, 0.0)),
]
REFUSED = ["negative_binomial", "tweedie", ("tweedie",), ("tweedie", 0.5), ("tweedie", float("nan")), ("tweedie", 0),
           ("tweedie", -1.0), ("tweedie", float("inf")), ("tweedie", 1.5, 2.0), ("tweedie", "1.5x"), ("tweedie", None),
           ("negative_binomial", 0), ("negative_binomial", -1.0), ("negative_binomial", float("inf")),
           ("negative_binomial",), ("gamma", 2.0), ("inverse_gaussian", 3.0), ("nope", 1.0), (), (4, 1.5), 4]


def _check_family_argument(mat):
    from tabmat_amd import matrix_base as mb

    n, m = mat.shape
    beta, y = np.ones(m), np.ones(n)
    for spelled, want in ACCEPTED:
        got = mb._glm_args(mat, spelled, beta, y, None, None).family
        assert got == want and type(got[0]) is int and type(got[1]) is float, (spelled, got)
        # the public call takes it too: it gets as far as the device
        with pytest.raises(AssertionError, match="device work"):
            mat.glm_loss_grad(spelled, beta, y)
    for bad in REFUSED:
        with pytest.raises(ValueError, match="family"):
            mat.glm_loss_grad(bad, beta, y)
    # a family without its parameter says which one is missing
    with pytest.raises(ValueError, match=r"parameter p\b"):
        mat.glm_loss_grad("tweedie", beta, y)
    with pytest.raises(ValueError, match=r"parameter theta\b"):
        mat.glm_loss_grad("negative_binomial", beta, y)


@pytest.mark.parametrize("k", range(8))
def test_family_argument_before_any_device_work(k, no_device):
    _check_family_argument(_mats()[k])


def test_standardized_family_argument_before_any_device_work(no_device):
    _check_family_argument(tm.StandardizedMatrix(tm.DenseMatrix(np.ones((4, 3))), np.zeros(3), np.ones(3)))


def test_alias_lives_outside_the_code_table():
    from tabmat_amd.ext import dense as xd

    assert xd.GLM_FAMILIES["tweedie"] == 4 and xd.GLM_FAMILIES["negative_binomial"] == 5
    assert "inverse_gaussian" not in xd.GLM_FAMILIES
    assert xd.resolve_glm_family("inverse_gaussian") == xd.resolve_glm_family(("tweedie", 3.0)) == (4, 3.0)


def test_wrappers_pick_the_entry_point_by_family():
    """Codes 0-3 (bare or resolved) go to the parameter-free symbols, 4 and 5 to the *_p ones with param after the
    code, as a host pointer to one double."""
    from tabmat_amd.ext import dense as xd

    for code in range(4):
        assert xd._glm_symbol("tm_glm_rowfn", code, "f64") == ("tm_glm_rowfn_f64", (code,))
        assert xd._glm_symbol("tm_dense_glm_loss_grad", (code, 0.0), "f32") == ("tm_dense_glm_loss_grad_f32", (code,))
    for stem, fam, suf in (("tm_glm_rowfn", (4, 1.5), "f32"), ("tm_dense_glm_loss_grad", (5, 0.5), "f64")):
        sym, (code, ref) = xd._glm_symbol(stem, fam, suf)
        assert sym == f"{stem}_p_{suf}" and code == fam[0]
        # a host pointer to one double
        assert isinstance(ref._obj, C.c_double) and ref._obj.value == fam[1]
        assert C.c_void_p.from_param(ref) is not None


def test_header_declares_the_p_entry_points():
    from tabmat_amd import _lib

    protos = _lib.prototypes()
    for suf in ("f32", "f64"):
        base, par = protos[f"tm_dense_glm_loss_grad_{suf}"], protos[f"tm_dense_glm_loss_grad_p_{suf}"]
        k = base.index(C.c_int)                      # family
        assert par == base[:k + 1] + [C.c_void_p] + base[k + 1:]      # const double *param
        base, par = protos[f"tm_glm_rowfn_{suf}"], protos[f"tm_glm_rowfn_p_{suf}"]
        assert base[0] is C.c_int and par == [C.c_int, C.c_void_p] + base[1:]


# ---------------------------------------------------------------------------------------------------------------
# RowShardedMatrix: a tuple family goes through untouched, ONE all-reduce of [grad, loss]
# ---------------------------------------------------------------------------------------------------------------
def _np_glm(A, family, beta, y, w, off):
    ref = gr.reference(A, family, beta, y, w, off)
    return (float(ref["loss"]), np.asarray(ref["grad"], dtype=np.float64), np.asarray(ref["eta"], dtype=np.float64),
            np.asarray(ref["d"], dtype=np.float64))


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    return port


def _worker(rank, world, port, q):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    try:
        from tabmat_amd.distributed import RowShardedMatrix, shard_bounds

        n, p = 1001, 13
        rng = np.random.default_rng(0)
        A = rng.standard_normal((n, p))
        beta = 0.1 * rng.standard_normal(p)
        w = rng.random(n)
        w[::7] = 0.0
        off = 0.1 * rng.standard_normal(n)
        lo, hi = shard_bounds(n, world, rank)

        class Local:
            shape = (hi - lo, p)
            dtype = np.dtype(np.float64)

        seen = []

        def loc(family, b, y, weights, offset):
            seen.append(family)
            return _np_glm(A[lo:hi], family, b, y, weights, offset)

        sh = RowShardedMatrix(Local(), local_glm_loss_grad=loc, bounds=(lo, hi), n_global=n)
        calls = []
        real = dist.all_reduce

        def counting(t, *a, **k):
            calls.append(tuple(t.shape))
            return real(t, *a, **k)

        dist.all_reduce = counting
        ok = True
        try:
            for family in (("tweedie", 1.5), ("negative_binomial", 0.5), "inverse_gaussian"):
                y = gr.draw_y(np.random.default_rng(5), family, A @ beta + off)
                for ww, oo in ((None, None), (w, off)):
                    want = _np_glm(A, family, beta, y, ww, oo)
                    before = len(calls)
                    loss, g, eta, d = sh.glm_loss_grad_global(family, beta, y, ww, oo)
                    ok &= len(calls) - before == 1 and calls[-1] == (p + 1,)     # ONE collective: [grad, loss]
                    ok &= seen[-1] == family                                     # passed through untouched
                    ok &= isinstance(loss, float) and isinstance(g, np.ndarray) and g.shape == (p,)
                    ok &= bool(np.isclose(loss, want[0], rtol=1e-12, atol=1e-12))
                    ok &= bool(np.allclose(g, want[1], rtol=1e-11, atol=1e-11))
                    ok &= eta.shape == (hi - lo,) and bool(np.allclose(eta, want[2][lo:hi], rtol=1e-13, atol=1e-13))     # eta, d stay local
                    ok &= d.shape == (hi - lo,) and bool(np.allclose(d, want[3][lo:hi], rtol=1e-12, atol=1e-13))
        finally:
            dist.all_reduce = real
        q.put((rank, bool(ok), (lo, hi)))
    except Exception as e:                # reported, not left for the parent's queue timeout
        q.put((rank, False, repr(e)))
    finally:
        dist.destroy_process_group()


def test_sharded_world2_one_all_reduce_tuple_family():
    world = 2
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = _free_port()
    procs = [ctx.Process(target=_worker, args=(r, world, port, q)) for r in range(world)]
    for pr in procs:
        pr.start()
    res = [q.get(timeout=300) for _ in procs]
    for pr in procs:
        pr.join(timeout=60)
        assert pr.exitcode == 0
    assert all(ok for _, ok, _ in res), res
    assert sorted(b[1] - b[0] for _, _, b in res) == [500, 501]
