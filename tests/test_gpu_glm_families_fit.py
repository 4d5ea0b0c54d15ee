"""examples/glm_lbfgs.py with the parameterised families: the L-BFGS fit of ("tweedie", 1.5) and
("negative_binomial", 1.0) on the design of test_gpu_glm_lbfgs.py.  Both deviances are convex in beta under the log
link (d2l/deta2 = (2-p) b + (p-1) y a and mu (1 + theta y) / (1 + theta mu)^2, both >= 0) and alpha = 1 makes the
objective strongly convex, so the fit has one minimiser: every evaluation is one tm_dense_glm_loss_grad_p_f64 call, and
the penalised gradient recomputed in float64 numpy from toarray() is below 10 gtol (the criterion of
test_gpu_glm_lbfgs.py)."""
import os
import sys

import numpy as np
import pytest
import torch

import _glm_families_ref as gr
from test_gpu_glm_lbfgs import ALPHA, GTOL, _design

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def _grad(E, family, beta, y, alpha):
    """Penalised gradient in float64 numpy."""
    name, param = family
    eta = E @ beta
    if name == "tweedie":
        r = np.exp((2.0 - param) * eta) - y * np.exp((1.0 - param) * eta)
    else:
        mu = np.exp(eta)
        r = (mu - y) / (1.0 + param * mu)
    return E.T @ r + alpha * beta


@pytest.mark.parametrize("family", [("tweedie", 1.5), ("negative_binomial", 1.0)], ids=str)
def test_lbfgs_reaches_the_minimiser(family):
    import glm_lbfgs
    from conftest import ABI_CALLS

    X, E, eta, rng = _design()
    y = gr.draw_y(rng, family, eta)
    y_dev = torch.from_numpy(y).cuda()
    evals = []
    before = dict(ABI_CALLS)
    beta = glm_lbfgs.fit_glm_lbfgs(X, y_dev, family, alpha=ALPHA, gtol=GTOL,
                                   callback=lambda it, b, f, gmax, ev: evals.append(ev))
    assert isinstance(beta, torch.Tensor) and beta.is_cuda
    # one fused call per evaluation (the start point included), nothing else evaluates the objective
    assert ABI_CALLS.get("tm_dense_glm_loss_grad_p_f64", 0) - before.get("tm_dense_glm_loss_grad_p_f64", 0) == evals[-1]
    for sym in ("tm_dense_glm_loss_grad_f64", "tm_glm_rowfn_f64", "tm_glm_rowfn_p_f64"):
        assert ABI_CALLS.get(sym, 0) == before.get(sym, 0), sym
    g = _grad(E, family, beta.cpu().numpy(), y, ALPHA)
    print(f"{family}: {len(evals)} iterations, {evals[-1]} evaluations, max |grad| = {np.abs(g).max():.2e}")
    assert np.abs(g).max() <= 10 * GTOL


def test_example_family_argument_and_draws():
    """The command line's family spellings, and a response in each family's domain with the family's mean."""
    import glm_lbfgs

    assert glm_lbfgs.parse_family("tweedie:1.5") == ("tweedie", 1.5)
    assert glm_lbfgs.parse_family("negative_binomial:0.5") == ("negative_binomial", 0.5)
    assert glm_lbfgs.parse_family("inverse_gaussian") == "inverse_gaussian"
    assert glm_lbfgs.parse_family("poisson") == "poisson"
    gen = torch.Generator(device="cuda").manual_seed(0)
    eta = 0.3 * torch.randn(100_000, dtype=torch.float64, device="cuda", generator=gen)
    mean = float(torch.exp(eta).mean())
    for spelled, zeros in (("tweedie:1.5", True), ("negative_binomial:0.5", True), ("inverse_gaussian", False)):
        y = glm_lbfgs.draw_response(glm_lbfgs.parse_family(spelled), eta, gen)
        assert y.is_cuda and y.dtype == torch.float64 and bool((y >= 0).all()) and bool(torch.isfinite(y).all())
        assert bool((y == 0).any()) == zeros
        # the sample mean of 1e5 draws with variance <= ~2: within 5 standard errors (0.025)
        assert abs(float(y.mean()) - mean) <= 0.025, spelled
