"""examples/glm_lbfgs.py end to end: every objective / gradient evaluation of the L-BFGS fit is one glm_loss_grad call
on a SplitMatrix, and the fit reaches the minimiser -- the penalised gradient recomputed in float64 numpy from
toarray() is below 10 gtol, and for Poisson beta lies within the strong-convexity bound of the IRLS fit
(f is alpha-strongly convex: |a - b| <= |grad f(a) - grad f(b)| / alpha <= (|grad f(a)| + |grad f(b)|) / alpha)."""
import os
import sys

import numpy as np
import pytest
import torch

import _cases as cs
from _gpu_util import to_tm_split

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))

ALPHA, GTOL = 1.0, 1e-8


def _grad(E, family, beta, y, alpha):
    """Penalised gradient in float64 numpy."""
    eta = E @ beta
    mu = np.exp(eta) if family == "poisson" else 1.0 / (1.0 + np.exp(-eta))
    return E.T @ (mu - y) + alpha * beta


def _design():
    n = 20_000
    specs, idx = cs.mixed_specs(n, 12, 60, (9, 4), seed=8)
    X = to_tm_split(specs, idx).to_device()
    E = np.hstack([cs.spec_toarray(s) for s in specs])
    rng = np.random.default_rng(1)
    truth = rng.standard_normal(E.shape[1]) * 0.1
    return X, E, E @ truth, rng


@pytest.mark.parametrize("family", ["poisson", "binomial"])
def test_lbfgs_reaches_the_minimiser(family):
    import glm_irls
    import glm_lbfgs
    from conftest import ABI_CALLS

    X, E, eta, rng = _design()
    if family == "poisson":
        y = rng.poisson(np.exp(eta)).astype(np.float64)
    else:
        y = (rng.random(eta.shape[0]) < 1.0 / (1.0 + np.exp(-eta))).astype(np.float64)
    y_dev = torch.from_numpy(y).cuda()
    evals = []
    before = ABI_CALLS.get("tm_dense_glm_loss_grad_f64", 0)
    beta = glm_lbfgs.fit_glm_lbfgs(X, y_dev, family, alpha=ALPHA, gtol=GTOL,
                                   callback=lambda it, b, f, gmax, ev: evals.append(ev))
    assert isinstance(beta, torch.Tensor) and beta.is_cuda
    # one fused call per evaluation (the start point included), nothing else evaluates the objective
    assert ABI_CALLS.get("tm_dense_glm_loss_grad_f64", 0) - before == evals[-1]
    b = beta.cpu().numpy()
    g = _grad(E, family, b, y, ALPHA)
    print(f"{family}: {len(evals)} iterations, {evals[-1]} evaluations, max |grad| = {np.abs(g).max():.2e}")
    assert np.abs(g).max() <= 10 * GTOL
    if family == "poisson":
        b_irls = glm_irls.fit_poisson(X, y_dev, alpha=ALPHA, iters=25).cpu().numpy()
        g_irls = _grad(E, family, b_irls, y, ALPHA)
        dist, bound = np.linalg.norm(b - b_irls), (np.linalg.norm(g) + np.linalg.norm(g_irls)) / ALPHA * 1.01
        print(f"|beta - beta_irls| = {dist:.2e}, bound {bound:.2e}")
        assert dist <= bound
