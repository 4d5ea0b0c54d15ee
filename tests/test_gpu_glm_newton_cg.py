"""examples/glm_newton_cg.py: truncated Newton with Hessian-vector products only (sandwich_matvec) reaches the IRLS
coefficients of examples/glm_irls.py, and runs on a categorical whose sandwich could not be formed."""
import os
import sys

import numpy as np
import pytest
import torch

import _cases as cs
from _gpu_util import to_tm_split

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "examples"))


def test_newton_cg_matches_irls():
    import glm_irls
    import glm_newton_cg

    n = 20_000
    specs, idx = cs.mixed_specs(n, 12, 60, (9, 4), seed=8)
    X = to_tm_split(specs, idx).to_device()
    E = np.hstack([cs.spec_toarray(s) for s in specs])
    rng = np.random.default_rng(1)
    truth = rng.standard_normal(E.shape[1]) * 0.1
    y = torch.from_numpy(rng.poisson(np.exp(E @ truth)).astype(np.float64)).cuda()
    want = glm_irls.fit_poisson(X, y, alpha=0.5, iters=25)
    got = glm_newton_cg.fit_poisson_newton_cg(X, y, alpha=0.5, iters=30, cg_rtol=1e-12, cg_maxiter=500)
    assert isinstance(got, torch.Tensor) and got.is_cuda
    rel = float((got - want).norm() / want.norm())
    assert rel <= 1e-6, rel


def test_newton_cg_high_cardinality_descends():
    import glm_newton_cg
    import tabmat_amd as tm

    n, L = 1_000_000, 200_000
    rng = np.random.default_rng(3)
    Xd = rng.standard_normal((n, 8)) * 0.3
    codes = rng.integers(0, L, n).astype(np.int32)
    X = tm.SplitMatrix([tm.DenseMatrix(Xd), tm.CategoricalMatrix(codes, categories=np.arange(L))]).to_device()
    eff = rng.standard_normal(L) * 0.2
    y = torch.from_numpy(rng.poisson(np.exp(Xd @ (rng.standard_normal(8) * 0.2) + eff[codes])).astype(np.float64))
    devs = []
    glm_newton_cg.fit_poisson_newton_cg(X, y.cuda(), alpha=1.0, iters=3, cg_rtol=1e-6, cg_maxiter=30,
                                        callback=lambda it, beta, step, k, dev: devs.append(dev))
    assert len(devs) == 3
    beta0_dev = float(glm_newton_cg.penalised_deviance(y.cuda(), torch.zeros(n, dtype=torch.float64, device="cuda"),
                                                       torch.zeros(X.shape[1], dtype=torch.float64,
                                                                   device="cuda"), 1.0))
    seq = [beta0_dev] + devs
    assert all(b < a for a, b in zip(seq, seq[1:])), seq
