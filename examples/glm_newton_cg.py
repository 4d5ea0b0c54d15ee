"""The Poisson + ridge fit of examples/glm_irls.py by truncated Newton (Newton-CG): no (p, p) matrix anywhere.

Each outer iteration takes one Newton step on  f(beta) = sum(mu - y eta) + alpha / 2 |beta|^2  (eta = X beta,
mu = exp(eta)), whose Hessian is X' diag(mu) X + alpha I.  The Newton system is solved by conjugate gradients that
only ever touch the Hessian through

    H s = X' (mu * (X s)) + alpha s        X.sandwich_matvec(mu, s) -- one pass over the dense block

so a categorical with hundreds of thousands of levels costs device vectors of length p, not the p x p sandwich
(400k levels: 1.28 TB in float64).  A step-halving line search on the penalised deviance keeps every step a
descent step.  IRLS (glm_irls.fit_poisson) and this solver have the same minimiser.

With --jacobi CG is preconditioned by the diagonal of the Hessian, X.sandwich_diag(mu) + alpha (one more pass over the
design per outer iteration), and the CG steps of both variants are printed.

    python examples/glm_newton_cg.py [rows] [levels] [--jacobi]   # configs[3] design + one categorical of `levels` levels
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def penalised_deviance(y, eta, beta, alpha):
    """2 sum(y log(y / mu) - (y - mu)) + alpha |beta|^2 (float64 device scalar)."""
    mu = torch.exp(eta.clamp(max=30.0))
    ylog = torch.where(y > 0, y * torch.log(y / mu), torch.zeros_like(y))
    return 2.0 * (ylog - (y - mu)).sum(dtype=torch.float64) + alpha * (beta.double() ** 2).sum()


def newton_cg_step(X, mu, grad, alpha, cg_rtol, cg_maxiter, precond=None):
    """s ~= -(X' diag(mu) X + alpha I)^-1 grad by CG with Hessian-vector products only; returns (s, CG steps).
    precond: the diagonal M of a Jacobi preconditioner (device vector, X.sandwich_diag(mu) + alpha) -- CG then
    runs on z = r / M; None is plain CG.  Either way it stops on the residual itself, |r| <= cg_rtol |r0|."""
    s = torch.zeros_like(grad)
    r = -grad
    z = r if precond is None else r / precond
    p = z.clone()
    rs = float(r.double() @ r.double())
    rz = rs if precond is None else float(r.double() @ z.double())
    stop = cg_rtol * rs ** 0.5
    k = 0
    while k < cg_maxiter and rs ** 0.5 > stop:
        Hp = X.sandwich_matvec(mu, p) + alpha * p
        a = rz / float(p.double() @ Hp.double())
        s += a * p
        r -= a * Hp
        rs = float(r.double() @ r.double())
        z = r if precond is None else r / precond
        rz_new = rs if precond is None else float(r.double() @ z.double())
        p = z + (rz_new / rz) * p
        rz = rz_new
        k += 1
    return s, k


def fit_poisson_newton_cg(X, y, alpha: float = 1.0, iters: int = 20, cg_rtol: float = 1e-10,
                          cg_maxiter: int = 200, tol: float = 1e-10, callback=None, precondition: bool = False):
    """X: any tabmat_amd matrix (n, p); y: device tensor of counts (n,).  Minimises the Poisson deviance
    + alpha / 2 * |beta|^2 by Newton-CG; returns beta as a device tensor of y's dtype.
    callback(it, beta, step, cg_steps, deviance) after every outer iteration.
    precondition: Jacobi-preconditioned CG with M = diag(X' diag(mu) X) + alpha, from one X.sandwich_diag(mu) per
    outer iteration (level counts of a high-cardinality categorical span orders of magnitude: far fewer CG steps)."""
    n, p = X.shape
    beta = torch.zeros(p, dtype=y.dtype, device=y.device)
    eta = X.matvec(beta)
    dev = penalised_deviance(y, eta, beta, alpha)
    for it in range(iters):
        mu = torch.exp(eta.clamp(max=30.0))
        grad = X.transpose_matvec((mu - y).contiguous()) + alpha * beta
        M = X.sandwich_diag(mu.contiguous()).to(grad.dtype) + alpha if precondition else None
        s, k = newton_cg_step(X, mu.contiguous(), grad, alpha, cg_rtol, cg_maxiter, M)
        # step halving on the penalised deviance: only descent steps are taken
        t = 1.0
        while True:
            cand = beta + t * s
            eta_c = X.matvec(cand)
            dev_c = penalised_deviance(y, eta_c, cand, alpha)
            if float(dev_c) <= float(dev) or t < 1e-6:
                break
            t *= 0.5
        if float(dev_c) > float(dev):
            break                      # no descent along s: beta is as good as this solver gets
        step = float((t * s).abs().max())
        beta, eta, dev = cand, eta_c, dev_c
        if callback is not None:
            callback(it, beta, step, k, float(dev))
        if step < tol:
            break
    return beta


def main():
    from tabmat_amd import synth

    args = [a for a in sys.argv[1:] if a != "--jacobi"]
    jacobi = "--jacobi" in sys.argv[1:] or len(args) > 2
    n = int(args[0]) if len(args) > 0 else 10_000_000
    levels = int(args[1]) if len(args) > 1 else 100_000
    X = synth.mixed_split(n, 128, 512, (256, 96, 32, levels), 0.05, torch.float64, 3)
    t0 = time.perf_counter()
    X.to_device()
    torch.cuda.synchronize()
    print(f"design {X.shape}: on the device in {(time.perf_counter() - t0) * 1e3:.0f} ms "
          f"(the float64 sandwich would be {X.shape[1] ** 2 * 8 / 1e9:.1f} GB)", flush=True)
    g = torch.Generator(device="cuda").manual_seed(0)
    truth = torch.randn(X.shape[1], dtype=torch.float64, device="cuda", generator=g) * 0.02
    y = torch.poisson(torch.exp(X.matvec(truth)), generator=g)
    for precondition in ((False, True) if jacobi else (False,)):
        ts, cgs = [], []

        def cb(it, beta, step, k, dev):
            torch.cuda.synchronize()
            ts.append(time.perf_counter())
            cgs.append(k)
            print(f"  iteration {it}: {k} CG steps, max |step| = {step:.3e}, penalised deviance = {dev:.6e}",
                  flush=True)

        torch.cuda.synchronize()
        ts.append(time.perf_counter())
        fit_poisson_newton_cg(X, y, alpha=1.0, iters=6, cg_rtol=1e-6, cg_maxiter=50 if not jacobi else 2000,
                              callback=cb, precondition=precondition)
        per = np.diff(ts) * 1e3
        print(f"Newton-CG ({'Jacobi' if precondition else 'plain'}): {len(per)} outer iterations, "
              f"{per.mean():.1f} ms per iteration, {np.mean(cgs):.1f} CG steps (sandwich_matvec calls) per iteration")


if __name__ == "__main__":
    main()
