"""A first-order GLM fit on tabmat_amd blocks: L-BFGS with an Armijo backtracking line search (glum's `lbfgs`).

    f(beta) = sum_i w_i l(y_i, eta_i) + alpha / 2 |beta|^2,      eta = X beta + offset

for the gaussian, poisson, binomial and gamma families (identity, log, logit, log links) and, with the log link,
("tweedie", p), ("negative_binomial", theta) and "inverse_gaussian".  A first-order solver does
nothing per iteration but evaluate f and its gradient, at the iterate and at every line-search trial, and every such
evaluation here is ONE call

    loss, grad, eta, d = X.glm_loss_grad(family, beta, y, weights, offset)

-- one pass over the dense block of the design for eta, the loss and the gradient together (two passes plus a
dozen elementwise launches when spelled out with matvec / transpose_matvec, as examples/glm_newton_cg.py does).  The
ridge term is the solver's.  Device vectors in, device results out; the only host traffic is the scalar the line
search branches on.

    python examples/glm_lbfgs.py [rows] [family]      # the design of examples/glm_irls.py
                                                      # family: a name, tweedie:1.5, negative_binomial:0.5
"""
from __future__ import annotations

import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _two_loop(g, S, Y, rho):
    """-H g with the L-BFGS inverse Hessian H of the stored pairs (two-loop recursion; H0 = s'y / y'y)."""
    q = g.clone()
    alphas = []
    for s, yv, r in zip(reversed(S), reversed(Y), reversed(rho)):
        a = r * (s @ q)
        alphas.append(a)
        q -= a * yv
    if S:
        q *= (S[-1] @ Y[-1]) / (Y[-1] @ Y[-1])
    for (s, yv, r), a in zip(zip(S, Y, rho), reversed(alphas)):
        q += (a - r * (yv @ q)) * s
    return -q


def parse_family(text: str):
    """The family argument of the command line: a name ("poisson", "inverse_gaussian", ...) or name:parameter
    ("tweedie:1.5", "negative_binomial:0.5") -> what glm_loss_grad takes."""
    name, sep, param = text.partition(":")
    return (name, float(param)) if sep else name


def draw_response(family, eta, gen):
    """y from the family at the true eta (device tensors).  tweedie with 1 < p < 2: a compound Poisson-gamma draw
    with mean mu and variance mu^p (exact zeros included); p > 2 and "inverse_gaussian": a positive draw around mu;
    negative binomial: a gamma-mixed Poisson with variance mu + theta mu^2.  (The gamma draws come from the global
    generator: torch's gamma sampler takes none.)"""
    n, kw = eta.shape[0], dict(dtype=eta.dtype, device=eta.device)
    rand = lambda: torch.rand(n, generator=gen, **kw)          # noqa: E731
    name, param = family if isinstance(family, tuple) else (family, None)
    if name == "inverse_gaussian":
        name, param = "tweedie", 3.0
    if name == "tweedie" and param == 1:
        name = "poisson"
    if name == "tweedie" and param == 2:
        name = "gamma"
    if name == "poisson":
        return torch.poisson(torch.exp(eta), generator=gen)
    if name == "binomial":
        return (rand() < torch.sigmoid(eta)).to(eta.dtype)
    if name == "gamma" or (name == "tweedie" and param > 2):
        return torch.exp(eta) * (0.5 + rand())
    if name == "tweedie":
        # N ~ Poisson(lam) gamma jumps of shape a and mean m: lam = mu^(2-p) / (2-p), a = (2-p) / (p-1), lam m = mu
        mu = torch.exp(eta)
        lam = mu ** (2.0 - param) / (2.0 - param)
        cnt = torch.poisson(lam, generator=gen)
        shape = cnt * ((2.0 - param) / (param - 1.0))
        g = torch.distributions.Gamma(shape.clamp(min=1e-30), torch.ones_like(mu)).sample()
        return torch.where(cnt > 0, g * (mu / lam) * ((param - 1.0) / (2.0 - param)), torch.zeros_like(mu))
    if name == "negative_binomial":
        k = 1.0 / param
        lam = torch.distributions.Gamma(torch.full((n,), k, **kw), k / torch.exp(eta)).sample()
        return torch.poisson(lam, generator=gen)
    return eta + torch.randn(n, generator=gen, **kw)


def fit_glm_lbfgs(X, y, family="poisson", alpha: float = 1.0, memory: int = 10, gtol: float = 1e-8,
                  maxiter: int = 500, weights=None, offset=None, callback=None):
    """X: any tabmat_amd matrix (n, p); y (and weights, offset): device tensors (n,); family: what glm_loss_grad
    takes (a name, ("tweedie", p), ("negative_binomial", theta)).  Minimises the family's half
    deviance + alpha / 2 |beta|^2 by L-BFGS with `memory` pairs; stops when the largest entry of the penalised
    gradient is at most gtol (or after maxiter iterations).  Returns beta as a float64 device tensor.
    callback(it, beta, f, gmax, evals) after every iteration (evals: glm_loss_grad calls so far)."""
    n, p = X.shape
    dt = y.dtype
    evals = 0

    def f_and_g(b):
        nonlocal evals
        evals += 1
        loss, grad, _, _ = X.glm_loss_grad(family, b.to(dt), y, weights, offset)
        return float(loss) + 0.5 * alpha * float(b @ b), grad.to(torch.float64) + alpha * b

    beta = torch.zeros(p, dtype=torch.float64, device=y.device)
    f, g = f_and_g(beta)
    S, Y, rho = [], [], []
    eps = np.finfo(np.float64).eps
    for it in range(maxiter):
        gmax = float(g.abs().max())
        if gmax <= gtol:
            break
        s = _two_loop(g, S, Y, rho)
        gs = float(g @ s)
        if gs >= 0.0:                                   # not a descent direction (rounding): restart from -g
            S, Y, rho = [], [], []
            s, gs = -g, -float(g @ g)
        t = 1.0 if S else min(1.0, 1.0 / float(g.abs().sum()))
        while True:
            cand = beta + t * s
            f_c, g_c = f_and_g(cand)
            # Armijo; once the decrease is below the rounding of f, a smaller gradient decides instead
            if f_c <= f + 1e-4 * t * gs or (f_c <= f + 8 * eps * abs(f) and float(g_c @ g_c) < float(g @ g)):
                break
            t *= 0.5
            if t < 1e-12:
                return beta                             # no progress along s: beta is as good as it gets
        sv, yv = cand - beta, g_c - g
        sy = float(sv @ yv)
        if sy > 1e-12 * float(sv.norm() * yv.norm()):
            S.append(sv)
            Y.append(yv)
            rho.append(1.0 / sy)
            if len(S) > memory:
                S.pop(0), Y.pop(0), rho.pop(0)
        beta, f, g = cand, f_c, g_c
        if callback is not None:
            callback(it, beta, f, float(g.abs().max()), evals)
    return beta


def main():
    from tabmat_amd import synth

    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    family = parse_family(sys.argv[2]) if len(sys.argv) > 2 else "poisson"
    X = synth.mixed_split(n, 128, 512, (256, 96, 32), 0.05, torch.float64, 3)
    t0 = time.perf_counter()
    X.to_device()
    torch.cuda.synchronize()
    print(f"design {X.shape}: twins built in {(time.perf_counter() - t0) * 1e3:.0f} ms", flush=True)
    gen = torch.Generator(device="cuda").manual_seed(0)
    truth = torch.randn(X.shape[1], dtype=torch.float64, device="cuda", generator=gen) * 0.02
    eta = X.matvec(truth)
    y = draw_response(family, eta, gen)
    ts, ev = [], [0]

    def cb(it, beta, f, gmax, evals):
        torch.cuda.synchronize()
        ts.append(time.perf_counter())
        ev.append(evals)
        if it % 10 == 0:
            print(f"  iteration {it}: f = {f:.9e}, max |gradient| = {gmax:.3e}, {evals} evaluations", flush=True)

    torch.cuda.synchronize()
    ts.append(time.perf_counter())
    beta = fit_glm_lbfgs(X, y, family, alpha=1.0, gtol=1e-6 * n, maxiter=60, callback=cb)
    per = np.diff(ts) * 1e3
    print(f"L-BFGS ({family}): {len(per)} iterations, {per[1:].mean() if len(per) > 1 else per[0]:.1f} ms per iteration, "
          f"{(ev[-1] - 1) / max(len(per), 1):.2f} evaluations (glm_loss_grad calls) per iteration; "
          f"max |beta - truth| = {float((beta - truth).abs().max()):.3e}")


if __name__ == "__main__":
    main()
