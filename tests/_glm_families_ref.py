"""Long-double reference of the parameterised GLM families of glm_loss_grad -- ("tweedie", p), ("negative_binomial",
theta), "inverse_gaussian" -- with the return dict of _reference in test_gpu_glm_loss_grad.py (so its _errors is
reused), and the natural scales of the errors.  Log link throughout: mu = exp(eta); l the half unit deviance,
r = dl/deta, h = (dmu/deta)^2 / V(mu).

With t_s = |A| |beta| + |offset| (eta is known to eps * t_s, so exp(c eta) to eps * |c| t_s relative):

    tweedie   a = exp((1-p) eta), b = exp((2-p) eta), l = t1 + t2 + t3 = y^(2-p) / ((1-p)(2-p)) - y a / (1-p) + b / (2-p)
              r_s = w (y a (1 + |1-p| t_s) + b (1 + |2-p| t_s))
              row loss scale = |t1| (1 + |2-p| |log y|) + |t2| (1 + |1-p| t_s) + |t3| (1 + |2-p| t_s)
    NB        r_s = w (y + mu (1 + t_s)) / (1 + theta mu)
              row loss scale = |y log y| + |y eta| + (y + 1/theta) (log1p(theta y) + log1p(theta mu))
    both      l_s = sum w (row loss scale) + sum r_s t_s,   g_s = |A|' r_s
"""
import numpy as np

LD = np.longdouble


def family_param(family):
    """("tweedie", p) / ("negative_binomial", theta) of a family spelling the references below take."""
    if family == "inverse_gaussian":
        return "tweedie", 3.0
    name, param = family
    return name, float(param)


def _xlogx(v):
    pos = v > 0
    return np.where(pos, v * np.log(np.where(pos, v, LD(1))), LD(0))


def row_terms(family, eta, y, t_s=None):
    """Long-double (l, r, h, r scale, loss scale) per row, unweighted.  t_s: the scale of eta's own error (|eta| when
    None: eta given exactly up to its rounding)."""
    name, param = family_param(family)
    eta = np.asarray(eta, dtype=LD)
    y = np.asarray(y, dtype=LD)
    t_s = np.abs(eta) if t_s is None else np.asarray(t_s, dtype=LD)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if name == "tweedie":
            p = LD(param)
            c1, c2 = 1 - p, 2 - p
            a, b = np.exp(c1 * eta), np.exp(c2 * eta)
            pos = y > 0
            ys = np.where(pos, y, LD(1))
            t1 = np.where(pos, np.exp(c2 * np.log(ys)) / (c1 * c2), LD(0))
            ya = np.where(pos, y * a, LD(0))
            t2, t3 = -ya / c1, b / c2
            l, r, h = t1 + t2 + t3, b - ya, b
            r_s = ya * (1 + abs(c1) * t_s) + b * (1 + abs(c2) * t_s)
            l_s = (np.abs(t1) * (1 + abs(c2) * np.abs(np.log(ys))) + np.abs(t2) * (1 + abs(c1) * t_s)
                   + np.abs(t3) * (1 + abs(c2) * t_s))
        elif name == "negative_binomial":
            th = LD(param)
            mu = np.exp(eta)
            den = 1 + th * mu
            ly, lm = np.log1p(th * y), np.log1p(th * mu)
            l = _xlogx(y) - y * eta - (y + 1 / th) * (ly - lm)
            r, h = (mu - y) / den, mu / den
            r_s = (y + mu * (1 + t_s)) / den
            l_s = np.abs(_xlogx(y)) + np.abs(y * eta) + (y + 1 / th) * (ly + lm)
        else:
            raise ValueError(family)
    return l, r, h, r_s, l_s


def reference(A, family, beta, y, w, off):
    """As _reference of test_gpu_glm_loss_grad.py: long-double loss / grad / eta / r / d and their error scales."""
    A = np.asarray(A, dtype=LD)
    beta = np.asarray(beta, dtype=LD)
    n = A.shape[0]
    w = np.ones(n, dtype=LD) if w is None else np.asarray(w, dtype=LD)
    off = np.zeros(n, dtype=LD) if off is None else np.asarray(off, dtype=LD)
    eta = A @ beta + off
    t_s = np.abs(A) @ np.abs(beta) + np.abs(off)
    l, r, h, r_s, l_s = row_terms(family, eta, y, t_s)
    r_s = w * r_s
    return dict(loss=(w * l).sum(), grad=A.T @ (w * r), eta=eta, r=w * r, d=w * h, t_s=t_s, r_s=r_s,
                g_s=np.abs(A).T @ r_s, l_s=(w * l_s).sum() + (r_s * t_s).sum(), const_d=False, w=w)


def draw_y(rng, family, eta):
    """A response in the family's domain around mu = exp(eta), float64: 30 % exact zeros for tweedie with p < 2,
    y > 0 for p > 2, counts for the negative binomial."""
    name, param = family_param(family)
    mu = np.exp(np.minimum(np.asarray(eta, dtype=np.float64), 30.0))
    n = mu.shape[0]
    if name == "tweedie":
        y = rng.gamma(2.0, mu / 2.0) + 1e-3
        if param < 2:
            y[rng.random(n) < 0.3] = 0.0
        return y
    lam = rng.gamma(1.0 / param, param * mu) if param < 1e3 else mu
    return rng.poisson(np.minimum(lam, 1e15)).astype(np.float64)
