"""glm_loss_grad (one pass over the dense block, tm_dense_glm_loss_grad_*; tm_glm_rowfn_* where no dense block takes
it) against the composition a caller had to spell out before -- matvec, the torch elementwise code of
examples/glm_newton_cg.py (its Poisson lines, and the same spelling for the other families), transpose_matvec --
and against sandwich_matvec on the same design: the row walk without transcendentals, the floor of the fused call.
Device vectors, a synchronize around every call, interleaved A / B / C in one process, min / median of 16 calls after
3 warm-up calls each.  Also the register / scratch / occupancy report of every K9 instantiation next to K8's and K8d's (from
hipcc's -Rpass-analysis=kernel-resource-usage; needs no GPU).

    python scripts/dev/time_glm_loss_grad.py [rows] [--out profiles/glm_loss_grad.txt] [--no-timings] [--no-resources]

The sections are APPENDED to --out (so the two halves can come from two machines).
"""
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

FAMILIES = ("gaussian", "poisson", "binomial", "gamma", ("tweedie", 1.5), ("negative_binomial", 1.0))
OUT = []


def say(line=""):
    print(line, flush=True)
    OUT.append(line)


def wall(fn, reps):
    import torch

    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def composition(X, family, beta, y):
    """(loss, grad, eta, d) the way the parent commit's callers wrote it (examples/glm_newton_cg.py:30-34, 72-76);
    the same spelling for tweedie and the negative binomial."""
    import torch

    eta = X.matvec(beta)
    if family == "gaussian":
        r = eta - y
        loss = 0.5 * (r * r).sum(dtype=torch.float64)
        d = torch.ones_like(eta)
    elif family == "poisson":
        mu = torch.exp(eta.clamp(max=30.0))
        ylog = torch.where(y > 0, y * torch.log(y / mu), torch.zeros_like(y))
        loss = (ylog - (y - mu)).sum(dtype=torch.float64)
        r, d = mu - y, mu
    elif family == "binomial":
        mu = torch.sigmoid(eta)
        loss = (torch.nn.functional.softplus(eta) - y * eta).sum(dtype=torch.float64)
        r, d = mu - y, mu * (1 - mu)
    elif family == "gamma":
        ye = y * torch.exp(-eta.clamp(min=-30.0))
        loss = (ye - 1 - torch.log(y) + eta).sum(dtype=torch.float64)
        r, d = 1 - ye, torch.ones_like(eta)
    elif family[0] == "tweedie":
        p = family[1]
        ec = eta.clamp(min=-30.0, max=30.0)
        a, b = torch.exp((1 - p) * ec), torch.exp((2 - p) * ec)
        ypow = torch.where(y > 0, y ** (2 - p), torch.zeros_like(y))
        loss = (ypow / ((1 - p) * (2 - p)) - y * a / (1 - p) + b / (2 - p)).sum(dtype=torch.float64)
        r, d = b - y * a, b
    else:
        th = family[1]
        mu = torch.exp(eta.clamp(max=30.0))
        den = 1 + th * mu
        loss = (torch.xlogy(y, y) - y * eta - (y + 1 / th) * (torch.log1p(th * y) - torch.log1p(th * mu))).sum(dtype=torch.float64)
        r, d = (mu - y) / den, mu / den
    return loss, X.transpose_matvec(r.contiguous()), eta, d


def draw_y(family, eta, gen):
    import torch

    if family == "poisson":
        return torch.poisson(torch.exp(eta), generator=gen)
    if family == "binomial":
        return (torch.rand(eta.shape, dtype=eta.dtype, device=eta.device, generator=gen) < torch.sigmoid(eta)).to(eta.dtype)
    if family == "gamma":
        return torch.exp(eta) * (0.5 + torch.rand(eta.shape, dtype=eta.dtype, device=eta.device, generator=gen))
    if isinstance(family, tuple):
        # tweedie (1 < p < 2): 30 % exact zeros, positive otherwise; negative binomial: counts
        if family[0] == "negative_binomial":
            return torch.poisson(torch.exp(eta), generator=gen)
        u = torch.rand(eta.shape, dtype=eta.dtype, device=eta.device, generator=gen)
        return torch.where(u < 0.3, torch.zeros_like(eta), torch.exp(eta) * (0.5 + u))
    return eta + torch.randn(eta.shape, dtype=eta.dtype, device=eta.device, generator=gen)


def abc(title, mat, rounds=8):
    import torch

    n, p = mat.shape
    tdt = torch.float64 if mat.dtype == np.float64 else torch.float32
    gen = torch.Generator(device="cuda").manual_seed(0)
    beta = torch.randn(p, dtype=tdt, device="cuda", generator=gen) * 0.02
    eta0 = mat.matvec(beta)
    d0 = torch.rand(n, dtype=tdt, device="cuda", generator=gen)
    say(f"{title}: ms per call (min / median of {2 * rounds})")
    smv = lambda: mat.sandwich_matvec(d0, beta)          # noqa: E731
    wall(smv, 3)
    for family in FAMILIES:
        y = draw_y(family, eta0, gen)
        runs = {
            "glm_loss_grad": lambda: mat.glm_loss_grad(family, beta, y),
            "matvec + torch + transpose_matvec": lambda: composition(mat, family, beta, y),
            "sandwich_matvec": smv,
        }
        for fn in runs.values():
            wall(fn, 3)
        res = {k: [] for k in runs}
        for _ in range(rounds):
            for k, fn in runs.items():
                res[k] += wall(fn, 2)
        a, b, c = (np.asarray(res[k]) for k in runs)
        say(f"  {family if isinstance(family, str) else '%s(%g)' % family}")
        for k, ts in res.items():
            say(f"    {k:36s} {min(ts):7.3f} / {float(np.median(ts)):7.3f}")
        say(f"    fused / composition (median) = {np.median(a) / np.median(b):.3f};  fused / sandwich_matvec (median) = "
            f"{np.median(a) / np.median(c):.3f}, spread of the ratio over the rounds "
            f"{(a / np.median(c)).min():.3f} .. {(a / np.median(c)).max():.3f}")


def timings(n):
    import torch

    from tabmat_amd import synth
    import tabmat_amd as tm

    say(f"== timings, one MI355X, {n} rows ==")
    X = synth.dense_block(n, 128, torch.float64, 3)
    abc(f"DenseMatrix {n} x 128 float64 (K9 alone)", X)
    del X
    torch.cuda.empty_cache()
    mat = synth.mixed_split(n)
    mat.to_device()
    abc(f"configs[3] SplitMatrix (dense 128 + sparse 512 @ 5 % + 3 categoricals), n = {n}", mat)
    del mat
    torch.cuda.empty_cache()
    blocks = [synth.sparse_block(n, 512, 0.05, torch.float64, 1003)]
    blocks += [synth.cat_block(n, c, 2003 + i, np.float64) for i, c in enumerate((256, 96, 32))]
    mat = tm.SplitMatrix(blocks)
    mat.to_device()
    abc(f"sparse 512 @ 5 % + 3 categoricals, no dense block (tm_glm_rowfn path), n = {n}", mat)


def resources():
    """vgpr / sgpr / scratch / waves per SIMD of every dense_glm_loss_grad_kernel, dense_sandwich_matvec_kernel and
    dense_sandwich_diag_kernel instantiation, from the compiler's resource report."""
    csrc = os.path.join(ROOT, "tabmat_amd", "csrc")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    table = {}
    with tempfile.TemporaryDirectory() as tmp:
        for src in ("glm.hip", "sandwich_matvec.hip"):
            r = subprocess.run([hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-munsafe-fp-atomics",
                                "--offload-device-only", "-Rpass-analysis=kernel-resource-usage", "-c",
                                os.path.join(csrc, src), "-o", os.path.join(tmp, "dev.o")],
                               capture_output=True, text=True, check=True)
            cur = None
            for line in r.stderr.splitlines():
                m = re.search(r"Function Name: (\S+)", line)
                if m:
                    cur = table.setdefault(m.group(1), {})
                m = re.search(r"remark:\s+(\w+)( \[[^]]*\])?: (\d+)", line)
                if m and cur is not None:
                    cur[m.group(1)] = int(m.group(3))
    rows = {}
    for name, v in table.items():
        # (the row function is the last template argument of K9 and of glm_rowfn: GlmRow, or GlmRowP = Tweedie / NB)
        m = re.search(r"\d+dense_(glm_loss_grad|sandwich_matvec|sandwich_diag)_kernelI([fd])Li(\d+)ELi(\d+)ELi(\d+)ELi(\d+)", name)
        if m:
            key = ("f32" if m.group(2) == "f" else "f64", int(m.group(3)), int(m.group(4)), int(m.group(5)), int(m.group(6)))
            kern = {"glm_loss_grad": "K9", "sandwich_matvec": "K8", "sandwich_diag": "K8d"}[m.group(1)]
            rows.setdefault(key, {})[kern + ("p" if "GlmRowP" in name else "")] = v
        m = re.search(r"\d+glm_rowfn_kernelI([fd])Li(\d+)", name)
        if m:
            key = ("f32" if m.group(1) == "f" else "f64", int(m.group(2)), 0, 0, 0)
            rows.setdefault(key, {})["rowfnp" if "GlmRowP" in name else "rowfn"] = v
    say("== registers, scratch and waves per SIMD (hipcc -Rpass-analysis=kernel-resource-usage, gfx950) ==")
    say("  K9 / glm_rowfn: gaussian, poisson, binomial, gamma;  K9p / second glm_rowfn column: tweedie, negative_binomial")
    say("  layout                           K9: vgpr scratch waves     K9p: vgpr scratch waves      K8: vgpr scratch waves"
        "     K8d: vgpr scratch waves")
    for key in sorted(rows):
        dt, vec, lpr, nl, r = key
        v = rows[key]
        if "rowfn" in v:
            say(f"  glm_rowfn {dt} VEC={vec}:      " + "".join(
                f"        {k['VGPRs']:8d} {k['ScratchSize']:7d} {k['Occupancy']:5d}" for k in (v["rowfn"], v["rowfnp"])))
            continue
        say(f"  {dt} VEC={vec} LPR={lpr:2d} NL={nl} R={r}" + "".join(
            f"        {k['VGPRs']:8d} {k['ScratchSize']:7d} {k['Occupancy']:5d}" for k in (v["K9"], v["K9p"], v["K8"], v["K8d"])))


def main():
    args = sys.argv[1:]
    out = os.path.join(ROOT, "profiles", "glm_loss_grad.txt")
    if "--out" in args:
        out = args[args.index("--out") + 1]
        del args[args.index("--out"):args.index("--out") + 2]
    flags = {a for a in args if a.startswith("--")}
    pos = [a for a in args if not a.startswith("--")]
    n = int(pos[0]) if pos else 10_000_000
    if "--no-resources" not in flags:
        resources()
    if "--no-timings" not in flags:
        timings(n)
    os.makedirs(os.path.dirname(os.path.abspath(out)) or ".", exist_ok=True)
    with open(out, "a") as f:
        f.write("\n".join(OUT) + "\n")


if __name__ == "__main__":
    main()
