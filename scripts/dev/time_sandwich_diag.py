"""sandwich_diag (the diagonal of X'DX from one pass over each block: tm_dense_sandwich_diag_*, tm_csr_sandwich_diag_*,
the categorical histograms) against sandwich(d).diagonal() and against sandwich_matvec on the same matrix; the fused
two-moment CSR kernel against tm_csr_rmatvec + tm_csr_col_sq on a compacted sparse block; and the Newton-CG example
plain against Jacobi-preconditioned.  Device vectors, a synchronize around every call, interleaved A / B in one
process, min / median of 16 calls after 3 warm-up calls each.

    python scripts/dev/time_sandwich_diag.py [rows] [rows of the Newton-CG design] [its levels]   # 10M, 10M, 100k
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
import tabmat_amd as tm  # noqa: E402
from tabmat_amd import synth  # noqa: E402


def wall(fn, reps):
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def interleaved(title, runs, rounds=8):
    for fn in runs.values():
        wall(fn, 3)
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            res[k] += wall(fn, 2)
    first = next(iter(res))
    print(f"{title}: ms per call (min / median of {len(res[first])})")
    for k, ts in res.items():
        print(f"  {k:34s} {min(ts):7.3f} / {float(np.median(ts)):7.3f}")
    base = float(np.median(res[first]))
    print("  " + ";  ".join(f"{first} / {k} (median) = {base / float(np.median(ts)):.3f}"
                            for k, ts in res.items() if k != first), flush=True)


def ab(title, mat, with_sandwich=True):
    n, p = mat.shape
    tdt = torch.float64 if mat.dtype == np.float64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.rand(n, dtype=tdt, device="cuda", generator=g)
    u = torch.randn(p, dtype=tdt, device="cuda", generator=g)
    runs = {"sandwich_diag": lambda: mat.sandwich_diag(d),
            "sandwich_matvec": lambda: mat.sandwich_matvec(d, u)}
    if with_sandwich:
        runs["sandwich(d).diagonal()"] = lambda: mat.sandwich(d).diagonal()
    interleaved(title, runs)


def sparse_alone(n):
    from tabmat_amd.ext import sparse as xs

    X = synth.sparse_block(n, 512, 0.05, torch.float64, 1003)
    X.to_device()
    A = X._dev()
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)

    def two_launches():
        s1 = xs.csc_rmatvec(A, d, None, None)
        return s1, xs.transpose_square_dot_weights(A, d)

    runs = {"tm_csr_sandwich_diag (s1 and s2)": lambda: xs.csr_sandwich_diag(A, d, want_s1=True),
            "tm_csr_sandwich_diag (s2 only)": lambda: xs.csr_sandwich_diag(A, d),
            "tm_csr_rmatvec + tm_csr_col_sq": two_launches}
    grow = {}
    for k, fn in runs.items():
        from tabmat_amd.ext import _types as ty

        ty.release_index_scratch()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        fn()
        torch.cuda.synchronize()
        grow[k] = (torch.cuda.max_memory_allocated() - base, torch.cuda.memory_allocated() - base)
    interleaved(f"SparseMatrix {n} x 512 @ 5 % float64, 16-bit column twin only ({A.data.numel()} nonzeros)", runs)
    for k, (peak, kept) in grow.items():
        print(f"  {k:34s} device bytes: peak growth {peak / 2**20:8.1f} MiB, kept after the call {kept / 2**20:8.1f} MiB")


def newton(n, levels):
    import glm_newton_cg

    X = synth.mixed_split(n, 128, 512, (256, 96, 32, levels), 0.05, torch.float64, 3)
    X.to_device()
    g = torch.Generator(device="cuda").manual_seed(0)
    truth = torch.randn(X.shape[1], dtype=torch.float64, device="cuda", generator=g) * 0.02
    y = torch.poisson(torch.exp(X.matvec(truth)), generator=g)
    print(f"Newton-CG, design {X.shape} (configs[3] + one categorical of {levels} levels), alpha = 1, cg_rtol = 1e-6, "
          f"cg_maxiter = 2000, 6 outer iterations")
    for pre in (False, True):
        ts, cgs = [], []

        def cb(it, beta, step, k, dev):
            torch.cuda.synchronize()
            ts.append(time.perf_counter())
            cgs.append(k)

        torch.cuda.synchronize()
        ts.append(time.perf_counter())
        glm_newton_cg.fit_poisson_newton_cg(X, y, alpha=1.0, iters=6, cg_rtol=1e-6, cg_maxiter=2000, tol=0.0,
                                            callback=cb, precondition=pre)
        per = np.diff(ts) * 1e3
        print(f"  {'Jacobi' if pre else 'plain '}: {per.mean():8.1f} ms per Newton iteration, CG steps {cgs} "
              f"(total {sum(cgs)}), fit {per.sum():.0f} ms", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    n_cg = int(sys.argv[2]) if len(sys.argv) > 2 else 10_000_000
    levels = int(sys.argv[3]) if len(sys.argv) > 3 else 100_000
    for k, dt in [(128, torch.float64), (128, torch.float32), (512, torch.float64)]:
        X = synth.dense_block(n, k, dt, 3)
        ab(f"DenseMatrix {n} x {k} {str(dt).replace('torch.', '')}", X)
        del X
        torch.cuda.empty_cache()
    mat = synth.mixed_split(n)
    mat.to_device()
    ab(f"configs[3] SplitMatrix, n = {n}", mat)
    del mat
    torch.cuda.empty_cache()
    sparse_alone(max(1, n // 5))
    torch.cuda.empty_cache()
    newton(n_cg, levels)


if __name__ == "__main__":
    main()
