"""sandwich_and_transpose_matvec against sandwich + transpose_matvec at BASELINE configs[3] (dense 128 + sparse 512 @ 5 %
+ categoricals 256 / 96 / 32, float64), and the IRLS iteration of examples/glm_irls.py.  Wall time per call with a
device vector and a synchronize, interleaved A / B so that clock drift hits both sides alike.

    python scripts/dev/time_sandwich_tmv.py [rows]        # default 10M
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "examples"))
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


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    mat = synth.mixed_split(n)
    mat.to_device()
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.rand(n, dtype=torch.float64, device="cuda", generator=g)
    v = torch.randn(n, dtype=torch.float64, device="cuda", generator=g)
    runs = {
        "sandwich": lambda: mat.sandwich(d),
        "transpose_matvec": lambda: mat.transpose_matvec(v),
        "separate (sandwich + transpose_matvec)": lambda: (mat.sandwich(d), mat.transpose_matvec(v)),
        "fused sandwich_and_transpose_matvec": lambda: mat.sandwich_and_transpose_matvec(d, v),
    }
    for fn in runs.values():
        wall(fn, 3)
    res = {k: [] for k in runs}
    for _ in range(8):
        for k, fn in runs.items():
            res[k] += wall(fn, 2)
    print(f"configs[3] shape, n = {n}: ms per call (min / median of {len(res['sandwich'])})")
    for k, ts in res.items():
        print(f"  {k:42s} {min(ts):7.3f} / {float(np.median(ts)):7.3f}")
    fused, sw = float(np.median(res["fused sandwich_and_transpose_matvec"])), float(np.median(res["sandwich"]))
    sep = float(np.median(res["separate (sandwich + transpose_matvec)"]))
    print(f"  fused - sandwich = {fused - sw:+.3f} ms (target <= +0.6);  saved against separate: {sep - fused:.3f} ms")

    # the IRLS iteration of examples/glm_irls.py (fused since round 7) and the same loop with the two calls
    import glm_irls

    truth = torch.randn(mat.shape[1], dtype=torch.float64, device="cuda", generator=g) * 0.02
    y = torch.poisson(torch.exp(mat.matvec(truth)), generator=g)

    def irls_ms(X):
        ts = []

        def cb(it, beta, step):
            torch.cuda.synchronize()
            ts.append(time.perf_counter())
        torch.cuda.synchronize()
        ts.append(time.perf_counter())
        glm_irls.fit_poisson(X, y, alpha=1.0, iters=8, callback=cb)
        return np.diff(ts)[1:] * 1e3

    class TwoCalls:                       # the loop as it was: sandwich, then transpose_matvec
        shape, dtype = mat.shape, mat.dtype
        matvec = staticmethod(mat.matvec)

        @staticmethod
        def sandwich_and_transpose_matvec(dd, vv):
            return mat.sandwich(dd), mat.transpose_matvec(vv)

    a, b = [], []
    for _ in range(2):
        a += list(irls_ms(mat))
        b += list(irls_ms(TwoCalls))
    print(f"IRLS iteration (matvec + products + solve), median ms: fused {np.median(a):.2f}, two calls {np.median(b):.2f}")


if __name__ == "__main__":
    main()
