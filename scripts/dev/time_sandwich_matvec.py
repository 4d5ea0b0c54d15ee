"""sandwich_matvec (one pass over the dense block, tm_dense_sandwich_matvec_*) against the composition
transpose_matvec(d * matvec(u)).  Device vectors, a synchronize around every call, interleaved A / B in one
process, min / median of >= 16 calls after warm-up.  Also the dense matvec alone (the bar for the fused kernel:
within 1.2x of it at 10M x 128).

    python scripts/dev/time_sandwich_matvec.py [rows]        # default 10M
"""
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
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


def ab(title, mat, rounds=8):
    n, p = mat.shape
    tdt = torch.float64 if mat.dtype == np.float64 else torch.float32
    g = torch.Generator(device="cuda").manual_seed(0)
    d = torch.rand(n, dtype=tdt, device="cuda", generator=g)
    u = torch.randn(p, dtype=tdt, device="cuda", generator=g)
    runs = {
        "sandwich_matvec": lambda: mat.sandwich_matvec(d, u),
        "transpose_matvec(d * matvec(u))": lambda: mat.transpose_matvec(d * mat.matvec(u)),
        "matvec alone": lambda: mat.matvec(u),
    }
    for fn in runs.values():
        wall(fn, 3)
    res = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            res[k] += wall(fn, 2)
    a = np.asarray(res["sandwich_matvec"])
    b = np.asarray(res["transpose_matvec(d * matvec(u))"])
    mv = np.asarray(res["matvec alone"])
    print(f"{title}: ms per call (min / median of {len(a)})")
    for k, ts in res.items():
        print(f"  {k:34s} {min(ts):7.3f} / {float(np.median(ts)):7.3f}")
    print(f"  fused / composition (median) = {np.median(a) / np.median(b):.3f};  "
          f"fused / matvec (median) = {np.median(a) / np.median(mv):.3f}", flush=True)


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 10_000_000
    for k, dt in [(128, torch.float64), (128, torch.float32), (512, torch.float64)]:
        X = synth.dense_block(n, k, dt, 3)
        ab(f"DenseMatrix {n} x {k} {str(dt).replace('torch.', '')}", X)
        del X
        torch.cuda.empty_cache()
    mat = synth.mixed_split(n)
    mat.to_device()
    ab(f"configs[3] SplitMatrix, n = {n}", mat)


if __name__ == "__main__":
    main()
