"""Main-kernel time (the library's event pair, minimum of six) of the slab-family K3 kernels the benchmark does not
reach: slab with a C- and an F-ordered B of 64 columns, ell (64 columns), ellw and lg (128 columns), on a
2M x 512 sparse block at 5 % density, f64."""
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from tabmat_amd import _lib, synth  # noqa: E402
from tabmat_amd.ext import sparse as xs  # noqa: E402

n = int(os.environ.get("N", 2_000_000))
sm = synth.sparse_block(n, 512, 0.05, torch.float64, 1003)
d = torch.rand(n, dtype=torch.float64, device="cuda")
b64c = synth.dense_block(n, 64, torch.float64, 3)._dev_c()
b64f = synth.dense_block(n, 64, torch.float64, 3, order="F")._dev()
assert b64f.order_f == 1 and b64c.order_f == 0
b128 = synth.dense_block(n, 128, torch.float64, 4)._dev_c()
cases = [("slab C 64", lambda: xs.csr_dense_sandwich_slab(sm._slab(), b64c, d)),
         ("slab F 64", lambda: xs.csr_dense_sandwich_slab(sm._slab(), b64f, d)),
         ("ell 64", lambda: xs.csr_dense_sandwich_ell(sm._ell(), b64c, d)),
         ("ellw 128", lambda: xs.csr_dense_sandwich_ell(sm._ell(wide=True), b128, d)),
         ("lg 128", lambda: xs.csr_dense_sandwich_lg(sm._lg(), b128, d))]
_lib.call("tm_profile_enable", 1)
for name, run in cases:
    ts = []
    for _ in range(6):
        run()
        ms = C.c_float(0)
        _lib.call("tm_profile_last_ms", C.byref(ms))
        ts.append(ms.value)
    print(f"K3 {name} f64: min {min(ts):.3f} ms  (all: {' '.join(f'{t:.3f}' for t in ts)})")
