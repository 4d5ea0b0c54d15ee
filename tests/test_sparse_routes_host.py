"""No GPU: the host decisions of SparseMatrix over CsrDevs of CPU tensors -- which way the self sandwich goes
(_sandwich_route), which kernel a dense operand gets (_dense_kernel), and that to_device pre-builds the twin that
kernel reads.  The expected names are what the predicates of ext/sparse.py and the thresholds of sparse_matrix.py say
for these designs (the designs of tests/test_gpu_sparse_dispatch.py, whose golden file shows the same choices as
launches); free device memory is patched to a constant."""
import os
import sys

import numpy as np
import pytest
import torch
from scipy import sparse as sps

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from test_k3_ent import _csr_cpu  # noqa: E402

N = 3001


@pytest.fixture(autouse=True)
def _plenty_of_memory(monkeypatch):
    from tabmat_amd import _device as D

    monkeypatch.setattr(D, "free_bytes", lambda device=None: 1 << 40)


def _block(m, density, seed, n=N):
    import tabmat_amd as tm

    S = sps.random(n, m, density=density, format="csr", random_state=np.random.default_rng(seed))
    return tm.SparseMatrix.from_device(_csr_cpu(S, np.float64))


def _verdicts(X):
    from tabmat_amd.ext import sparse as xs

    A = X._dev()
    return xs.pairs_sandwich_pays(A), xs.direct_sandwich_pays(A), xs.blocks_sandwich_pays(A)


def test_self_sandwich_routes(monkeypatch):
    import tabmat_amd.categorical_matrix as cmod
    import tabmat_amd.sparse_matrix as spm
    from tabmat_amd.ext import sparse as xs

    X = _block(90, 0.1, 21)                                   # 9 entries per row and chunk: above 4.5
    assert _verdicts(X) == (False, False, True)
    assert X._sandwich_route() == "blocks"
    assert X._sandwich_route(n_rows=N // 3) == "rows"         # at most ROW_LIST_FRACTION of the rows
    assert X._sandwich_route(n_rows=int(0.7 * N)) == "blocks"
    assert not X._narrow_pays(17) and X._sandwich_route(n_cols=17) == "blocks"
    X._narrow_pays = lambda w: True
    assert X._sandwich_route(n_cols=17) == "narrow" and X._sandwich_route(N // 3, 17) == "narrow"
    assert X._sandwich_route(n_cols=45) == "blocks"           # not under half of the columns
    X = _block(90, 0.02, 21)
    assert _verdicts(X) == (False, False, False) and X._sandwich_route() == "chunked"
    X = _block(2000, 0.001, 24)
    assert _verdicts(X)[:2] == (False, True)
    assert X._sandwich_route() == "direct" and X._sandwich_route(N // 5, 300) == "direct"
    Z = _block(90, 0.0, 0)
    assert Z._sandwich_route() == "generic" and Z._sandwich_route(N // 2, 17) == "generic"
    monkeypatch.setattr(xs, "K2_PAIRS", "0")
    X = _block(5000, 0.02, 25, n=500)                         # more than 32 column chunks
    assert _verdicts(X) == (False, False, False) and X._sandwich_route() == "generic"
    monkeypatch.setattr(xs, "K2_PAIRS", "1")
    X = _block(600, 0.05, 27)
    assert xs.pairs_sandwich_pays(X._dev())
    assert X._sandwich_route() == "pairs" and X._sandwich_route(n_cols=200) == "pairs"
    assert X._sandwich_route(n_rows=N // 2) == "pairs"        # above 0.3 n: a masked d on the stream
    assert X._sandwich_route(n_rows=N // 5) == "rows"
    monkeypatch.setattr(xs, "K2_PAIRS", "auto")
    assert not xs.pairs_sandwich_pays(X._dev())               # (the model asks for about a million rows)
    monkeypatch.setattr(cmod, "DETERMINISTIC", True)
    X = _block(90, 0.1, 21)
    assert X._sandwich_route() == "deterministic" and X._sandwich_route(N // 3, 17) == "deterministic"
    assert X._sandwich_route(deterministic=False) == "blocks"
    assert Z._sandwich_route() == "generic"
    monkeypatch.setattr(spm, "PART_NNZ", int(X._dev().data.numel()) // 3)
    X = _block(90, 0.1, 21)
    assert X._sandwich_route() == "parts" and len(X._row_parts()) >= 3


def _operand(width, order_f=0):
    from tabmat_amd.ext._types import DenseDev

    return DenseDev(torch.zeros((width, N) if order_f else (N, width), dtype=torch.float64), N, width, order_f)


def _kernel_for(X, B, n_rows=None):
    from tabmat_amd.ext import sparse as xs

    return X._dense_kernel(B.m, xs.ell_supported(B), n_rows)


def test_sparse_x_dense_kernels():
    import tabmat_amd.sparse_matrix as spm

    X = _block(90, 0.1, 21)
    assert _kernel_for(X, _operand(100)) == "ent"
    assert _kernel_for(X, _operand(40)) == "ell"
    assert _kernel_for(X, _operand(101)) == "slab"            # rows of 808 bytes: not 16-byte aligned
    assert _kernel_for(X, _operand(100, order_f=1)) == "slab"
    assert _kernel_for(X, _operand(100), N // 5) == "rows"    # at most ROW_LIST_FRACTION_K3 of the rows
    assert _kernel_for(X, _operand(100), N // 2) == "ent"
    W = _block(1500, 0.003, 31)
    assert int(W._dev().data.numel()) <= spm.SORTED_K3_NNZ_PER_ROW * N
    assert _kernel_for(W, _operand(100)) == "sorted" and _kernel_for(W, _operand(100), N // 2) == "sorted"
    assert _kernel_for(W, _operand(101)) == "slab" and _kernel_for(W, _operand(100), N // 5) == "rows"
    X._ent = lambda: None
    assert _kernel_for(X, _operand(100)) == "lg"
    X._lg = lambda: None
    assert _kernel_for(X, _operand(100)) == "ellw"
    assert _kernel_for(_block(90, 0.0, 0), _operand(100)) == "generic"


@pytest.mark.parametrize("density", [0.1, 0.02])
@pytest.mark.parametrize("width", [1, 40, 64, 65, 100, 101])
def test_to_device_builds_the_twin_the_product_reads(width, density, monkeypatch):
    """to_device knows a width, not an operand: it assumes the C-ordered, 16-byte aligned one.  What it builds is the
    twin _dense_kernel names for that operand (the function the product asks), and the slab form beside it unless
    that is the entry twin -- nothing else."""
    from tabmat_amd.ext import _types as T

    built = []
    for cls, name in ((T.SlabEnt, "ent"), (T.SlabLg, "lg"), (T.SlabEll, "ell"), (T.SlabCsc, "slab")):
        def from_csr(*a, _fn=cls.from_csr, _name=name, **kw):
            twin = _fn(*a, **kw)
            built.append(_name + ("w" if getattr(twin, "wide", False) else ""))
            return twin

        monkeypatch.setattr(cls, "from_csr", staticmethod(from_csr))
    X = _block(90, density, 21)
    X.to_device(dense_width=width)
    want = "ell" if width <= 64 else "ent"                    # (no small block is refused by either twin)
    assert sorted(built) == sorted({want, "slab"} - ({"slab"} if want == "ent" else set()))
    del built[:]
    assert X._dense_kernel(width) == want and not built       # the product's choice, and it builds nothing more
    if width in (40, 64, 100):                                # (widths an aligned float64 operand can have)
        assert _kernel_for(X, _operand(width)) == want
