"""-m gpu: WHICH tm_* entry points a product call reaches, in what order and with which scalar arguments, pinned
against tests/golden/sandwich_dispatch.json.  The kernels are tested product by product elsewhere; this file pins the
host code in between (SplitMatrix._sandwich_dev and its phases, the matvec / transpose_matvec assembly): a change that
reroutes a design to another kernel, or adds, drops or reorders a launch, shows up as a diff of the golden file.

How a call is traced: for its duration every tm_* attribute of the ctypes handle is wrapped (monkeypatch.setattr, on top
of the conftest spy, which keeps counting) and (name, scalar arguments) is appended to a list.  Scalar = every argument
whose prototype type is not a pointer; pointers and the stream are left out.  Entry points WITHOUT any pointer argument
are not recorded at all: they take no stream and no buffer, so they launch nothing -- they are size queries whose
results the callers cache per process, which would make the record depend on what ran before.  Every call is made
twice and both records are kept (the int8 syrk's history changes the second call's launches).

Every sandwich result is also compared with the float64 numpy image of the design at the natural scale (nat_err):
1e-10 for float64 designs, the fuzz net's 2e-3 for float32 blocks.

Re-recording (after a change that is MEANT to move launches):
    python tests/test_gpu_sandwich_dispatch.py --commit <hash of the commit recorded> [--out FILE]
records every case twice, drops the scalar positions that differ between the two recordings (listed per symbol under
"dropped"), refuses a case whose two recordings disagree on the names, and writes the file.  The module uses the public
API and the module constants other tests patch, nothing else, so it runs unchanged on the commit before a refactor."""
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
from scipy import sparse as sps

HERE = os.path.dirname(os.path.abspath(__file__))
for _p in (HERE, os.path.dirname(HERE)):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import _cases as cs  # noqa: E402
from _gpu_util import nat_err, to_tm_split  # noqa: E402

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(HERE, "golden", "sandwich_dispatch.json")
F64_TOL, F32_TOL = 1e-10, 2e-3          # nat_err bounds of tests/test_gpu_fuzz.py


def _scalar(a):
    a = getattr(a, "value", a)
    return float(a) if isinstance(a, float) else int(a)


def _host(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class Tracer:
    """calls[label] = [first call, second call], each a list of (name, {argument position: scalar})."""

    def __init__(self, mp):
        self.mp = mp                    # a pytest.MonkeyPatch
        self.calls = {}

    def spy(self, seq):
        """Context: every tm_* attribute of the handle appends to `seq` before it runs."""
        from tabmat_amd import _lib

        handle = _lib.lib()
        ctx = self.mp.context()
        m = ctx.__enter__()
        for name, types in _lib.prototypes().items():
            if C.c_void_p not in types:
                continue                # no stream, no buffer: a size query (see the module docstring)
            keep = [k for k, t in enumerate(types) if t is not C.c_void_p]

            def spy(*args, _fn=getattr(handle, name), _name=name, _keep=keep):
                seq.append((_name, {k: _scalar(args[k]) for k in _keep}))
                return _fn(*args)

            m.setattr(handle, name, spy)
        return ctx

    def call(self, label, fn, want=None, tol=F64_TOL):
        """Run fn() twice under the spy; want: the float64 image of a sandwich result (checked both times)."""
        assert label not in self.calls, label
        seqs = []
        for _ in range(2):
            seq = []
            ctx = self.spy(seq)
            try:
                res = fn()
            finally:
                ctx.__exit__(None, None, None)
            seqs.append(seq)
            if want is not None:
                err = nat_err(_host(res), want)
                assert err < tol, (label, err)
        self.calls[label] = seqs
        return res


def _sand(E, d, rows=None, cols=None):
    d = np.asarray(d, dtype=np.float64)
    if rows is not None:
        E, d = E[np.asarray(rows, dtype=np.int64)], d[np.asarray(rows, dtype=np.int64)]
    if cols is not None:
        E = E[:, np.asarray(cols, dtype=np.int64)]
    return E.T @ (d[:, None] * E)


def _cat(codes, ncat, dtype=np.float64, drop=False):
    import tabmat_amd as tm

    oh = np.zeros((len(codes), ncat))
    oh[np.arange(len(codes)), codes] = 1.0
    return tm.CategoricalMatrix(codes, categories=np.arange(ncat), drop_first=drop, dtype=dtype), oh[:, int(drop):]


def _sorted_choice(rng, n, k):
    return np.sort(rng.choice(n, size=k, replace=False)).astype(np.int32)


# ---- the cases -------------------------------------------------------------------------------------------------
def _mixed(t, dtype):
    n = 3001
    tol = F64_TOL if dtype == np.float64 else F32_TOL
    specs, idx = cs.mixed_specs(n, 40, 90, (30, 7, 120), seed=0, dtype=dtype, missing=True, drop_first=True)
    X = to_tm_split(specs, idx, dtype)
    E = np.hstack([cs.spec_toarray(s) for s in specs])
    p = E.shape[1]
    rng = np.random.default_rng(1)
    d = rng.random(n).astype(dtype)
    v = rng.standard_normal(p).astype(dtype)
    w = rng.standard_normal(n).astype(dtype)
    rows = _sorted_choice(rng, n, n // 3)
    short = _sorted_choice(rng, n, n // 30)
    c17 = _sorted_choice(rng, p, 17)
    c70 = _sorted_choice(rng, p, int(0.7 * p))
    t.call("sandwich", lambda: X.sandwich(d), _sand(E, d), tol)
    t.call("sandwich rows/3", lambda: X.sandwich(d, rows), _sand(E, d, rows), tol)
    t.call("sandwich rows/30", lambda: X.sandwich(d, short), _sand(E, d, short), tol)
    t.call("sandwich cols17", lambda: X.sandwich(d, cols=c17), _sand(E, d, None, c17), tol)
    t.call("sandwich cols70%", lambda: X.sandwich(d, cols=c70), _sand(E, d, None, c70), tol)
    t.call("sandwich cols=all", lambda: X.sandwich(d, cols=np.arange(p)), _sand(E, d), tol)
    t.call("matvec", lambda: X.matvec(v))
    t.call("matvec cols17", lambda: X.matvec(v, c17))
    t.call("transpose_matvec", lambda: X.transpose_matvec(w))
    t.call("transpose_matvec rows/3 cols17", lambda: X.transpose_matvec(w, rows, c17))
    t.call("sandwich_matvec", lambda: X.sandwich_matvec(d, v))
    t.call("sandwich_matvec rows/3 cols17", lambda: X.sandwich_matvec(d, v[c17], rows, c17))
    t.call("sandwich_diag", lambda: X.sandwich_diag(d))
    t.call("sandwich_diag rows/3 cols17", lambda: X.sandwich_diag(d, rows, c17))
    beta = (0.01 * v).astype(dtype)
    y = rng.poisson(1.0, n).astype(dtype)
    t.call("glm_loss_grad poisson", lambda: X.glm_loss_grad("poisson", beta, y))
    t.call("glm_loss_grad poisson weights offset", lambda: X.glm_loss_grad("poisson", beta, y, d, (0.01 * w).astype(dtype)))


def case_mixed_f64(t):
    _mixed(t, np.float64)


def case_mixed_f32(t):
    _mixed(t, np.float32)


def case_int8_dense(t):
    """C-ordered float64 dense block of 128 columns over more than 4096 rows: the int8 syrk and the forms of it that
    carry a second vector (X' v, X' d) or the column centres."""
    import tabmat_amd as tm

    n = 5003
    rng = np.random.default_rng(2)
    A = rng.standard_normal((n, 128))
    S = sps.random(n, 200, density=0.05, format="csc", random_state=rng)
    c1, o1 = _cat(rng.integers(0, 6, n), 6)
    c2, o2 = _cat(rng.integers(0, 11, n), 11)
    X = tm.SplitMatrix([tm.DenseMatrix(A), tm.SparseMatrix(S), c1, c2])
    E = np.hstack([A, S.toarray(), o1, o2])
    p = E.shape[1]
    d = rng.random(n)
    v = rng.standard_normal(n)
    rows = _sorted_choice(rng, n, n // 2)
    cols = _sorted_choice(rng, p, 25)
    t.call("sandwich", lambda: X.sandwich(d), _sand(E, d))
    t.call("sandwich_and_transpose_matvec", lambda: X.sandwich_and_transpose_matvec(d, v)[0], _sand(E, d))
    t.call("sandwich_and_transpose_matvec rows/2", lambda: X.sandwich_and_transpose_matvec(d, v, rows)[0],
           _sand(E, d, rows))
    shift, mult = rng.standard_normal(p), rng.random(p) + 0.5
    Sm = tm.StandardizedMatrix(X, shift, mult)
    Es = E * mult + shift
    t.call("standardized sandwich", lambda: Sm.sandwich(d), _sand(Es, d))
    t.call("standardized sandwich rows/2", lambda: Sm.sandwich(d, rows), _sand(Es, d, rows))
    t.call("standardized sandwich cols25", lambda: Sm.sandwich(d, cols=cols), _sand(Es, d, None, cols))
    c70 = _sorted_choice(rng, p, int(0.7 * p))
    t.call("standardized sandwich cols70%", lambda: Sm.sandwich(d, cols=c70), _sand(Es, d, None, c70))
    # without a complete categorical the dense block's column sums come out of its own syrk pass
    c3, o3 = _cat(rng.integers(0, 9, n), 9, drop=True)
    Xi = tm.SplitMatrix([tm.DenseMatrix(A), tm.SparseMatrix(S), c3])
    Ei = np.hstack([A, S.toarray(), o3])
    Si = tm.StandardizedMatrix(Xi, shift[:Ei.shape[1]], mult[:Ei.shape[1]])
    Eis = Ei * mult[:Ei.shape[1]] + shift[:Ei.shape[1]]
    ci = _sorted_choice(rng, Ei.shape[1], 25)
    t.call("no complete categorical: standardized sandwich", lambda: Si.sandwich(d), _sand(Eis, d))
    t.call("no complete categorical: standardized sandwich cols25", lambda: Si.sandwich(d, cols=ci),
           _sand(Eis, d, None, ci))


def case_wide_selection(t):
    """More selected dense + sparse columns than NARROW_COLS, under half of p, a small unselected share: "wide"."""
    import tabmat_amd as tm

    n = 3001
    rng = np.random.default_rng(3)
    A = rng.standard_normal((n, 140))
    S = sps.random(n, 200, density=0.05, format="csc", random_state=rng)
    c1, o1 = _cat(rng.integers(0, 500, n), 500)
    X = tm.SplitMatrix([tm.DenseMatrix(A), tm.SparseMatrix(S), c1])
    E = np.hstack([A, S.toarray(), o1])
    d = rng.random(n)
    cols = np.concatenate([_sorted_choice(rng, 140, 130), 140 + _sorted_choice(rng, 200, 20)]).astype(np.int32)
    t.call("sandwich cols130+20", lambda: X.sandwich(d, cols=cols), _sand(E, d, None, cols))
    shift = rng.standard_normal(E.shape[1])
    Sm = tm.StandardizedMatrix(X, shift)
    t.call("standardized sandwich cols130+20", lambda: Sm.sandwich(d, cols=cols), _sand(E + shift, d, None, cols))


def case_heavy_block_skipped(t):
    """The design and selection of test_column_selection_skips_unselected_heavy_blocks: the generic restricted path."""
    import tabmat_amd as tm

    rng = np.random.default_rng(11)
    n = 6000
    A = rng.standard_normal((n, 140))
    S = sps.random(n, 60, density=0.1, format="csc", random_state=rng)
    big = rng.integers(0, 9000, n)
    small = rng.integers(0, 7, n)
    X = tm.SplitMatrix([tm.DenseMatrix(A), tm.SparseMatrix(S), tm.CategoricalMatrix(big, categories=np.arange(9000)),
                        tm.CategoricalMatrix(small, categories=np.arange(7))])
    p = X.shape[1]
    cols = np.concatenate([np.arange(200), np.arange(200 + 9000, p)]).astype(np.int32)
    d = rng.random(n)
    E = np.hstack([A, S.toarray(), np.eye(7)[small]])
    rows = _sorted_choice(rng, n, n // 2)
    t.call("sandwich cols", lambda: X.sandwich(d, cols=cols), _sand(E, d))
    t.call("sandwich rows/2 cols", lambda: X.sandwich(d, rows, cols), _sand(E, d, rows))
    Sm = tm.StandardizedMatrix(X, rng.standard_normal(p))
    t.call("standardized sandwich cols", lambda: Sm.sandwich(d, cols=cols), _sand(E + Sm.shift[cols], d))


def case_big_categoricals(t):
    """Two categoricals with more levels than FUSED_LEVELS, a small one, and a narrow dense block of odd width."""
    import tabmat_amd as tm

    n = 3001
    rng = np.random.default_rng(4)
    A = rng.standard_normal((n, 5))
    c1, o1 = _cat(rng.integers(0, 1000, n), 1000)
    c2, o2 = _cat(rng.integers(0, 1000, n), 1000)
    c3, o3 = _cat(rng.integers(0, 7, n), 7, drop=True)
    X = tm.SplitMatrix([tm.DenseMatrix(A), c1, c2, c3])
    E = np.hstack([A, o1, o2, o3])
    d = rng.random(n)
    rows = _sorted_choice(rng, n, n // 3)
    t.call("sandwich", lambda: X.sandwich(d), _sand(E, d))
    t.call("sandwich rows/3", lambda: X.sandwich(d, rows), _sand(E, d, rows))
    Sm = tm.StandardizedMatrix(X, rng.standard_normal(E.shape[1]))
    t.call("standardized sandwich", lambda: Sm.sandwich(d), _sand(E + Sm.shift, d))


def case_twelve_categoricals(t):
    """Categorical blocks only: the fused pair tables, then pair by pair, then the deterministic histograms."""
    import tabmat_amd as tm
    import tabmat_amd.categorical_matrix as cmod
    import tabmat_amd.split_matrix as smod

    n = 2000
    rng = np.random.default_rng(5)
    levels = [2, 3, 5, 12, 40, 7, 4, 9, 16, 3, 25, 6]
    blocks = [_cat(rng.integers(0, k, n), k, drop=bool(b % 3 == 1)) for b, k in enumerate(levels)]
    X = tm.SplitMatrix([b for b, _ in blocks])
    E = np.hstack([o for _, o in blocks])
    p = E.shape[1]
    d = rng.random(n)
    rows = _sorted_choice(rng, n, n // 3)
    cols = _sorted_choice(rng, p, p // 3)

    def trace(tag):
        t.call(tag + "sandwich", lambda: X.sandwich(d), _sand(E, d))
        t.call(tag + "sandwich rows/3 cols/3", lambda: X.sandwich(d, rows, cols), _sand(E, d, rows, cols))
        t.call(tag + "transpose_matvec", lambda: X.transpose_matvec(d))

    trace("")
    with t.mp.context() as m:
        m.setattr(smod, "CAT_PAIRS_FUSED", False)
        trace("CAT_PAIRS_FUSED off: ")
    with t.mp.context() as m:
        m.setattr(cmod, "DETERMINISTIC", True)
        trace("DETERMINISTIC: ")


def case_onehot_slab(t):
    """An F-ordered dense block without its row-major twin: the categorical x dense terms through the one-hot slab."""
    import tabmat_amd as tm
    import tabmat_amd.dense_matrix as dmod

    n = 3001
    rng = np.random.default_rng(6)
    A = np.asfortranarray(rng.standard_normal((n, 200)))
    blocks = [_cat(rng.integers(0, k, n), k) for k in (10, 20, 30)]
    E = np.hstack([A] + [o for _, o in blocks])
    d = rng.random(n)
    rows = _sorted_choice(rng, n, n // 3)
    with t.mp.context() as m:
        m.setattr(dmod, "ROW_MAJOR_TWIN", False)
        X = tm.SplitMatrix([tm.DenseMatrix(A)] + [b for b, _ in blocks])
        t.call("sandwich", lambda: X.sandwich(d), _sand(E, d))
        t.call("sandwich rows/3", lambda: X.sandwich(d, rows), _sand(E, d, rows))


def case_row_parts(t):
    """A sparse block at three times PART_NNZ: the sandwich as a sum over row parts."""
    import tabmat_amd as tm
    import tabmat_amd.sparse_matrix as spm

    n = 4000
    specs, idx = cs.mixed_specs(n, 64, 120, (12,), seed=4, drop_first=True)
    E = np.hstack([cs.spec_toarray(s) for s in specs])
    p = E.shape[1]
    rng = np.random.default_rng(7)
    d = rng.random(n)
    rows = _sorted_choice(rng, n, n // 3)
    first = _sorted_choice(rng, n // 4, n // 40)          # (leaves the later parts without a row)
    cols = np.sort(np.concatenate([rng.choice(184, 30, replace=False), 184 + np.arange(5)])).astype(np.int32)
    shift, mult = rng.standard_normal(p), rng.random(p) + 0.5
    Es = E * mult + shift
    with t.mp.context() as m:
        m.setattr(spm, "PART_NNZ", specs[1][1].nnz // 3)
        X = to_tm_split(specs, idx)
        assert X._parts() is not None and len(X._parts()) >= 3
        Sm = tm.StandardizedMatrix(X, shift, mult)
        t.call("sandwich", lambda: X.sandwich(d), _sand(E, d))
        t.call("sandwich rows/3", lambda: X.sandwich(d, rows), _sand(E, d, rows))
        t.call("sandwich rows in the first part", lambda: X.sandwich(d, first), _sand(E, d, first))
        t.call("standardized sandwich", lambda: Sm.sandwich(d), _sand(Es, d))
        t.call("standardized sandwich rows/3", lambda: Sm.sandwich(d, rows), _sand(Es, d, rows))
        t.call("standardized sandwich cols35", lambda: Sm.sandwich(d, cols=cols), _sand(Es, d, None, cols))
        t.call("sandwich_diag", lambda: X.sandwich_diag(d))
        t.call("sandwich_diag rows/3 cols35", lambda: X.sandwich_diag(d, rows, cols))


def case_graph_capture(t):
    """sandwich_graph with a column selection: the capture is traced, the replay equals sandwich."""
    import torch

    n = 3001
    specs, idx = cs.mixed_specs(n, 40, 90, (30, 7), seed=8)
    X = to_tm_split(specs, idx)
    E = np.hstack([cs.spec_toarray(s) for s in specs])
    rng = np.random.default_rng(8)
    d = rng.random(n)
    dd = torch.as_tensor(d, device="cuda")
    for tag, cols in (("cols40%", _sorted_choice(rng, E.shape[1], int(0.4 * E.shape[1]))),
                      ("cols70%", _sorted_choice(rng, E.shape[1], int(0.7 * E.shape[1])))):
        g = t.call("sandwich_graph " + tag, lambda: X.sandwich_graph(dd, cols=cols))
        replay = _host(g(dd)).copy()
        want = _sand(E, d, None, cols)
        assert nat_err(replay, want) < F64_TOL
        assert nat_err(replay, X.sandwich(d, cols=cols)) < F64_TOL


def _fuzz(t, seed):
    """The four sandwich calls of test_gpu_fuzz.test_random_split_products on its design number `seed`."""
    from test_gpu_fuzz import _random_split

    rng = np.random.default_rng(1000 + seed)
    dtype = np.float64 if seed % 4 else np.float32
    tol = F64_TOL if dtype == np.float64 else F32_TOL
    X, E = _random_split(rng, dtype)
    if X is None:
        return
    n, p = E.shape
    d = rng.random(n).astype(dtype)
    d[rng.random(n) < 0.1] = 0.0
    rng.standard_normal(p), rng.standard_normal(n)          # (the draws of v and w there)
    rows = np.sort(rng.choice(n, size=max(1, n // 2), replace=False)).astype(np.int32)
    cols = np.sort(rng.choice(p, size=max(1, (2 * p) // 3), replace=False)).astype(np.int32)
    few_c = np.sort(rng.choice(p, size=max(1, p // 5), replace=False)).astype(np.int32)
    few = rng.choice(n, size=max(1, n // 9), replace=False).astype(np.int64)
    t.call("sandwich", lambda: X.sandwich(d), _sand(E, d), tol)
    t.call("sandwich rows/2 cols2/3", lambda: X.sandwich(d, rows, cols), _sand(E, d, rows, cols), tol)
    t.call("sandwich cols/5", lambda: X.sandwich(d, None, few_c), _sand(E, d, None, few_c), tol)
    t.call("sandwich rows/9", lambda: X.sandwich(d, few), _sand(E, d, few), tol)


CASES = {f.__name__[5:]: f for f in (
    case_mixed_f64, case_mixed_f32, case_int8_dense, case_wide_selection, case_heavy_block_skipped,
    case_big_categoricals, case_twelve_categoricals, case_onehot_slab, case_row_parts, case_graph_capture)}
for _seed in range(8):
    CASES[f"fuzz_{_seed}"] = (lambda t, _s=_seed: _fuzz(t, _s))


def record(case, mp, cases=CASES):
    t = Tracer(mp)
    cases[case](t)
    return t.calls


def _encode(seq, dropped):
    """One traced call as a list of strings "name pos=value ..." (a dropped position shows as pos=*)."""
    return [" ".join([name] + [f"{k}={'*' if k in dropped.get(name, ()) else repr(v)}" for k, v in sc.items()])
            for name, sc in seq]


# ---- the test --------------------------------------------------------------------------------------------------
_golden = {}


def _load(path=GOLDEN):
    if path not in _golden:
        with open(path) as f:
            _golden[path] = json.load(f)
    return _golden[path]


# one test per group of cases (a case is one design; the golden file is keyed by case)
GROUPS = {"mixed": ["mixed_f64", "mixed_f32"],
          "designs": ["int8_dense", "wide_selection", "heavy_block_skipped", "big_categoricals", "twelve_categoricals",
                      "onehot_slab", "row_parts", "graph_capture"],
          "fuzz": [f"fuzz_{seed}" for seed in range(8)]}
assert sorted(c for g in GROUPS.values() for c in g) == sorted(CASES)


def _check_case(case, mp, cases=CASES, golden=GOLDEN):
    """(cases / golden: another module's case table and golden file -- tests/test_gpu_sparse_dispatch.py)"""
    gold = _load(golden)
    assert case in gold["cases"], f"{case} is not in the golden file (dropped there as data-dependent?)"
    want = gold["cases"][case]
    got = record(case, mp, cases)
    assert list(got) == list(want), case
    for label, seqs in got.items():
        for k, seq in enumerate(seqs):
            have = _encode(seq, gold["dropped"])
            ref = [gold["launches"][i] for i in want[label][k]]
            assert have == ref, f"{case} / {label} / call {k + 1}: first difference at launch " \
                f"{next((i for i, (a, b) in enumerate(zip(have, ref)) if a != b), min(len(have), len(ref)))}"


@pytest.mark.parametrize("group", list(GROUPS))
def test_sandwich_dispatch(group, monkeypatch):
    for case in GROUPS[group]:
        with monkeypatch.context() as mp:       # (what a case patches is undone before the next one)
            _check_case(case, mp)


# ---- the recorder ----------------------------------------------------------------------------------------------
def _record_all(cases=CASES):
    out = {}
    for case in cases:
        mp = pytest.MonkeyPatch()
        try:
            out[case] = record(case, mp, cases)
        finally:
            mp.undo()
        print(f"recorded {case}: {sum(len(s) for v in out[case].values() for s in v)} launches", flush=True)
    return out


def main(argv, cases=CASES, golden=GOLDEN):
    import argparse
    import subprocess

    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", help="hash of the commit this is recorded on (default: git rev-parse HEAD)")
    ap.add_argument("--out", default=golden)
    a = ap.parse_args(argv)
    commit = a.commit or subprocess.check_output(["git", "rev-parse", "HEAD"], cwd=HERE, text=True).strip()
    first, second = _record_all(cases), _record_all(cases)
    dropped, unstable = {}, []
    for case in cases:
        names = [[[n for n, _ in s] for s in seqs] for seqs in first[case].values()]
        if names != [[[n for n, _ in s] for s in seqs] for seqs in second[case].values()]:
            unstable.append(case)
            continue
        for label in first[case]:
            for sa, sb in zip(first[case][label], second[case][label]):
                for (name, xa), (_, xb) in zip(sa, sb):
                    for k in xa:
                        if xa[k] != xb[k]:
                            dropped.setdefault(name, set()).add(k)
    dropped = {k: sorted(v) for k, v in sorted(dropped.items())}
    table, recorded = {}, {}
    for case in cases:
        if case in unstable:
            continue
        recorded[case] = {label: [[table.setdefault(s, len(table)) for s in _encode(seq, dropped)] for seq in seqs]
                       for label, seqs in first[case].items()}
    lines = ["{", f' "parent": {json.dumps(commit)},', f' "dropped": {json.dumps(dropped)},', ' "launches": [']
    lines += [f"  {json.dumps(s)}," for s in table]
    lines[-1] = lines[-1][:-1]
    lines += [" ],", ' "cases": {']
    for case, labels in recorded.items():
        lines.append(f"  {json.dumps(case)}: {{")
        lines += [f"   {json.dumps(label)}: {json.dumps(seqs, separators=(',', ':'))}," for label, seqs in labels.items()]
        if labels:
            lines[-1] = lines[-1][:-1]
        lines.append("  },")
    lines[-1] = lines[-1][:-1]
    lines += [" }", "}"]
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    json.load(open(a.out))
    print(f"wrote {a.out}: {len(table)} distinct launches, dropped scalar positions {dropped}, "
          f"cases dropped as data-dependent {unstable}")


if __name__ == "__main__":
    main(sys.argv[1:])
