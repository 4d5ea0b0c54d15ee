"""The entry twin's slab decode over LONG row ranges (tabmat_amd/ext/_types.py::SlabEnt; csrc/sparse_ent.hip `expand`,
csrc/cat_multi.hip `load_rows`).

A slot carries `slab & 63`; the kernels rebuild the slab of all 64 slots of a step against ONE running slab, taken
over from the step's last slot.  That is right only if the five batches a step sees -- the last one of the step before
and its own four -- span at most 63 slabs, whatever slab the range starts at.  The builder guarantees it with a
padding ("continuity") batch in an EMPTY block at every SlabEnt.CONT_PERIOD-th slab.  With a period of 32 (until this
file existed) two consecutive batches were close enough, five were not: a range of more than 64 slabs with an empty
stretch decoded its later entries to wrong rows, silently.  At the default launch a range is n / 64 / 256 slabs, so no
test at n <= 45 000 could see it.

Host part: a model of the kernels' decode (tests/_ent_stream.py) over every cut of the slabs into workgroup and wave
ranges, and the invariant on the stream alone.  With the 32-slab rule the model counts (real slots decoded to a wrong
row / real slots): far_apart-44805x48 one range 92 / 136, nblk = 9 48 / 136, nblk >= 16 0; random 128 000 x 40 @ 1e-4
in ranges of 100 slabs 6 / 512; 2 400 000 x 40 with entries only in the last slab of each 147-slab range, at the
default launch (nblk = 256): 11 220 / 11 264.  test_the_model_sees_the_32_slab_rule_fail pins that the model has teeth.

GPU part: the kernels at FORCED cuts (one workgroup over all slabs) against the oracle, and the public API at the
default launch at the size where the default cut is long enough."""
import numpy as np
import pytest
import torch
from scipy import sparse as sps

import _ent_stream as es
from tabmat_amd.ext._types import CsrDev, SlabEnt
from test_k3_ent import _catsparse_kernel  # noqa: F401  (fixture: forces the staged / the gather kernel)

gpu = pytest.mark.gpu
ALL = [d[0] for d in es.SMALL_DESIGNS + es.LARGE_DESIGNS]
SMALL = [d[0] for d in es.SMALL_DESIGNS]


def _twin_cpu(name, dtype=np.float64):
    S, max_pad = es.build_design(name)
    tw = SlabEnt.from_csr(es.csr_cpu(S, dtype), max_pad=max_pad)
    assert tw is not None, "the design must keep its twin (small streams are always built)"
    return S, tw


def _wrong_by_cut(st, every_s0):
    """{cut: wrong real slots} over all groups, for the cuts with at least one."""
    bad = {}
    cuts = es.all_cuts(st.S)
    if every_s0:
        cuts["every s0"] = [(s0, st.S, tail) for s0 in range(st.S) for tail in ("stream", "last")]
    for label, ranges in cuts.items():
        w = sum(es.wrong_real_slots(st, g, a, b, tail) for g in range(st.G) for a, b, tail in ranges)
        if w:
            bad[label] = w
    return bad


@pytest.mark.parametrize("name", ALL)
def test_kernel_decode_finds_every_real_slot(name):
    """Every slot with a non-zero value decodes -- by the KERNELS' rule, not with the slab taken from bstart -- to the
    (row, column) it holds in the matrix: for every group, every nblk in {1, 2, 3, 5, 9, 16, 64, 256}, each split again
    into 2 and 8 wave ranges, and for the small matrices every possible first slab."""
    S, tw = _twin_cpu(name)
    st = es.Stream(tw)
    # the stream read with the TRUE slabs is the matrix (so "true slab" below means the matrix's row)
    got = st.to_coo()
    assert got.shape == S.shape and (got != S).nnz == 0 and got.nnz == S.nnz
    assert int(st.real.sum()) == S.nnz
    bad = _wrong_by_cut(st, every_s0=name in SMALL)
    assert not bad, f"real slots decoded to a wrong row, of {S.nnz}: {bad}"


@pytest.mark.parametrize("name", ALL)
def test_builder_keeps_five_batches_within_63_slabs(name):
    """The contract of the stream, stated on bstart alone (include/tabmat_hip.h, tm_csr_dense_sandwich_ent_*): for every
    group and every slab s0 the first four batches at or after s0 lie in [s0, s0 + 63], and any five consecutive
    batches span at most 63 slabs."""
    _, tw = _twin_cpu(name)
    st = es.Stream(tw)
    for g in range(st.G):
        bs = st.batch_slabs(g)
        assert (np.diff(bs) >= 0).all()
        if len(bs) > 4:
            span = bs[4:] - bs[:-4]
            assert span.max() <= 63, (g, int(span.max()))
        s0 = np.arange(st.S)
        first = np.searchsorted(bs, s0, side="left")
        some = first < len(bs)                       # (behind the last batch: nothing to decode)
        fourth = np.minimum(first[some] + 3, len(bs) - 1)
        assert (bs[fourth] - s0[some] <= 63).all(), g
        if tw.vals.numel() > SlabEnt.SLACK:          # a matrix with entries: every group's stream starts in slab 0
            assert len(bs) and bs[0] == 0


def test_the_model_sees_the_32_slab_rule_fail(monkeypatch):
    """The rule this file replaced (a continuity batch at every 32nd slab) and the nearest one that still wraps (every
    16th: 4 x 16 = 64) must FAIL the model and the invariant -- else the two tests above prove nothing."""
    counts = {}
    for period in (32, 16, 15):
        monkeypatch.setattr(SlabEnt, "CONT_PERIOD", period)
        S, tw = _twin_cpu("far_apart-44805x48")
        st = es.Stream(tw)
        counts[period] = {nblk: sum(es.wrong_real_slots(st, g, a, b, "stream") for g in range(st.G)
                                    for a, b in es.block_ranges(st.S, nblk)) for nblk in (1, 9, 16)}
        spans = [int((st.batch_slabs(g)[4:] - st.batch_slabs(g)[:-4]).max()) for g in range(st.G)]
        assert (max(spans) > 63) == (period != 15), (period, spans)
    assert S.nnz == 136
    assert counts[32] == {1: 92, 9: 48, 16: 0}, counts
    assert counts[16][1] > 0, counts
    assert counts[15] == {1: 0, 9: 0, 16: 0}, counts


def test_stream_without_empty_blocks_does_not_depend_on_the_period(monkeypatch):
    """Continuity batches go into EMPTY blocks only: a design without one (BASELINE configs[3] is such a design) has the
    same stream, byte for byte, under the old rule and the new one."""
    S, _ = es.build_design("no_empty_block-5003x40")
    twins = {}
    for period in (32, 15):
        monkeypatch.setattr(SlabEnt, "CONT_PERIOD", period)
        twins[period] = SlabEnt.from_csr(es.csr_cpu(S, np.float64), max_pad=8.0)
    old, new = twins[32], twins[15]
    st = es.Stream(new)
    assert (np.diff(st.bst, axis=1) > 0).all()                   # no empty (group, slab) block at all
    for a, b in ((old.vals, new.vals), (old.meta, new.meta), (old.bstart, new.bstart), (old.inv, new.inv)):
        assert a.dtype == b.dtype and a.shape == b.shape
        assert a.numpy().tobytes() == b.numpy().tobytes()


# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def tune():
    """tune(knob=value, ...) sets launcher knobs through tm_tune_set; all of them are reset (-2**63) afterwards."""
    from tabmat_amd import _lib

    touched = []

    def set_(**kw):
        for k, v in kw.items():
            if v is None:
                continue                              # None = the launcher's default
            touched.append(k)
            _lib.call("tm_tune_set", k.encode(), int(v))

    try:
        yield set_
    finally:
        for k in touched:
            _lib.call("tm_tune_set", k.encode(), -2**63)


def _csr_gpu(S, dtype):
    S = sps.csr_matrix(S).astype(dtype)
    S.sort_indices()
    return CsrDev(torch.from_numpy(S.data.copy()).cuda(), torch.from_numpy(S.indices.astype(np.int32)).cuda(),
                  torch.from_numpy(S.indptr.astype(np.int64)).cuda(), S.shape[0], S.shape[1])


K3_DESIGNS = SMALL + ["random-128000x40@1e-4", "random-128000x40@2e-4", "random-128000x8@1e-4"]


@gpu
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("ent_rounds", [0, None])
@pytest.mark.parametrize("name", K3_DESIGNS)
def test_k3_at_forced_cuts(name, ent_rounds, dtype, tune):
    """tm_csr_dense_sandwich_ent_* with ONE workgroup over all slabs (ent_rounds = 0: nblk = 1, a wave range of up to
    2000 slabs) and at the default launch, k = 128 and 136, with the column sums, against the oracle's
    csr_dense_sandwich: 1e-10 (float64) / 2e-5 (float32) of max|ref|, as tests/test_k3_ent.py."""
    from oracle import oracle as orc
    from tabmat_amd.ext import sparse as xs
    from tabmat_amd.ext._types import DenseDev

    S, max_pad = es.build_design(name)
    n, m = S.shape
    rng = np.random.default_rng(n + m)
    S = S.astype(dtype)
    tw = SlabEnt.from_csr(_csr_gpu(S, dtype), max_pad=max_pad)
    assert tw is not None
    d = rng.random(n).astype(dtype)
    tol = 1e-10 if dtype == np.float64 else 2e-5
    S64 = S.astype(np.float64).tocsr()
    cref = S64.T @ d.astype(np.float64)
    tune(ent_rounds=ent_rounds)
    for k in (128, 136):
        B = rng.standard_normal((n, k)).astype(dtype)
        out, cs = xs.csr_dense_sandwich_ent(tw, DenseDev(torch.from_numpy(B).cuda(), n, k, 0),
                                            torch.from_numpy(d).cuda(), want_colsum=True)
        ref = orc.csr_dense_sandwich(S64, B.astype(np.float64), d.astype(np.float64), None, None, None)
        err = np.abs(out.cpu().numpy().astype(np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300)
        cerr = np.abs(cs.cpu().numpy() - cref).max() / max(np.abs(cref).max(), 1e-300)
        print(f"k3 {name} rounds={ent_rounds} {np.dtype(dtype).name} k={k}: err {err:.3e} colsum {cerr:.3e}")
        assert err < tol and cerr < tol, (k, err, cerr)


CS_DESIGNS = [nm for nm in SMALL if "44805" in nm or "19201" in nm or "5003" in nm or "130" in nm] + \
    ["random-128000x40@1e-4"]


@gpu
@pytest.mark.parametrize("_catsparse_kernel", ["staged", "gather"], indirect=True)
@pytest.mark.parametrize("dtype", [np.float64, np.float32])
@pytest.mark.parametrize("waves", [4, 16])
@pytest.mark.parametrize("name", CS_DESIGNS)
def test_cat_sparse_at_forced_cuts(name, waves, dtype, _catsparse_kernel, tune):
    """tm_multi_cat_sparse_sandwich_ent{,p}_* with ONE workgroup per pair of groups over all slabs (catsparse_rounds = 0)
    and 4 or 16 waves (2 or 8 wave ranges per group: 350 / 88 slabs each at n = 44 805), packed and unpacked codes,
    drop_first, missing codes, zeros in d, against the oracle's sandwich_cat_sparse: 1e-10 / 3e-5 of max|ref|.  The
    staged kernel walks bstart and never rebuilds a slab: it passes with any placement of the continuity batches, the
    gather kernel only with the right one."""
    from oracle import oracle as orc
    from tabmat_amd.ext import split as xsplit

    S, max_pad = es.build_design(name)
    n, m = S.shape
    rng = np.random.default_rng(n + m + 1)
    S = S.astype(dtype)
    tw = SlabEnt.from_csr(_csr_gpu(S, dtype), max_pad=max_pad)
    assert tw is not None
    d = rng.random(n).astype(dtype)
    d[::7] = 0
    S64 = S.astype(np.float64).tocsr()
    cats, refs = [], []
    for k, lv in enumerate((9, 4, 6)):
        codes = rng.integers(0, lv, n).astype(np.int32)
        if k == 1:
            codes[rng.random(n) < 0.05] = -1
        drop = k == 2
        cats.append((torch.from_numpy(codes).cuda(), lv - int(drop), drop))
        refs.append(orc.sandwich_cat_sparse(codes, lv, d.astype(np.float64), S64, None, None, None)[int(drop):])
    want = np.vstack(refs)
    tol = 1e-10 if dtype == np.float64 else 3e-5
    pk = xsplit.pack_codes(cats)
    assert pk is not None
    tune(catsparse_rounds=0, catsparse_waves=waves)
    for packed in (None, pk):
        got = xsplit.multi_cat_sparse_sandwich_ent(cats, torch.from_numpy(d).cuda(), tw, packed).cpu().numpy()
        assert got.shape == want.shape
        err = np.abs(got - want).max() / max(np.abs(want).max(), 1e-300)
        print(f"catsparse {name} {_catsparse_kernel} waves={waves} {np.dtype(dtype).name} "
              f"packed={packed is not None}: err {err:.3e}")
        assert err < tol, (packed is not None, err)


@gpu
def test_deterministic_self_sandwich_over_one_long_range(tune, monkeypatch):
    """TABMAT_AMD_DETERMINISTIC runs column chunks of a sparse block through K3 on its entry twin: 128 000 x 40 at 1e-4
    (2000 slabs, most blocks empty) with one workgroup over all slabs, against scipy; bit-identical run to run."""
    import tabmat_amd as tm
    import tabmat_amd.categorical_matrix as cmod
    import tabmat_amd.ext.sparse as xs_mod
    from tabmat_amd import _lib

    S, _ = es.build_design("random-128000x40@1e-4")
    n = S.shape[0]
    d = np.random.default_rng(4).random(n)
    sm = tm.SparseMatrix(S.tocsc())
    monkeypatch.setattr(cmod, "DETERMINISTIC", True)
    tune(ent_rounds=0)
    seen = []
    orig = _lib.call

    def spy(name, *a):
        seen.append(name)
        return orig(name, *a)

    monkeypatch.setattr(xs_mod, "call", spy)
    a = sm.sandwich(d)
    b = sm.sandwich(d)
    assert any(s.startswith("tm_csr_dense_sandwich_ent_") for s in seen), seen
    assert sm._ent_det() is not None
    assert np.array_equal(a, b) and np.array_equal(a, a.T)
    want = (S.T.multiply(d)).dot(S).toarray()
    assert np.abs(a - want).max() / np.abs(want).max() < 1e-12


# ---- the public API at the default launch ------------------------------------------------------------------------------
def k3_default_slabs_per_range(n, k_dense, m_sparse):
    """run_csr_dense_ent (csrc/sparse_ent.hip): nblk = NUM_CU / (dense parts of 128 columns x workgroups of 256 sparse
    columns), ranges of ceil(slabs / nblk) slabs."""
    n_slabs = -(-n // 64)
    n_parts = -(-k_dense // 128)
    nz = -(-(-(-m_sparse // 16)) // 16)
    nblk = max(1, min(es.NUM_CU // (n_parts * nz), n_slabs))
    return -(-n_slabs // nblk)


@gpu
def test_sparse_times_dense_2_4M_rows_default_launch():
    """SparseMatrix (2 400 000 x 40, entries only in the LAST slab of each workgroup's range) x DenseMatrix (128 columns,
    C order, float64), no knob touched: `_cross_sandwich` and the SplitMatrix sandwich that holds the two, against
    float64 scipy / numpy -- 1e-10 of max|ref| on the cross block, nat_err < 1e-10 on the whole sandwich (README).
    With a continuity batch at every 32nd slab only, 11 220 of the 11 264 entries were read against wrong rows."""
    import tabmat_amd as tm
    import tabmat_amd.ext.sparse as xs_mod
    from _gpu_util import nat_err
    from tabmat_amd import _lib

    n, m, k = 2_400_000, 40, 128
    span = k3_default_slabs_per_range(n, k, m)
    assert span == 147, "the launch rule changed: this design (and tests/_ent_stream.py) is stale"
    S, _ = es.build_design("last_slab_of_147-2400000x40")
    assert S.shape == (n, m) and S.nnz == 11_264
    rng = np.random.default_rng(7)
    X = rng.standard_normal((n, k))
    d = rng.random(n)
    sm, dm = tm.SparseMatrix(S.tocsc()), tm.DenseMatrix(X)
    seen = []
    orig = _lib.call

    def spy(name, *a):
        seen.append(name)
        return orig(name, *a)

    xs_mod.call = spy
    try:
        out = sm._cross_sandwich(dm, d, None, None, None)
        full = tm.SplitMatrix([dm, sm]).sandwich(d)
    finally:
        xs_mod.call = orig
    assert sum(s.startswith("tm_csr_dense_sandwich_ent_") for s in seen) >= 2, seen
    dX = d[:, None] * X
    ref = S.T @ dX
    err = np.abs(out - ref).max() / np.abs(ref).max()
    print(f"2.4M cross block: err {err:.3e}")
    assert err < 1e-10
    want = np.zeros((k + m, k + m))
    want[:k, :k] = X.T @ dX
    want[k:, :k] = ref
    want[:k, k:] = ref.T
    want[k:, k:] = (S.T.multiply(d)).dot(S).toarray()
    ne = nat_err(full, want)
    print(f"2.4M split sandwich: nat_err {ne:.3e}")
    assert ne < 1e-10
