"""Host model of how the kernels on the entry twin (tabmat_amd/ext/_types.py::SlabEnt) rebuild a slot's slab, the
cuts of a block's slabs into workgroup and wave ranges, and the sparsity designs of tests/test_ent_stream_ranges.py.

The meta word of a slot carries `slab & 63` only.  Both kernels walk a range of slabs [s0, s1) of one 16-column group
in steps of 64 slots (lane <-> slot), aligned to the first batch of the range, and rebuild

    slab     = cur_slab + ((tag - cur_slab) & 63)      all 64 lanes against the same cur_slab
    cur_slab = the slab lane 63 got                    for the NEXT step;  cur_slab = s0 before the first

-- `expand` in csr_dense_ent_kernel (csrc/sparse_ent.hip, "auto expand = [&](unsigned m16)") and `load_rows` in
multi_cat_sparse_ent_kernel (csrc/cat_multi.hip, "auto load_rows = [&](Step &t)": EN_CS_U chained 64-slot sub-steps per call,
which is the same chain).  Lanes past the end of the range: K3 reads whatever follows in the stream (the next group's
batches or the zero slack), the gather kernel reads the range's last slot (`load_stream`: `e1 - 1`)."""
import numpy as np
from scipy import sparse as sps

R, C, U, STEP = 64, 16, 16, 64
NUM_CU = 256


def csr_cpu(S, dtype=np.float64):
    import torch

    from tabmat_amd.ext._types import CsrDev

    S = sps.csr_matrix(S).astype(dtype)
    S.sort_indices()
    return CsrDev(torch.from_numpy(S.data.copy()), torch.from_numpy(S.indices.astype(np.int32)),
                  torch.from_numpy(S.indptr.astype(np.int64)), S.shape[0], S.shape[1])


class Stream:
    """A twin's arrays on the host, plus what the stream says about itself WITHOUT the tags: the slab of every batch
    (from bstart)."""

    def __init__(self, tw):
        self.tw = tw
        self.vals = tw.vals.cpu().numpy()
        self.meta = tw.meta.cpu().numpy().view(np.uint16).astype(np.int64)
        self.tag = self.meta >> 10
        self.bst = tw.bstart.cpu().numpy().view(np.uint32).astype(np.int64)
        self.G, self.S = self.bst.shape[0], self.bst.shape[1] - 1
        self.T = int(self.bst[-1, -1]) * U if self.S else 0
        # true slab of every slot of the stream
        self.true_slab = np.zeros(self.T, dtype=np.int64)
        for g in range(self.G):
            nb = np.diff(self.bst[g])
            lo, hi = int(self.bst[g, 0]) * U, int(self.bst[g, -1]) * U
            self.true_slab[lo:hi] = np.repeat(np.repeat(np.arange(self.S), nb), U)
        self.real = self.vals[:self.T] != 0

    def batch_slabs(self, g):
        return np.repeat(np.arange(self.S), np.diff(self.bst[g]))

    def to_coo(self):
        """The matrix the stream holds, decoded with the TRUE slabs (kernel column order undone)."""
        q = np.nonzero(self.real)[0]
        grp = np.searchsorted(self.bst[:, 0] * U, q, side="right") - 1
        # (groups without a batch share their start with the next one: the LAST group that starts at or before q)
        row = self.true_slab[q] * R + ((self.meta[q] >> 4) & 63)
        kcol = grp * C + (self.meta[q] & 15)
        inv = self.tw.inv.cpu().numpy()
        col_of = np.full(self.tw.mk, -1, dtype=np.int64)
        col_of[inv] = np.arange(self.tw.m)
        assert (col_of[kcol] >= 0).all()
        return sps.coo_matrix((self.vals[q], (row, col_of[kcol])), shape=(self.tw.n, self.tw.m)).tocsr()


def decode_range(st, group, s0, s1, tail="stream"):
    """Slabs the kernels rebuild for the slots of batches [bstart[group, s0], bstart[group, s1]), as an array over
    those slots.  tail: what lanes past the end of the range read -- "stream" (K3: what follows) or "last" (gather
    kernel: the range's last slot)."""
    e0, e1 = int(st.bst[group, s0]) * U, int(st.bst[group, s1]) * U
    out = np.empty(e1 - e0, dtype=np.int64)
    tag = st.tag
    cur = int(s0)
    for e in range(e0, e1, STEP):
        if e + STEP <= e1 or tail == "stream":
            t = tag[e:e + STEP]                       # (the slack covers a read past the last group's end)
        else:
            t = tag[np.minimum(np.arange(e, e + STEP), e1 - 1)]
        slab = cur + ((t - cur) & 63)
        k = min(STEP, e1 - e)
        out[e - e0:e - e0 + k] = slab[:k]
        cur = int(slab[STEP - 1])
    return out


def wrong_real_slots(st, group, s0, s1, tail):
    """Real (value != 0) slots of the range whose rebuilt slab -- and with it the row -- is not the true one."""
    e0, e1 = int(st.bst[group, s0]) * U, int(st.bst[group, s1]) * U
    if e1 == e0:
        return 0
    got = decode_range(st, group, s0, s1, tail)
    return int(((got != st.true_slab[e0:e1]) & st.real[e0:e1]).sum())


def block_ranges(n_slabs, nblk):
    """The launchers' cut of the slabs into workgroup ranges (csrc/sparse_ent.hip run_csr_dense_ent, csrc/cat_multi.hip
    run_multi_cat_sparse_ent: nblk = min(nblk, slabs); spb = ceil(slabs / nblk); ranges of spb slabs)."""
    if n_slabs == 0:
        return []
    nblk = max(1, min(nblk, n_slabs))
    spb = -(-n_slabs // nblk)
    return [(s, min(s + spb, n_slabs)) for s in range(0, n_slabs, spb)]


def wave_ranges(s0, s1, nwh):
    """The gather kernel's cut of a workgroup's range among the nwh waves of a group (`spw`, csrc/cat_multi.hip
    multi_cat_sparse_ent_kernel)."""
    spw = -(-(s1 - s0) // nwh)
    out = []
    for wi in range(nwh):
        sa = min(s0 + wi * spw, s1)
        sb = min(sa + spw, s1)
        if sb > sa:
            out.append((sa, sb))
    return out


NBLKS = (1, 2, 3, 5, 9, 16, 64, 256)
WAVE_SPLITS = (2, 8)


def all_cuts(n_slabs):
    """{label: [(s0, s1, tail)]}: K3's ranges for every nblk, and the gather kernel's wave ranges inside them."""
    cuts = {}
    for nblk in NBLKS:
        br = block_ranges(n_slabs, nblk)
        cuts[f"nblk={nblk}"] = [(a, b, "stream") for a, b in br]
        for nwh in WAVE_SPLITS:
            cuts[f"nblk={nblk}/waves={nwh}"] = [(a, b, "last") for s0, s1 in br for a, b in wave_ranges(s0, s1, nwh)]
    return cuts


# ---- designs -------------------------------------------------------------------------------------------------------
def _finish(S):
    S = sps.csr_matrix(S)
    S.sum_duplicates()
    S.eliminate_zeros()
    S.sort_indices()
    return S


def entries_in_slabs(n, m, slabs, per_slab, rng):
    """per_slab entries (distinct rows where the slab has that many, columns spread over all of them) in each of the
    given slabs."""
    rows, cols = [], []
    for k, s in enumerate(sorted(set(int(s) for s in slabs))):
        lo, hi = s * R, min(s * R + R, n)
        j = np.arange(per_slab)
        rows.append(lo + (j * 13 + k) % (hi - lo))
        cols.append((j * 7 + k) % m)
    rows, cols = np.concatenate(rows), np.concatenate(cols)
    vals = rng.standard_normal(rows.shape[0])
    vals[vals == 0] = 1.0
    S = sps.coo_matrix((vals, (rows, cols)), shape=(n, m)).tocsr()
    S.sum_duplicates()
    S.data[S.data == 0] = 1.0
    return _finish(S)


def design(kind, n, m, rng, arg=None):
    n_slabs = (n + R - 1) // R
    if kind == "far_apart_slabs":
        from test_k3_ent import _structured

        return _finish(_structured("far_apart_slabs", n, m, rng))
    if kind == "last_slab_of_range":              # arg = slabs per range
        last = [min(s + arg, n_slabs) - 1 for s in range(0, n_slabs, arg)]
        return entries_in_slabs(n, m, last, 44, rng)
    if kind == "first_slab_of_range":
        return entries_in_slabs(n, m, range(0, n_slabs, arg), 44, rng)
    if kind == "every_k_slabs":                   # ONE entry every arg slabs (one column: the other groups stay empty)
        sl = np.arange(arg - 1, n_slabs, arg)
        rows = np.minimum(sl * R + (sl * 5) % R, n - 1)
        return _finish(sps.coo_matrix((1.0 + np.arange(len(sl)), (rows, np.full(len(sl), m // 3))), shape=(n, m)))
    if kind == "empty_group":                     # two full columns: with three groups, the third holds no entry at all
        S = sps.lil_matrix((n, m))
        S[:, 5] = rng.standard_normal((n, 1)) + 3.0
        S[:, m // 2] = rng.standard_normal((n, 1)) - 3.0
        return _finish(S)
    if kind == "random":                          # arg = density
        S = sps.random(n, m, density=arg, format="csr", random_state=rng, dtype=np.float64)
        S.data = S.data + 0.5
        if n:                                     # the last row holds an entry: the ragged tail is not empty
            S = S.tolil()
            S[n - 1, m - 1] = 2.5
        return _finish(S)
    raise ValueError(kind)


# (id, kind, n, m, arg, max_pad)
SMALL_DESIGNS = [
    ("far_apart-5003x100", "far_apart_slabs", 5003, 100, None, 1e9),
    ("far_apart-2560x512", "far_apart_slabs", 64 * 40, 512, None, 1e9),
    ("far_apart-130x17", "far_apart_slabs", 130, 17, None, 1e9),
    ("far_apart-44805x48", "far_apart_slabs", 64 * 700 + 5, 48, None, 1e9),
    ("last_slab_of_78-44805x48", "last_slab_of_range", 64 * 700 + 5, 48, 78, 1e9),
    ("last_slab_of_147-44805x40", "last_slab_of_range", 64 * 700 + 5, 40, 147, 8.0),
    ("first_slab_of_78-44805x48", "first_slab_of_range", 64 * 700 + 5, 48, 78, 1e9),
    ("first_slab_of_147-44805x40", "first_slab_of_range", 64 * 700 + 5, 40, 147, 8.0),
    ("every_63-44805x48", "every_k_slabs", 64 * 700 + 5, 48, 63, None),
    ("every_64-44805x48", "every_k_slabs", 64 * 700 + 5, 48, 64, None),
    ("every_65-44805x48", "every_k_slabs", 64 * 700 + 5, 48, 65, None),
    ("every_127-44805x48", "every_k_slabs", 64 * 700 + 5, 48, 127, None),
    ("every_129-44805x48", "every_k_slabs", 64 * 700 + 5, 48, 129, None),
    ("empty_group-19201x40", "empty_group", 64 * 300 + 1, 40, None, 8.0),
    ("no_empty_block-5003x40", "random", 5003, 40, 0.3, 8.0),
    ("n=1", "random", 1, 20, 0.0, None),
    ("n=63", "random", 63, 20, 0.01, None),
    ("n=65", "random", 65, 20, 0.01, None),
    ("n=64*130-1", "random", 64 * 130 - 1, 20, 0.0005, None),
    ("n=64*130+1", "random", 64 * 130 + 1, 20, 0.0005, None),
]
LARGE_DESIGNS = [
    ("random-128000x8@1e-4", "random", 128_000, 8, 1e-4, None),
    ("random-128000x8@2e-4", "random", 128_000, 8, 2e-4, None),
    ("random-128000x40@1e-4", "random", 128_000, 40, 1e-4, None),
    ("random-128000x40@2e-4", "random", 128_000, 40, 2e-4, None),
    ("last_slab_of_147-2400000x40", "last_slab_of_range", 2_400_000, 40, 147, 8.0),
]
DESIGNS = {d[0]: d for d in SMALL_DESIGNS + LARGE_DESIGNS}


def build_design(name, seed=0):
    _, kind, n, m, arg, max_pad = DESIGNS[name]
    rng = np.random.default_rng(seed + n + m)
    return design(kind, n, m, rng, arg), max_pad
