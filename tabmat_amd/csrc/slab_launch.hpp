// Host skeleton of the slab-family sparse x dense launchers (K3: sparse_slab.hip, sparse_lg.hip, sparse_ent.hip).
// All five kernels cut the rows into slabs, the sparse columns into per-wave groups and the dense operand into
// column parts; a workgroup (blockIdx.x = slab range, .y = dense part, .z = layer of `waves` groups) writes one
// partial tile, and the tiles are reduced over the slab ranges, untiled into out and -- lg and ent -- joined by the
// column sums A' d.  A launcher checks its arguments, makes a plan, carves the workspace and hands its kernel launch
// to slab_launch_and_finish as a callable; what differs between the kernels (lg's lockstep counters and kernel
// ladder, ent's kernel pick) stays in their launchers.
#pragma once
#include <string.h>

#include <algorithm>

#include "common.hpp"
#include "reduce.hpp"

namespace tmh {

struct SlabGeom {
    int rows;       // rows per slab
    int cpw;        // sparse columns per wave (a group)
    int waves;      // waves per workgroup
    int width;      // dense columns per part: 64 or 128
    bool pad_m;     // tiles hold whole groups (m rounded up); else m is a multiple of cpw
};

struct SlabPlan {
    int64_t n_slabs, mpad, nblk, spb, stride;   // nblk workgroups of spb slabs; stride: elements per (part, workgroup)
    int n_groups, n_parts, nz, threads, width;
    dim3 grid() const { return dim3((unsigned)nblk, (unsigned)n_parts, (unsigned)nz); }
};

// rounds: workgroups per CU the slabs are cut for (the *_rounds tune knobs; 1 where a kernel has none)
inline SlabPlan slab_plan(int64_t n, int64_t m, int64_t nB, const SlabGeom &g, int64_t rounds = 1) {
    SlabPlan p{};
    p.n_slabs = ceil_div(n, g.rows);
    p.n_groups = (int)(g.pad_m ? ceil_div(m, g.cpw) : m / g.cpw);
    p.mpad = (int64_t)p.n_groups * g.cpw;
    p.n_parts = (int)ceil_div(nB, g.width);
    p.nz = (int)ceil_div(p.n_groups, g.waves);
    p.threads = g.waves * 64;
    p.width = g.width;
    p.stride = p.mpad * g.width;
    if (p.n_slabs == 0) return p;
    p.nblk = std::max<int64_t>(1, rounds * NUM_CU / ((int64_t)p.n_parts * p.nz));
    p.nblk = std::min<int64_t>(p.nblk, p.n_slabs);
    p.spb = ceil_div(p.n_slabs, p.nblk);
    p.nblk = ceil_div(p.n_slabs, p.spb);
    return p;
}

// the asynchronous slab copy moves 16-byte vectors of whole rows (`entry`: the entry point's name without suffix)
template <typename F>
inline int slab_check_b(const char *entry, const F *B, int64_t r) {
    constexpr int VEC = 16 / (int)sizeof(F);
    if ((reinterpret_cast<uintptr_t>(B) & 15) != 0 || r % VEC != 0 || r < VEC) {
        set_error("%s: B must be C-ordered with 16-byte aligned rows", entry);
        return TM_EUNSUPPORTED;
    }
    return TM_OK;
}
// (the twin's name is the last word of the entry point's: tm_csr_dense_sandwich_lg -> tm_lg_group_cols)
inline int slab_check_m(const char *entry, int64_t m, int cpw) {
    if (m % cpw != 0) {
        set_error("%s: m must be a multiple of tm_%s_group_cols()", entry, strrchr(entry, '_') + 1);
        return TM_EINVAL;
    }
    return TM_OK;
}

// no rows: the product is zero (colsum may be NULL)
template <typename F>
inline int slab_zero_fill(F *out, int64_t m, int64_t nB, F *colsum, hipStream_t st) {
    TM_HIP(hipMemsetAsync(out, 0, sizeof(F) * (size_t)(m * nB), st));
    if (colsum) TM_HIP(hipMemsetAsync(colsum, 0, sizeof(F) * (size_t)m, st));
    return TM_OK;
}

template <typename F>
struct SlabWs {
    F *tmp;        // [part][mpad][width]: the reduced tiles
    F *part;       // [part][workgroup][mpad][width]: the kernels' partial tiles
    F *csum;       // [workgroup][m] partial column sums (csum_m > 0)
    void *extra;   // extra_bytes of the caller's
};
// every piece starts on a 256-byte boundary
template <typename F>
inline int slab_workspace(const SlabPlan &p, int64_t csum_m, size_t extra_bytes, hipStream_t st, SlabWs<F> *w) {
    const size_t tmp_bytes = align256(sizeof(F) * (size_t)(p.n_parts * p.stride));
    const size_t part_bytes = align256(sizeof(F) * (size_t)((int64_t)p.n_parts * p.nblk * p.stride));
    const size_t csum_bytes = align256(sizeof(F) * (size_t)(p.nblk * csum_m)) + 256;
    void *wsv = nullptr;
    int rc = get_workspace(tmp_bytes + part_bytes + csum_bytes + extra_bytes + 256, &wsv, st);
    if (rc) return rc;
    char *base = reinterpret_cast<char *>(wsv);
    w->tmp = reinterpret_cast<F *>(base);
    w->part = reinterpret_cast<F *>(base + tmp_bytes);
    w->csum = reinterpret_cast<F *>(base + tmp_bytes + part_bytes);
    w->extra = base + tmp_bytes + part_bytes + csum_bytes;
    return TM_OK;
}

// tmp [part][mpad][W] -> out[m][nB]
template <typename F, int W>
__global__ void slab_untile_kernel(const F *__restrict__ tmp, int64_t m, int64_t nB, int64_t mpad,
                                   F *__restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= m * nB) return;
    const int64_t i = e / nB, j = e % nB;
    out[e] = tmp[((j / W) * mpad + i) * W + (j % W)];
}

// column sums: csum[c] = sum over the workgroups (fixed order) of their partial sums
template <typename F>
__global__ void slab_csum_kernel(const F *__restrict__ part, int nblk, int64_t m, F *__restrict__ csum) {
    const int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= m) return;
    double a = 0.0;
    for (int b = 0; b < nblk; ++b) a += (double)part[(int64_t)b * m + c];
    csum[c] = (F)a;
}

// launch(grid, block): the main kernel on st, timed by the profile events; then reduce, untile, column sums
template <typename F, typename Kern, typename Launch>
static int slab_launch_and_finish(Kern kern, const SlabPlan &p, size_t lds, const SlabWs<F> &w, int64_t m, int64_t nB,
                                  F *out, F *colsum, hipStream_t st, Launch &&launch) {
    TM_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)lds));
    prof_begin(st);
    launch(p.grid(), dim3((unsigned)p.threads));
    prof_end(st);
    TM_LAUNCH_CHECK();
    int rc = launch_reduce_partials<F>(w.part, p.stride, (int)p.nblk, p.n_parts, w.tmp, p.n_parts * p.stride, false, st);
    if (rc) return rc;
    auto untile = p.width == 64 ? &slab_untile_kernel<F, 64> : &slab_untile_kernel<F, 128>;
    hipLaunchKernelGGL(untile, dim3((unsigned)ceil_div(m * nB, 256)), dim3(256), 0, st, w.tmp, m, nB, p.mpad, out);
    TM_LAUNCH_CHECK();
    if (colsum) {
        hipLaunchKernelGGL((slab_csum_kernel<F>), dim3((unsigned)ceil_div(m, 256)), dim3(256), 0, st, w.csum,
                           (int)p.nblk, m, colsum);
        TM_LAUNCH_CHECK();
    }
    return TM_OK;
}

}  // namespace tmh
