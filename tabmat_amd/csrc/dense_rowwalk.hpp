// The dense row walk K8, K8d (sandwich_matvec.hip) and K9 (glm.hip) share: everything around their loop bodies.
//
// A workgroup of 4 waves owns a contiguous run of rows of a row-major block.  A wave step loads R rows per lane
// segment into registers (LPR lanes per row, NL loads of VEC elements per lane and row), the kernel's own loop
// body does its per-row math and adds into per-lane column sums acc[NL][VEC].  Here: the constants, the per-lane
// column setup, the fixed-order fold of those sums (row segments of a wave, waves of a workgroup, workgroups in
// a second launch -- no floating-point atomics, bitwise reproducible), and the host side: launch geometry,
// launcher, the (VEC, LPR, NL) ladder and the width limits.  The loop bodies stay in the kernels: the row
// registers x[R][NL] do not cross a function boundary (the compiler splits the array differently when they do,
// and the 128-column float64 layout of K8 sits exactly on the 80-VGPR occupancy step).
#pragma once

#include <algorithm>

#include "common.hpp"

namespace tmh {
namespace rowwalk {

constexpr int THREADS = 256;
constexpr int WAVES = THREADS / WAVE;
constexpr int MAX_NL = 8;              // loads per lane and row: m <= 64 * VEC * 8
constexpr int MAX_WG = 1024;

// R, the rows per lane segment and wave step: 8 loads in flight per lane
constexpr int rows_per_segment(int nl) { return nl >= 8 ? 1 : 8 / nl; }

// ---------------------------------------------------------------------------------
// device
// ---------------------------------------------------------------------------------
// sum over the LPR lanes of each row segment; every lane of the segment gets the sum (DPP for the strides below
// 16, ds_bpermute above)
template <int LPR>
__device__ __forceinline__ double segment_allreduce(double v) {
    v += dpp_xor<1>(v);
    v += dpp_xor<2>(v);
    v += dpp_xor<4>(v);
    if constexpr (LPR >= 16) v += dpp_xor<8>(v);
    if constexpr (LPR >= 32) v += __shfl_xor(v, 16, 64);
    if constexpr (LPR >= 64) v += __shfl_xor(v, 32, 64);
    return v;
}

// this lane's columns (q * LPR + sl) * VEC + e: which loads are inside the block, their centres (0 without), and
// zeroed sums.  m % VEC == 0, so a vector is all in or all out.
template <int LPR, typename F, int NL, int VEC>
__device__ __forceinline__ void lane_columns(int m, int sl, const F *__restrict__ center, bool (&live)[NL],
                                             F (&cc)[NL][VEC], double (&acc)[NL][VEC]) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int j0 = (q * LPR + sl) * VEC;
        live[q] = j0 < m;
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            cc[q][e] = (live[q] && center) ? center[j0 + e] : F(0);
            acc[q][e] = 0.0;
        }
    }
}

// ... and the entries of u that go with them (0 outside the block)
template <int LPR, typename F, int NL, int VEC>
__device__ __forceinline__ void lane_u(int m, int sl, const F *__restrict__ u, F (&uu)[NL][VEC]) {
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int j0 = (q * LPR + sl) * VEC;
#pragma unroll
        for (int e = 0; e < VEC; ++e) uu[q][e] = j0 < m ? u[j0 + e] : F(0);
    }
}

// the workgroup's column sums in red[0 .. m): the row segments of a wave hold the same columns and are folded
// with a fixed xor tree, then the waves add one after the other.  Ends behind a barrier.
template <int LPR, int NL, int VEC>
__device__ __forceinline__ void fold_columns(double (&acc)[NL][VEC], const bool (&live)[NL], double *red) {
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int seg = lane / LPR;
    const int sl = lane % LPR;
#pragma unroll
    for (int s = LPR; s < WAVE; s <<= 1)
#pragma unroll
        for (int q = 0; q < NL; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] += __shfl_xor(acc[q][e], s, 64);
    for (int wv = 0; wv < WAVES; ++wv) {
        if (wave == wv && seg == 0) {
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int j = (q * LPR + sl) * VEC + e;
                        red[j] = wv == 0 ? acc[q][e] : red[j] + acc[q][e];
                    }
                }
        }
        __syncthreads();
    }
}

// red[0 .. width) -> the workgroup's row of the partial sums
__device__ __forceinline__ void store_partial(const double *red, double *__restrict__ part, int width) {
    double *dst = part + (int64_t)blockIdx.x * width;
    for (int j = threadIdx.x; j < width; j += THREADS) dst[j] = red[j];
}

// g[j] = sum over the nb partials (rows of m + extra doubles, extra 0 or 1) in a fixed order: 16 waves per 64
// columns striding the partials, a fixed tree at the end.  Column m, when there is one, goes to loss[0].
template <typename F>
__global__ __launch_bounds__(1024) void reduce_kernel(const double *__restrict__ part, int nb, int m, int extra,
                                                      F *__restrict__ g, double *__restrict__ loss) {
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    const int width = m + extra;
    double s = 0.0;
    if (j < width)
        for (int b = wave; b < nb; b += 16) s += part[(int64_t)b * width + j];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && j < width) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k += 4) t += (red[k][lane] + red[k + 1][lane]) + (red[k + 2][lane] + red[k + 3][lane]);
        if (j < m) g[j] = (F)t;
        else loss[0] = t;
    }
}

// ---------------------------------------------------------------------------------
// host
// ---------------------------------------------------------------------------------
// elements of a 16-byte load, and the widest block 64 lanes x MAX_NL loads of `vec` elements serve
template <typename F>
constexpr int FULL_VEC = 16 / (int)sizeof(F);
constexpr int64_t max_columns(int vec) { return (int64_t)WAVE * MAX_NL * vec; }

// VEC of a block: FULL_VEC on 16-byte aligned rows, 1 (one element per load) otherwise; 0 when the block is wider
// than that form serves
template <typename F>
inline int load_form(const F *X, int64_t m) {
    const int vec = (m % FULL_VEC<F> == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0) ? FULL_VEC<F> : 1;
    return m <= max_columns(vec) ? vec : 0;
}

// contiguous runs of whole wave steps (`rows_per_step` rows each), at most MAX_WG of them
struct Geometry {
    int64_t rows_per_wg;
    int nwg;
};
inline Geometry geometry(int64_t n, int rows_per_step) {
    const int64_t steps = ceil_div(n, rows_per_step);
    const int64_t steps_per_wg = std::max<int64_t>(WAVES, ceil_div(steps, MAX_WG));
    const int64_t rows_per_wg = steps_per_wg * rows_per_step;
    return {rows_per_wg, (int)ceil_div(n, rows_per_wg)};
}

// f(VEC, LPR, NL) as integral_constants for a block of m columns read `vec` elements per load: LPR lanes per
// row (8 .. 64), NL loads per lane and row (> 1 only with LPR = 64)
template <typename F, typename Fn>
int dispatch(int vec, int m, Fn &&f) {
    auto ladder = [&](auto v) {
        constexpr int VEC = decltype(v)::value;
        auto go = [&](auto lpr, auto nl) { return f(v, lpr, nl); };
        using std::integral_constant;
        const int nvec = (m + VEC - 1) / VEC;          // vectors per row
        if (nvec <= 8) return go(integral_constant<int, 8>{}, integral_constant<int, 1>{});
        if (nvec <= 16) return go(integral_constant<int, 16>{}, integral_constant<int, 1>{});
        if (nvec <= 32) return go(integral_constant<int, 32>{}, integral_constant<int, 1>{});
        if (nvec <= 64) return go(integral_constant<int, 64>{}, integral_constant<int, 1>{});
        if (nvec <= 128) return go(integral_constant<int, 64>{}, integral_constant<int, 2>{});
        if (nvec <= 256) return go(integral_constant<int, 64>{}, integral_constant<int, 4>{});
        return go(integral_constant<int, 64>{}, integral_constant<int, 8>{});
    };
    if (vec == 1) return ladder(std::integral_constant<int, 1>{});
    return ladder(std::integral_constant<int, FULL_VEC<F>>{});
}

// One walk: main_kernel(geometry, LDS bytes, partials) launches the kernel (THREADS threads, geometry.nwg
// workgroups) that leaves one row of m + extra doubles per workgroup; the reduce kernel finishes g (and loss).
template <typename F, typename Main>
int launch(int64_t n, int m, int extra, int rows_per_step, F *g, double *loss, hipStream_t st, Main &&main_kernel) {
    const Geometry ge = geometry(n, rows_per_step);
    const int width = m + extra;
    void *ws = nullptr;
    int rc = get_workspace((size_t)ge.nwg * width * sizeof(double), &ws, st);
    if (rc) return rc;
    double *part = static_cast<double *>(ws);
    prof_begin(st);
    main_kernel(ge, (size_t)width * sizeof(double), part);
    prof_end(st);
    TM_LAUNCH_CHECK();
    hipLaunchKernelGGL((reduce_kernel<F>), dim3((unsigned)ceil_div(width, 64)), dim3(1024), 0, st, part, ge.nwg, m,
                       extra, g, loss);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

}  // namespace rowwalk
}  // namespace tmh
