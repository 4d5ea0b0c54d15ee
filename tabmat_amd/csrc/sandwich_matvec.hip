// K8  dense Hessian-vector product in one pass over a row-major block (gfx950).
//
//   t_r = (x_r - c) . u + shift + t_add[r]        (c, shift, t_add optional)
//   w_r = dm[r] * t_r                             (written when w != NULL)
//   g   = sum_r (x_r - c) w_r                     (written, never accumulated)
//
// i.e. g = X' diag(dm) X u without forming X' diag(dm) X.  A wave loads R rows (R * NL 16-byte loads
// per lane) into registers, reduces the R dot products across the lanes of each row (DPP for the
// strides below 16, ds_bpermute above), forms w_r and adds x_r w_r into per-lane column accumulators --
// the row is still in the registers, so HBM delivers X exactly once and no LDS tile is needed.  Every
// workgroup owns a contiguous run of rows; at its end the 4 waves (and the row segments of a wave when
// a row is narrower than 64 lanes) are summed in a fixed order and written as the workgroup's partial
// g, which a second launch sums in a fixed order: no floating-point atomics, bitwise reproducible.
// The products are formed in float64 for both data types (float32 data is widened on load).
#include <algorithm>

#include "common.hpp"

namespace tmh {

namespace {

constexpr int SMV_THREADS = 256;
constexpr int SMV_WAVES = SMV_THREADS / WAVE;
constexpr int SMV_MAX_NL = 8;          // 16-byte loads per lane and row: m <= 64 * VEC * 8
constexpr int SMV_MAX_WG = 1024;

// sum over the LPR lanes of each row segment; every lane of the segment gets the sum
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

// VEC: elements per load (16 / sizeof(F) on 16-byte aligned rows, 1 else); LPR: lanes per row (8 .. 64,
// a power of two); NL: loads per lane and row (> 1 only with LPR = 64); R: rows per lane segment and step.
template <typename F, int VEC, int LPR, int NL, int R>
__global__ __launch_bounds__(SMV_THREADS) void dense_sandwich_matvec_kernel(
    const F *__restrict__ X, int64_t n, int m, const F *__restrict__ u, const F *__restrict__ dm,
    const F *__restrict__ t_add, const F *__restrict__ center, const F *__restrict__ shift,
    int64_t rows_per_wg, double *__restrict__ part, F *__restrict__ w) {
    typedef F vec_t __attribute__((ext_vector_type(VEC)));
    constexpr int RPL = WAVE / LPR;                    // row segments of a wave
    constexpr int ROWS = R * RPL;                      // rows of one wave step
    extern __shared__ double smv_red[];                // m doubles
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int seg = lane / LPR;
    const int sl = lane % LPR;

    // this lane's columns: (q * LPR + sl) * VEC + e
    F uu[NL][VEC], cc[NL][VEC];
    double acc[NL][VEC];
    bool live[NL];
#pragma unroll
    for (int q = 0; q < NL; ++q) {
        const int j0 = (q * LPR + sl) * VEC;
        live[q] = j0 < m;                              // m % VEC == 0: a vector is all in or all out
#pragma unroll
        for (int e = 0; e < VEC; ++e) {
            uu[q][e] = live[q] ? u[j0 + e] : F(0);
            cc[q][e] = (live[q] && center) ? center[j0 + e] : F(0);
            acc[q][e] = 0.0;
        }
    }
    const double s0 = shift ? (double)shift[0] : 0.0;

    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r_end = min(r_begin + rows_per_wg, n);
    for (int64_t r0 = r_begin + (int64_t)wave * ROWS; r0 < r_end; r0 += (int64_t)SMV_WAVES * ROWS) {
        vec_t x[R][NL];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = min(r0 + r * RPL + seg, r_end - 1);
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                if (live[q]) {
                    x[r][q] = __builtin_nontemporal_load(
                        reinterpret_cast<const vec_t *>(X + row * (int64_t)m + (q * LPR + sl) * VEC));
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) x[r][q][e] = F(0);
                }
            }
        }
        double wr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = r0 + r * RPL + seg;
            double dmr = 0.0, ta = 0.0;
            if (row < r_end) {
                dmr = (double)dm[row];
                if (t_add) ta = (double)t_add[row];
            }
            double p = 0.0;
#pragma unroll
            for (int q = 0; q < NL; ++q)
#pragma unroll
                for (int e = 0; e < VEC; ++e) p = fma((double)x[r][q][e] - (double)cc[q][e], (double)uu[q][e], p);
            const double t = segment_allreduce<LPR>(p) + s0 + ta;
            // rows past the end (clamped loads) get w = 0 and are not written
            wr[r] = row < r_end ? dmr * t : 0.0;
            if (w && sl == 0 && row < r_end) w[row] = (F)wr[r];
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[q][e] = fma((double)x[r][q][e] - (double)cc[q][e], wr[r], acc[q][e]);
                }
    }

    // the row segments of a wave hold the same columns: fold them (fixed xor tree)
#pragma unroll
    for (int s = LPR; s < WAVE; s <<= 1)
#pragma unroll
        for (int q = 0; q < NL; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] += __shfl_xor(acc[q][e], s, 64);
    // then the waves, one after the other
    for (int wv = 0; wv < SMV_WAVES; ++wv) {
        if (wave == wv && seg == 0) {
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int j = (q * LPR + sl) * VEC + e;
                        smv_red[j] = wv == 0 ? acc[q][e] : smv_red[j] + acc[q][e];
                    }
                }
        }
        __syncthreads();
    }
    double *dst = part + (int64_t)blockIdx.x * m;
    for (int j = threadIdx.x; j < m; j += SMV_THREADS) dst[j] = smv_red[j];
}

// K8d  the diagonal of the same product: acc_j += dm[r] (x_rj - c_j)^2.  K8's row walk, registers and fold without
// the dot product (nothing crosses lanes inside the loop); the partials go through smv_reduce_kernel.
template <typename F, int VEC, int LPR, int NL, int R>
__global__ __launch_bounds__(SMV_THREADS) void dense_sandwich_diag_kernel(
    const F *__restrict__ X, int64_t n, int m, const F *__restrict__ dm, const F *__restrict__ center,
    int64_t rows_per_wg, double *__restrict__ part) {
    typedef F vec_t __attribute__((ext_vector_type(VEC)));
    constexpr int RPL = WAVE / LPR;
    constexpr int ROWS = R * RPL;
    extern __shared__ double smv_red[];                // m doubles
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    const int seg = lane / LPR;
    const int sl = lane % LPR;

    F cc[NL][VEC];
    double acc[NL][VEC];
    bool live[NL];
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

    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r_end = min(r_begin + rows_per_wg, n);
    for (int64_t r0 = r_begin + (int64_t)wave * ROWS; r0 < r_end; r0 += (int64_t)SMV_WAVES * ROWS) {
        vec_t x[R][NL];
        double dr[R];
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const int64_t row = r0 + r * RPL + seg;
            const int64_t rowc = min(row, r_end - 1);
#pragma unroll
            for (int q = 0; q < NL; ++q) {
                if (live[q]) {
                    x[r][q] = __builtin_nontemporal_load(
                        reinterpret_cast<const vec_t *>(X + rowc * (int64_t)m + (q * LPR + sl) * VEC));
                } else {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) x[r][q][e] = F(0);
                }
            }
            // rows past the end (clamped loads) get weight 0
            dr[r] = row < r_end ? (double)dm[row] : 0.0;
        }
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const double xc = (double)x[r][q][e] - (double)cc[q][e];
                        acc[q][e] = fma(xc * xc, dr[r], acc[q][e]);
                    }
                }
    }

#pragma unroll
    for (int s = LPR; s < WAVE; s <<= 1)
#pragma unroll
        for (int q = 0; q < NL; ++q)
#pragma unroll
            for (int e = 0; e < VEC; ++e) acc[q][e] += __shfl_xor(acc[q][e], s, 64);
    for (int wv = 0; wv < SMV_WAVES; ++wv) {
        if (wave == wv && seg == 0) {
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) {
                        const int j = (q * LPR + sl) * VEC + e;
                        smv_red[j] = wv == 0 ? acc[q][e] : smv_red[j] + acc[q][e];
                    }
                }
        }
        __syncthreads();
    }
    double *dst = part + (int64_t)blockIdx.x * m;
    for (int j = threadIdx.x; j < m; j += SMV_THREADS) dst[j] = smv_red[j];
}

// g[j] = sum over the nb partials in a fixed order (16 waves per 64 columns, fixed tree at the end)
template <typename F>
__global__ __launch_bounds__(1024) void smv_reduce_kernel(const double *__restrict__ part, int nb, int m,
                                                          F *__restrict__ g) {
    __shared__ double red[16][64];
    const int lane = threadIdx.x & 63;
    const int wave = threadIdx.x >> 6;
    const int j = blockIdx.x * 64 + lane;
    double s = 0.0;
    if (j < m)
        for (int b = wave; b < nb; b += 16) s += part[(int64_t)b * m + j];
    red[wave][lane] = s;
    __syncthreads();
    if (wave == 0 && j < m) {
        double t = 0.0;
#pragma unroll
        for (int k = 0; k < 16; k += 4) t += (red[k][lane] + red[k + 1][lane]) + (red[k + 2][lane] + red[k + 3][lane]);
        g[j] = (F)t;
    }
}

template <typename F, int VEC, int LPR, int NL>
int launch_smv(const F *X, int64_t n, int m, const F *u, const F *dm, const F *t_add, const F *center,
               const F *shift, F *g, F *w, hipStream_t st) {
    constexpr int R = NL >= 8 ? 1 : 8 / NL;
    constexpr int ROWS = R * (WAVE / LPR);
    // contiguous runs of whole wave steps, at most SMV_MAX_WG of them
    const int64_t steps = ceil_div(n, ROWS);
    const int64_t steps_per_wg = std::max<int64_t>(SMV_WAVES, ceil_div(steps, SMV_MAX_WG));
    const int64_t rows_per_wg = steps_per_wg * ROWS;
    const int nwg = (int)ceil_div(n, rows_per_wg);
    void *ws = nullptr;
    int rc = get_workspace((size_t)nwg * m * sizeof(double), &ws, st);
    if (rc) return rc;
    double *part = static_cast<double *>(ws);
    prof_begin(st);
    hipLaunchKernelGGL((dense_sandwich_matvec_kernel<F, VEC, LPR, NL, R>), dim3(nwg), dim3(SMV_THREADS),
                       (size_t)m * sizeof(double), st, X, n, m, u, dm, t_add, center, shift, rows_per_wg, part, w);
    prof_end(st);
    TM_LAUNCH_CHECK();
    hipLaunchKernelGGL((smv_reduce_kernel<F>), dim3((unsigned)ceil_div(m, 64)), dim3(1024), 0, st, part, nwg, m, g);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

template <typename F, int VEC>
int dispatch_smv(const F *X, int64_t n, int m, const F *u, const F *dm, const F *t_add, const F *center,
                 const F *shift, F *g, F *w, hipStream_t st) {
    const int nvec = (m + VEC - 1) / VEC;              // vectors per row
    if (nvec <= 8) return launch_smv<F, VEC, 8, 1>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    if (nvec <= 16) return launch_smv<F, VEC, 16, 1>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    if (nvec <= 32) return launch_smv<F, VEC, 32, 1>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    if (nvec <= 64) return launch_smv<F, VEC, 64, 1>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    if (nvec <= 128) return launch_smv<F, VEC, 64, 2>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    if (nvec <= 256) return launch_smv<F, VEC, 64, 4>(X, n, m, u, dm, t_add, center, shift, g, w, st);
    return launch_smv<F, VEC, 64, 8>(X, n, m, u, dm, t_add, center, shift, g, w, st);
}

template <typename F, int VEC, int LPR, int NL>
int launch_sdiag(const F *X, int64_t n, int m, const F *dm, const F *center, F *out, hipStream_t st) {
    constexpr int R = NL >= 8 ? 1 : 8 / NL;
    constexpr int ROWS = R * (WAVE / LPR);
    const int64_t steps = ceil_div(n, ROWS);
    const int64_t steps_per_wg = std::max<int64_t>(SMV_WAVES, ceil_div(steps, SMV_MAX_WG));
    const int64_t rows_per_wg = steps_per_wg * ROWS;
    const int nwg = (int)ceil_div(n, rows_per_wg);
    void *ws = nullptr;
    int rc = get_workspace((size_t)nwg * m * sizeof(double), &ws, st);
    if (rc) return rc;
    double *part = static_cast<double *>(ws);
    prof_begin(st);
    hipLaunchKernelGGL((dense_sandwich_diag_kernel<F, VEC, LPR, NL, R>), dim3(nwg), dim3(SMV_THREADS),
                       (size_t)m * sizeof(double), st, X, n, m, dm, center, rows_per_wg, part);
    prof_end(st);
    TM_LAUNCH_CHECK();
    hipLaunchKernelGGL((smv_reduce_kernel<F>), dim3((unsigned)ceil_div(m, 64)), dim3(1024), 0, st, part, nwg, m, out);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

template <typename F, int VEC>
int dispatch_sdiag(const F *X, int64_t n, int m, const F *dm, const F *center, F *out, hipStream_t st) {
    const int nvec = (m + VEC - 1) / VEC;
    if (nvec <= 8) return launch_sdiag<F, VEC, 8, 1>(X, n, m, dm, center, out, st);
    if (nvec <= 16) return launch_sdiag<F, VEC, 16, 1>(X, n, m, dm, center, out, st);
    if (nvec <= 32) return launch_sdiag<F, VEC, 32, 1>(X, n, m, dm, center, out, st);
    if (nvec <= 64) return launch_sdiag<F, VEC, 64, 1>(X, n, m, dm, center, out, st);
    if (nvec <= 128) return launch_sdiag<F, VEC, 64, 2>(X, n, m, dm, center, out, st);
    if (nvec <= 256) return launch_sdiag<F, VEC, 64, 4>(X, n, m, dm, center, out, st);
    return launch_sdiag<F, VEC, 64, 8>(X, n, m, dm, center, out, st);
}

}  // namespace

template <typename F>
int run_dense_sandwich_matvec(const F *X, int64_t n, int64_t m, const F *u, const F *dm, const F *t_add,
                              const F *center, const F *shift, F *g, F *w, hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(F);
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
    TM_REQUIRE(m <= (int64_t)WAVE * V * SMV_MAX_NL, "more columns than tm_dense_sandwich_matvec serves");
    TM_REQUIRE(n == 0 || m == 0 || (X && u && dm), "X, u and dm are required");
    TM_REQUIRE(m == 0 || g, "g is required");
    if (m == 0) return TM_OK;
    if (n == 0) {
        TM_HIP(hipMemsetAsync(g, 0, (size_t)m * sizeof(F), st));
        return TM_OK;
    }
    const bool vec_ok = m % V == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    // one element per load: only widths up to 512 (64 lanes x 8 loads)
    if (!vec_ok) {
        TM_REQUIRE(m <= (int64_t)WAVE * SMV_MAX_NL, "unaligned rows: at most 512 columns");
        return dispatch_smv<F, 1>(X, n, (int)m, u, dm, t_add, center, shift, g, w, st);
    }
    return dispatch_smv<F, V>(X, n, (int)m, u, dm, t_add, center, shift, g, w, st);
}

template <typename F>
int run_dense_sandwich_diag(const F *X, int64_t n, int64_t m, const F *dm, const F *center, F *out,
                            hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(F);
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
    TM_REQUIRE(m <= (int64_t)WAVE * V * SMV_MAX_NL, "more columns than tm_dense_sandwich_diag serves");
    TM_REQUIRE(n == 0 || m == 0 || (X && dm), "X and dm are required");
    TM_REQUIRE(m == 0 || out, "out is required");
    if (m == 0) return TM_OK;
    if (n == 0) {
        TM_HIP(hipMemsetAsync(out, 0, (size_t)m * sizeof(F), st));
        return TM_OK;
    }
    const bool vec_ok = m % V == 0 && (reinterpret_cast<uintptr_t>(X) & 15) == 0;
    if (!vec_ok) {
        TM_REQUIRE(m <= (int64_t)WAVE * SMV_MAX_NL, "unaligned rows: at most 512 columns");
        return dispatch_sdiag<F, 1>(X, n, (int)m, dm, center, out, st);
    }
    return dispatch_sdiag<F, V>(X, n, (int)m, dm, center, out, st);
}

}  // namespace tmh

extern "C" {

int tm_dense_sandwich_matvec_f32(const float *X, int64_t n, int64_t m, const float *u, const float *dm,
                                 const float *t_add, const float *center, const float *shift, float *g, float *w,
                                 void *stream) {
    return tmh::run_dense_sandwich_matvec<float>(X, n, m, u, dm, t_add, center, shift, g, w, tmh::as_stream(stream));
}
int tm_dense_sandwich_matvec_f64(const double *X, int64_t n, int64_t m, const double *u, const double *dm,
                                 const double *t_add, const double *center, const double *shift, double *g,
                                 double *w, void *stream) {
    return tmh::run_dense_sandwich_matvec<double>(X, n, m, u, dm, t_add, center, shift, g, w, tmh::as_stream(stream));
}

int tm_dense_sandwich_diag_f32(const float *X, int64_t n, int64_t m, const float *dm, const float *center,
                               float *out, void *stream) {
    return tmh::run_dense_sandwich_diag<float>(X, n, m, dm, center, out, tmh::as_stream(stream));
}
int tm_dense_sandwich_diag_f64(const double *X, int64_t n, int64_t m, const double *dm, const double *center,
                               double *out, void *stream) {
    return tmh::run_dense_sandwich_diag<double>(X, n, m, dm, center, out, tmh::as_stream(stream));
}

}  // extern "C"
