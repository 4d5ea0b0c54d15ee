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
#include "dense_rowwalk.hpp"

namespace tmh {

using namespace rowwalk;

namespace {

// VEC: elements per load (16 / sizeof(F) on 16-byte aligned rows, 1 else); LPR: lanes per row (8 .. 64,
// a power of two); NL: loads per lane and row (> 1 only with LPR = 64); R: rows per lane segment and step.
template <typename F, int VEC, int LPR, int NL, int R>
__global__ __launch_bounds__(THREADS) void dense_sandwich_matvec_kernel(
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

    F uu[NL][VEC], cc[NL][VEC];
    double acc[NL][VEC];
    bool live[NL];
    lane_columns<LPR>(m, sl, center, live, cc, acc);
    lane_u<LPR>(m, sl, u, uu);
    const double s0 = shift ? (double)shift[0] : 0.0;

    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r_end = min(r_begin + rows_per_wg, n);
    for (int64_t r0 = r_begin + (int64_t)wave * ROWS; r0 < r_end; r0 += (int64_t)WAVES * ROWS) {
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

    fold_columns<LPR>(acc, live, smv_red);
    store_partial(smv_red, part, m);
}

// K8d  the diagonal of the same product: acc_j += dm[r] (x_rj - c_j)^2.  K8's row walk, registers and fold without
// the dot product (nothing crosses lanes inside the loop); the partials go through the same reduce kernel.
template <typename F, int VEC, int LPR, int NL, int R>
__global__ __launch_bounds__(THREADS) void dense_sandwich_diag_kernel(
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
    lane_columns<LPR>(m, sl, center, live, cc, acc);

    const int64_t r_begin = (int64_t)blockIdx.x * rows_per_wg;
    const int64_t r_end = min(r_begin + rows_per_wg, n);
    for (int64_t r0 = r_begin + (int64_t)wave * ROWS; r0 < r_end; r0 += (int64_t)WAVES * ROWS) {
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

    fold_columns<LPR>(acc, live, smv_red);
    store_partial(smv_red, part, m);
}

}  // namespace

template <typename F>
int run_dense_sandwich_matvec(const F *X, int64_t n, int64_t m, const F *u, const F *dm, const F *t_add,
                              const F *center, const F *shift, F *g, F *w, hipStream_t st) {
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
    TM_REQUIRE(m <= max_columns(FULL_VEC<F>), "more columns than tm_dense_sandwich_matvec serves");
    TM_REQUIRE(n == 0 || m == 0 || (X && u && dm), "X, u and dm are required");
    TM_REQUIRE(m == 0 || g, "g is required");
    if (m == 0) return TM_OK;
    if (n == 0) {
        TM_HIP(hipMemsetAsync(g, 0, (size_t)m * sizeof(F), st));
        return TM_OK;
    }
    const int vec = load_form(X, m);
    TM_REQUIRE(vec != 0, "unaligned rows: at most 512 columns");
    return dispatch<F>(vec, (int)m, [&](auto v, auto lpr, auto nl) {
        constexpr int VEC = decltype(v)::value, LPR = decltype(lpr)::value, NL = decltype(nl)::value;
        constexpr int R = rows_per_segment(NL);
        return launch<F>(n, (int)m, 0, R * (WAVE / LPR), g, nullptr, st, [&](Geometry ge, size_t lds, double *part) {
            hipLaunchKernelGGL((dense_sandwich_matvec_kernel<F, VEC, LPR, NL, R>), dim3(ge.nwg), dim3(THREADS), lds, st,
                               X, n, (int)m, u, dm, t_add, center, shift, ge.rows_per_wg, part, w);
        });
    });
}

template <typename F>
int run_dense_sandwich_diag(const F *X, int64_t n, int64_t m, const F *dm, const F *center, F *out,
                            hipStream_t st) {
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
    TM_REQUIRE(m <= max_columns(FULL_VEC<F>), "more columns than tm_dense_sandwich_diag serves");
    TM_REQUIRE(n == 0 || m == 0 || (X && dm), "X and dm are required");
    TM_REQUIRE(m == 0 || out, "out is required");
    if (m == 0) return TM_OK;
    if (n == 0) {
        TM_HIP(hipMemsetAsync(out, 0, (size_t)m * sizeof(F), st));
        return TM_OK;
    }
    const int vec = load_form(X, m);
    TM_REQUIRE(vec != 0, "unaligned rows: at most 512 columns");
    return dispatch<F>(vec, (int)m, [&](auto v, auto lpr, auto nl) {
        constexpr int VEC = decltype(v)::value, LPR = decltype(lpr)::value, NL = decltype(nl)::value;
        constexpr int R = rows_per_segment(NL);
        return launch<F>(n, (int)m, 0, R * (WAVE / LPR), out, nullptr, st, [&](Geometry ge, size_t lds, double *part) {
            hipLaunchKernelGGL((dense_sandwich_diag_kernel<F, VEC, LPR, NL, R>), dim3(ge.nwg), dim3(THREADS), lds, st,
                               X, n, (int)m, dm, center, ge.rows_per_wg, part);
        });
    });
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
