// K9  GLM loss, gradient and Hessian weights in one pass over a row-major dense block (gfx950), and the same row
// function as a streaming kernel over an existing eta.
//
//   eta_r = (x_r - c) . u + shift + t_add[r]           (c, shift, t_add optional)
//   (l_r, r_r, h_r) = the family's row function of (eta_r, y_r)          (glm_row below, float64)
//   r[r] = wt_r r_r     d[r] = wt_r h_r     loss = sum_r wt_r l_r     g = sum_r (x_r - c) wt_r r_r
//
// The row walk is the shared one (dense_rowwalk.hpp): a wave loads R rows per lane segment into registers, reduces
// the dot products across the lanes of each row, and adds x_r r_r into per-lane column accumulators while the
// rows are still in registers.  Between the two the row function runs ONCE per wave step: after the reduction every
// lane of a segment holds the R row sums of that segment, so lane k of the segment (k < R <= 8 <= LPR) takes row
// k -- a register select, nothing crosses lanes -- and a step's R * (64 / LPR) rows are evaluated side by side in
// as many lanes.  r then goes back to the row's lanes (v_readlane when a row spans the wave, ds_bpermute
// otherwise).  One exp / log sequence per 8 KB of X instead of one per row.
//
// Sums are fixed-order: per-workgroup partials of g plus one loss slot, finished by a second launch.  No
// floating-point atomics; results are bitwise reproducible.
#include "dense_rowwalk.hpp"
#include "glm_math.hpp"

namespace tmh {

using namespace rowwalk;

namespace {

constexpr int GLM_ROWFN_MAX_WG = 1024;      // all resident at once (4 per CU): no tail of late workgroups

// one row of a GLM: half unit deviance l, r = dl/deta, Fisher weight h (include/tabmat_hip.h).  `family` is
// uniform over the launch: a scalar branch.  exp / log are the register-lean ones of glm_math.hpp.
__device__ __forceinline__ void glm_row(int family, double eta, double y, double &l, double &r, double &h) {
    switch (family) {
    case TM_GLM_GAUSSIAN: {
        r = eta - y;
        l = 0.5 * r * r;
        h = 1.0;
        break;
    }
    case TM_GLM_POISSON: {
        const double mu = glm_exp(eta);
        r = mu - y;
        l = (y > 0.0 ? y * (glm_log(y) - eta) : 0.0) - (y - mu);
        h = mu;
        break;
    }
    case TM_GLM_BINOMIAL: {
        const double e = glm_exp(-fabs(eta));          // (0, 1]
        const double u = 1.0 + e;
        const double q = glm_div(1.0, u);
        const double mu = eta >= 0.0 ? q : e * q;
        const double z = 1.0 - y;
        // log1p(e) = log(u) + (e - (u - 1)) / u: the rounding of 1 + e, put back to first order
        l = fmax(eta, 0.0) + (glm_log(u) + (e - (u - 1.0)) * q) - y * eta;
        l += y > 0.0 ? y * glm_log(y) : 0.0;
        l += z > 0.0 ? z * glm_log(z) : 0.0;
        r = mu - y;
        h = e * q * q;
        break;
    }
    default: {  // TM_GLM_GAMMA
        const double ye = y * glm_exp(-eta);
        r = 1.0 - ye;
        l = ye - 1.0 - glm_log(y) + eta;
        h = 1.0;
        break;
    }
    }
}

// ... with the row's weight: a zero weight SELECTS zeros (0 * inf of an overflowed row would be NaN)
__device__ __forceinline__ void glm_row_weighted(int family, double eta, double y, bool has_w, double w, double &l,
                                                 double &r, double &d) {
    glm_row(family, eta, y, l, r, d);
    if (has_w) {
        const bool zero = w == 0.0;
        l = zero ? 0.0 : w * l;
        r = zero ? 0.0 : w * r;
        d = zero ? 0.0 : w * d;
    }
}

// the value lane K of the own row segment holds, in every lane of the segment
template <int LPR, int K>
__device__ __forceinline__ double segment_bcast(double v, int seg) {
    if constexpr (LPR == WAVE) {
        return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), K),
                                __builtin_amdgcn_readlane(__double2loint(v), K));
    } else {
        return __shfl(v, seg * LPR + K, 64);
    }
}

// fixed-order sum of one double per thread over the workgroup: xor tree in the wave, then the waves one after
// the other through `slot` (shared); valid in every thread after the call
__device__ __forceinline__ double block_sum_fixed(double v, double *slot) {
#pragma unroll
    for (int s = 1; s < WAVE; s <<= 1) v += __shfl_xor(v, s, 64);
    const int lane = threadIdx.x & (WAVE - 1);
    const int wave = threadIdx.x / WAVE;
    for (int wv = 0; wv < WAVES; ++wv) {
        if (wave == wv && lane == 0) *slot = wv == 0 ? v : *slot + v;
        __syncthreads();
    }
    return *slot;
}

// VEC: elements per load (16 / sizeof(F) on 16-byte aligned rows, 1 else); LPR: lanes per row (8 .. 64, a power
// of two); NL: loads per lane and row (> 1 only with LPR = 64); R: rows per lane segment and step (<= 8).
template <typename F, int VEC, int LPR, int NL, int R>
__global__ __launch_bounds__(THREADS) void dense_glm_loss_grad_kernel(
    const F *__restrict__ X, int64_t n, int m, const F *__restrict__ u, int family, const F *__restrict__ y,
    const F *__restrict__ wt, const F *__restrict__ t_add, const F *__restrict__ center,
    const F *__restrict__ shift, int64_t rows_per_wg, double *__restrict__ part, F *__restrict__ eta,
    F *__restrict__ rout, F *__restrict__ dout) {
    typedef F vec_t __attribute__((ext_vector_type(VEC)));
    static_assert(R <= 8 && R <= LPR, "lane k of a segment evaluates the segment's row k");
    constexpr int RPL = WAVE / LPR;                    // row segments of a wave
    constexpr int ROWS = R * RPL;                      // rows of one wave step
    extern __shared__ double glm_red[];                // m + 1 doubles
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
    double lacc = 0.0;                                 // this lane's share of the loss

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
        // lane sl < R of a segment evaluates the segment's row sl
        const int64_t row_e = r0 + (int64_t)sl * RPL + seg;
        const bool ev = sl < R && row_e < r_end;
        double tsel = 0.0;
#pragma unroll
        for (int r = 0; r < R; ++r) {
            double p = 0.0;
#pragma unroll
            for (int q = 0; q < NL; ++q)
#pragma unroll
                for (int e = 0; e < VEC; ++e) p = fma((double)x[r][q][e] - (double)cc[q][e], (double)uu[q][e], p);
            const double t = segment_allreduce<LPR>(p);
            tsel = sl == r ? t : tsel;
        }
        // rows past the end (clamped loads) get r = 0 and are not written
        double re = 0.0;
        if (ev) {
            const double t = tsel + s0 + (t_add ? (double)t_add[row_e] : 0.0);
            double le, de;
            glm_row_weighted(family, t, (double)y[row_e], wt != nullptr, wt ? (double)wt[row_e] : 1.0, le, re, de);
            eta[row_e] = (F)t;
            rout[row_e] = (F)re;
            dout[row_e] = (F)de;
            lacc += le;
        }
        static_for<R>([&](auto rc) {
            constexpr int r = decltype(rc)::value;
            const double wr = segment_bcast<LPR, r>(re, seg);
#pragma unroll
            for (int q = 0; q < NL; ++q)
                if (live[q]) {
#pragma unroll
                    for (int e = 0; e < VEC; ++e) acc[q][e] = fma((double)x[r][q][e] - (double)cc[q][e], wr, acc[q][e]);
                }
        });
    }

    fold_columns<LPR>(acc, live, glm_red);
    block_sum_fixed(lacc, &glm_red[m]);
    store_partial(glm_red, part, m + 1);
}

// the row function over an existing eta: grid-stride over vectors of VEC elements, GLM_ROWFN_U independent
// vectors per thread and step (their loads are issued together: the resident grid is 4 waves per SIMD, one
// vector each would not cover the memory latency); one loss partial per workgroup
constexpr int GLM_ROWFN_U = 4;

template <typename F, int VEC>
__global__ __launch_bounds__(THREADS) void glm_rowfn_kernel(int family, const F *__restrict__ eta,
                                                             const F *__restrict__ y, const F *__restrict__ wt,
                                                             int64_t n, F *__restrict__ rout,
                                                             F *__restrict__ dout, double *__restrict__ part) {
    typedef F vec_t __attribute__((ext_vector_type(VEC)));
    constexpr int U = GLM_ROWFN_U;
    __shared__ double slot;
    const int64_t nfull = n / VEC;                     // whole vectors
    double lacc = 0.0;
    for (int64_t v0 = (int64_t)blockIdx.x * (THREADS * U) + threadIdx.x; v0 < nfull;
         v0 += (int64_t)gridDim.x * (THREADS * U)) {
        vec_t ev[U], yv[U], wv[U];
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t v = v0 + (int64_t)k * THREADS;
            if (v < nfull) {
                ev[k] = *reinterpret_cast<const vec_t *>(eta + v * VEC);
                yv[k] = *reinterpret_cast<const vec_t *>(y + v * VEC);
                if (wt) wv[k] = *reinterpret_cast<const vec_t *>(wt + v * VEC);
            }
        }
#pragma unroll
        for (int k = 0; k < U; ++k) {
            const int64_t v = v0 + (int64_t)k * THREADS;
            if (v < nfull) {
                vec_t rv, dv;
#pragma unroll
                for (int e = 0; e < VEC; ++e) {
                    double l, r, d;
                    glm_row_weighted(family, (double)ev[k][e], (double)yv[k][e], wt != nullptr,
                                     wt ? (double)wv[k][e] : 1.0, l, r, d);
                    rv[e] = (F)r;
                    dv[e] = (F)d;
                    lacc += l;
                }
                *reinterpret_cast<vec_t *>(rout + v * VEC) = rv;
                *reinterpret_cast<vec_t *>(dout + v * VEC) = dv;
            }
        }
    }
    // the n % VEC elements after the last whole vector
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        for (int64_t i = nfull * VEC; i < n; ++i) {
            double l, r, d;
            glm_row_weighted(family, (double)eta[i], (double)y[i], wt != nullptr, wt ? (double)wt[i] : 1.0, l, r, d);
            rout[i] = (F)r;
            dout[i] = (F)d;
            lacc += l;
        }
    }
    const double s = block_sum_fixed(lacc, &slot);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

inline bool glm_family_ok(int family) { return family >= TM_GLM_GAUSSIAN && family <= TM_GLM_GAMMA; }

}  // namespace

template <typename F>
int run_dense_glm_loss_grad(const F *X, int64_t n, int64_t m, const F *u, int family, const F *y, const F *wt,
                            const F *t_add, const F *center, const F *shift, F *g, F *eta, F *r, F *d,
                            double *loss, hipStream_t st) {
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
    TM_REQUIRE(glm_family_ok(family), "unknown family");
    TM_REQUIRE(m > 0, "a block without columns has no row walk: use tm_glm_rowfn");
    TM_REQUIRE(m <= max_columns(FULL_VEC<F>), "more columns than tm_dense_glm_loss_grad serves");
    TM_REQUIRE(g && loss, "g and loss are required");
    TM_REQUIRE(n == 0 || (X && u && y && eta && r && d), "X, u, y, eta, r and d are required");
    if (n == 0) {
        TM_HIP(hipMemsetAsync(g, 0, (size_t)m * sizeof(F), st));
        TM_HIP(hipMemsetAsync(loss, 0, sizeof(double), st));
        return TM_OK;
    }
    const int vec = load_form(X, m);
    TM_REQUIRE(vec != 0, "unaligned rows: at most 512 columns");
    return dispatch<F>(vec, (int)m, [&](auto v, auto lpr, auto nl) {
        constexpr int VEC = decltype(v)::value, LPR = decltype(lpr)::value, NL = decltype(nl)::value;
        constexpr int R = rows_per_segment(NL);
        return launch<F>(n, (int)m, 1, R * (WAVE / LPR), g, loss, st, [&](Geometry ge, size_t lds, double *part) {
            hipLaunchKernelGGL((dense_glm_loss_grad_kernel<F, VEC, LPR, NL, R>), dim3(ge.nwg), dim3(THREADS), lds, st,
                               X, n, (int)m, u, family, y, wt, t_add, center, shift, ge.rows_per_wg, part, eta, r, d);
        });
    });
}

template <typename F>
int run_glm_rowfn(int family, const F *eta, const F *y, const F *wt, int64_t n, F *r, F *d, double *loss,
                  hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(F);
    TM_REQUIRE(n >= 0, "negative length");
    TM_REQUIRE(glm_family_ok(family), "unknown family");
    TM_REQUIRE(loss, "loss is required");
    TM_REQUIRE(n == 0 || (eta && y && r && d), "eta, y, r and d are required");
    if (n == 0) {
        TM_HIP(hipMemsetAsync(loss, 0, sizeof(double), st));
        return TM_OK;
    }
    const uintptr_t bits = reinterpret_cast<uintptr_t>(eta) | reinterpret_cast<uintptr_t>(y) |
                           reinterpret_cast<uintptr_t>(wt) | reinterpret_cast<uintptr_t>(r) |
                           reinterpret_cast<uintptr_t>(d);
    const bool vec_ok = (bits & 15) == 0;
    const int64_t nv = vec_ok ? ceil_div(n, V) : n;
    const int nwg = (int)std::min<int64_t>(GLM_ROWFN_MAX_WG, ceil_div(nv, THREADS * GLM_ROWFN_U));
    void *ws = nullptr;
    int rc = get_workspace((size_t)nwg * sizeof(double), &ws, st);
    if (rc) return rc;
    double *part = static_cast<double *>(ws);
    prof_begin(st);
    if (vec_ok)
        hipLaunchKernelGGL((glm_rowfn_kernel<F, V>), dim3(nwg), dim3(THREADS), 0, st, family, eta, y, wt, n, r, d,
                           part);
    else
        hipLaunchKernelGGL((glm_rowfn_kernel<F, 1>), dim3(nwg), dim3(THREADS), 0, st, family, eta, y, wt, n, r, d,
                           part);
    prof_end(st);
    TM_LAUNCH_CHECK();
    hipLaunchKernelGGL((reduce_kernel<F>), dim3(1), dim3(1024), 0, st, part, nwg, 0, 1, (F *)nullptr, loss);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

}  // namespace tmh

extern "C" {

int tm_dense_glm_loss_grad_f32(const float *X, int64_t n, int64_t m, const float *u, int family, const float *y,
                               const float *wt, const float *t_add, const float *center, const float *shift,
                               float *g, float *eta, float *r, float *d, double *loss, void *stream) {
    return tmh::run_dense_glm_loss_grad<float>(X, n, m, u, family, y, wt, t_add, center, shift, g, eta, r, d, loss,
                                               tmh::as_stream(stream));
}
int tm_dense_glm_loss_grad_f64(const double *X, int64_t n, int64_t m, const double *u, int family, const double *y,
                               const double *wt, const double *t_add, const double *center, const double *shift,
                               double *g, double *eta, double *r, double *d, double *loss, void *stream) {
    return tmh::run_dense_glm_loss_grad<double>(X, n, m, u, family, y, wt, t_add, center, shift, g, eta, r, d, loss,
                                                tmh::as_stream(stream));
}

int tm_glm_rowfn_f32(int family, const float *eta, const float *y, const float *wt, int64_t n, float *r, float *d,
                     double *loss, void *stream) {
    return tmh::run_glm_rowfn<float>(family, eta, y, wt, n, r, d, loss, tmh::as_stream(stream));
}
int tm_glm_rowfn_f64(int family, const double *eta, const double *y, const double *wt, int64_t n, double *r,
                     double *d, double *loss, void *stream) {
    return tmh::run_glm_rowfn<double>(family, eta, y, wt, n, r, d, loss, tmh::as_stream(stream));
}

}  // extern "C"
