// K9  GLM loss, gradient and Hessian weights in one pass over a row-major dense block (gfx950), and the same row
// function as a streaming kernel over an existing eta.
//
//   eta_r = (x_r - c) . u + shift + t_add[r]           (c, shift, t_add optional)
//   (l_r, r_r, h_r) = the family's row function of (eta_r, y_r)          (GlmRow / GlmRowP below, float64)
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
#include <cmath>

#include "dense_rowwalk.hpp"
#include "glm_math.hpp"

namespace tmh {

using namespace rowwalk;

namespace {

constexpr int GLM_ROWFN_MAX_WG = 1024;      // all resident at once (4 per CU): no tail of late workgroups

// one row of a GLM: half unit deviance l, r = dl/deta, Fisher weight h (include/tabmat_hip.h).  `family` is
// uniform over the launch: a scalar branch.  exp / log are the register-lean ones of glm_math.hpp.  The row
// function is a kernel ARGUMENT type: the four parameter-free families (GlmRow) and the two with a parameter
// (GlmRowP) are separate instantiations, so the registers of the second set are not the first set's maximum.
struct GlmRow {
    int family;
    __device__ __forceinline__ void operator()(double eta, double y, double &l, double &r, double &h) const {
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
};

// log(1 + x) for x >= 0, with the rounding of u = 1 + x put back to first order (as the binomial branch does).
// The correction is at most half an ulp of u: the bare hardware reciprocal is more than it needs.
__device__ __forceinline__ double glm_log1p_pos(double x) {
    const double u = 1.0 + x;
    return glm_log(u) + (x - (u - 1.0)) * __builtin_amdgcn_rcp(u);
}

// The families with a parameter, log link.  The constants are derived from the parameter once on the host
// (glm_param) and travel as kernel arguments: scalar registers, no memory behind them.
//   TM_GLM_TWEEDIE            c0 = 1 - p, c1 = 2 - p, c2 = 1 / ((1 - p)(2 - p)), c3 = 1 / (1 - p), c4 = 1 / (2 - p)
//   TM_GLM_NEGATIVE_BINOMIAL  c0 = theta, c1 = 1 / theta, c2 = max(0, -log theta): eta there is theta mu = 1
struct GlmRowP {
    int family;
    double c0, c1, c2, c3, c4;
    __device__ __forceinline__ void operator()(double eta, double y, double &l, double &r, double &h) const {
        if (family == TM_GLM_TWEEDIE) {
            const double a = glm_exp(c0 * eta);            // mu^(1-p)
            const double b = glm_exp(c1 * eta);            // mu^(2-p)
            const bool pos = y > 0.0;
            const double ya = pos ? y * a : 0.0;           // (y = 0 against an overflowed a: 0, not NaN)
            r = b - ya;
            h = b;
            l = (pos ? c2 * glm_exp(c1 * glm_log(y)) : 0.0) - c3 * ya + c4 * b;
        } else {  // TM_GLM_NEGATIVE_BINOMIAL
            // plain while theta mu <= 1, from e = exp(-eta) beyond (eta > c2 = max(0, -log theta)), where mu may
            // overflow while r, h and log(1 + theta mu) do not:
            //   eta <= c2: E = mu,  u = 1 + theta mu,  r = (mu - y) / u,    h = mu / u,  log(1 + theta mu) = log1p(theta mu)
            //   eta >  c2: E = e,   u = theta + e,     r = (1 - y e) / u,   h = 1 / u,   log(1 + theta mu) = eta + log u
            // (eta + log(theta + e) cancels when theta mu is small: its error would grow as eps / theta, so the
            // switch is at theta mu = 1, not at eta = 0; one exp, one division and one log either way)
            const bool big = eta > c2;
            const double E = glm_exp(big ? -eta : eta);
            const double x = c0 * E;
            const double u = big ? c0 + E : 1.0 + x;
            const double q = glm_div(1.0, u);
            const double L = (big ? eta : (x - (u - 1.0)) * q) + glm_log(u);
            r = (big ? fma(-y, E, 1.0) : E - y) * q;
            h = (big ? 1.0 : E) * q;
            l = (y > 0.0 ? y * (glm_log(y) - eta) : 0.0) - (y + c1) * (glm_log1p_pos(c0 * y) - L);
        }
    }
};

// ... with the row's weight: a zero weight SELECTS zeros (0 * inf of an overflowed row would be NaN)
template <typename ROWFN>
__device__ __forceinline__ void glm_row_weighted(const ROWFN &fn, double eta, double y, bool has_w, double w, double &l,
                                                 double &r, double &d) {
    fn(eta, y, l, r, d);
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
// of two); NL: loads per lane and row (> 1 only with LPR = 64); R: rows per lane segment and step (<= 8); ROWFN:
// GlmRow or GlmRowP.
template <typename F, int VEC, int LPR, int NL, int R, typename ROWFN>
__global__ __launch_bounds__(THREADS) void dense_glm_loss_grad_kernel(
    const F *__restrict__ X, int64_t n, int m, const F *__restrict__ u, ROWFN fn, const F *__restrict__ y,
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
            glm_row_weighted(fn, t, (double)y[row_e], wt != nullptr, wt ? (double)wt[row_e] : 1.0, le, re, de);
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

template <typename F, int VEC, typename ROWFN>
__global__ __launch_bounds__(THREADS) void glm_rowfn_kernel(ROWFN fn, const F *__restrict__ eta,
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
                    glm_row_weighted(fn, (double)ev[k][e], (double)yv[k][e], wt != nullptr,
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
            glm_row_weighted(fn, (double)eta[i], (double)y[i], wt != nullptr, wt ? (double)wt[i] : 1.0, l, r, d);
            rout[i] = (F)r;
            dout[i] = (F)d;
            lacc += l;
        }
    }
    const double s = block_sum_fixed(lacc, &slot);
    if (threadIdx.x == 0) part[blockIdx.x] = s;
}

inline bool glm_family_ok(int family) { return family >= TM_GLM_GAUSSIAN && family <= TM_GLM_GAMMA; }
inline bool glm_family_has_param(int family) { return family == TM_GLM_TWEEDIE || family == TM_GLM_NEGATIVE_BINOMIAL; }

// the constants of GlmRowP from the family's parameter; false for a parameter outside the family's domain
// (Tweedie: 1 < p < 2 or p > 2; negative binomial: theta > 0; both finite)
inline bool glm_param(int family, double param, GlmRowP &fn) {
    if (!std::isfinite(param)) return false;
    fn = GlmRowP{family, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (family == TM_GLM_TWEEDIE) {
        if (!((param > 1.0 && param < 2.0) || param > 2.0)) return false;
        fn.c0 = 1.0 - param;
        fn.c1 = 2.0 - param;
        fn.c2 = 1.0 / (fn.c0 * fn.c1);
        fn.c3 = 1.0 / fn.c0;
        fn.c4 = 1.0 / fn.c1;
        return true;
    }
    if (family == TM_GLM_NEGATIVE_BINOMIAL) {
        if (!(param > 0.0)) return false;
        fn.c0 = param;
        fn.c1 = 1.0 / param;
        fn.c2 = std::max(0.0, -std::log(param));
        return true;
    }
    return false;
}

}  // namespace

template <typename F, typename ROWFN>
int run_dense_glm_loss_grad(const F *X, int64_t n, int64_t m, const F *u, const ROWFN &fn, const F *y, const F *wt,
                            const F *t_add, const F *center, const F *shift, F *g, F *eta, F *r, F *d,
                            double *loss, hipStream_t st) {
    TM_REQUIRE(n >= 0 && m >= 0, "negative shape");
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
            hipLaunchKernelGGL((dense_glm_loss_grad_kernel<F, VEC, LPR, NL, R, ROWFN>), dim3(ge.nwg), dim3(THREADS), lds,
                               st, X, n, (int)m, u, fn, y, wt, t_add, center, shift, ge.rows_per_wg, part, eta, r, d);
        });
    });
}

template <typename F, typename ROWFN>
int run_glm_rowfn(const ROWFN &fn, const F *eta, const F *y, const F *wt, int64_t n, F *r, F *d, double *loss,
                  hipStream_t st) {
    constexpr int V = 16 / (int)sizeof(F);
    TM_REQUIRE(n >= 0, "negative length");
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
        hipLaunchKernelGGL((glm_rowfn_kernel<F, V, ROWFN>), dim3(nwg), dim3(THREADS), 0, st, fn, eta, y, wt, n, r, d,
                           part);
    else
        hipLaunchKernelGGL((glm_rowfn_kernel<F, 1, ROWFN>), dim3(nwg), dim3(THREADS), 0, st, fn, eta, y, wt, n, r, d,
                           part);
    prof_end(st);
    TM_LAUNCH_CHECK();
    hipLaunchKernelGGL((reduce_kernel<F>), dim3(1), dim3(1024), 0, st, part, nwg, 0, 1, (F *)nullptr, loss);
    TM_LAUNCH_CHECK();
    return TM_OK;
}

// the entry points: the parameter-free families run GlmRow, Tweedie and negative binomial GlmRowP.  param: a HOST
// pointer to the family's parameter, read here (NULL from the parameter-free entry points: codes 4 and 5 are then
// unknown families).  family and *param are checked before anything is launched.
template <typename F>
int dense_glm_loss_grad_entry(const F *X, int64_t n, int64_t m, const F *u, int family, const double *param,
                              const F *y, const F *wt, const F *t_add, const F *center, const F *shift, F *g, F *eta,
                              F *r, F *d, double *loss, void *stream) {
    if (glm_family_has_param(family) && param) {
        GlmRowP fn;
        TM_REQUIRE(glm_param(family, *param, fn), "family parameter outside its domain");
        return run_dense_glm_loss_grad<F>(X, n, m, u, fn, y, wt, t_add, center, shift, g, eta, r, d, loss,
                                          as_stream(stream));
    }
    TM_REQUIRE(glm_family_ok(family), "unknown family (tweedie and negative_binomial: the *_p entry points, with param)");
    return run_dense_glm_loss_grad<F>(X, n, m, u, GlmRow{family}, y, wt, t_add, center, shift, g, eta, r, d, loss,
                                      as_stream(stream));
}

template <typename F>
int glm_rowfn_entry(int family, const double *param, const F *eta, const F *y, const F *wt, int64_t n, F *r,
                    F *d, double *loss, void *stream) {
    if (glm_family_has_param(family) && param) {
        GlmRowP fn;
        TM_REQUIRE(glm_param(family, *param, fn), "family parameter outside its domain");
        return run_glm_rowfn<F>(fn, eta, y, wt, n, r, d, loss, as_stream(stream));
    }
    TM_REQUIRE(glm_family_ok(family), "unknown family (tweedie and negative_binomial: the *_p entry points, with param)");
    return run_glm_rowfn<F>(GlmRow{family}, eta, y, wt, n, r, d, loss, as_stream(stream));
}

}  // namespace tmh

extern "C" {

int tm_dense_glm_loss_grad_f32(const float *X, int64_t n, int64_t m, const float *u, int family, const float *y,
                               const float *wt, const float *t_add, const float *center, const float *shift,
                               float *g, float *eta, float *r, float *d, double *loss, void *stream) {
    return tmh::dense_glm_loss_grad_entry<float>(X, n, m, u, family, nullptr, y, wt, t_add, center, shift, g, eta,
                                                 r, d, loss, stream);
}
int tm_dense_glm_loss_grad_f64(const double *X, int64_t n, int64_t m, const double *u, int family, const double *y,
                               const double *wt, const double *t_add, const double *center, const double *shift,
                               double *g, double *eta, double *r, double *d, double *loss, void *stream) {
    return tmh::dense_glm_loss_grad_entry<double>(X, n, m, u, family, nullptr, y, wt, t_add, center, shift, g, eta,
                                                  r, d, loss, stream);
}
int tm_dense_glm_loss_grad_p_f32(const float *X, int64_t n, int64_t m, const float *u, int family, const double *param,
                                 const float *y, const float *wt, const float *t_add, const float *center,
                                 const float *shift, float *g, float *eta, float *r, float *d, double *loss,
                                 void *stream) {
    return tmh::dense_glm_loss_grad_entry<float>(X, n, m, u, family, param, y, wt, t_add, center, shift, g, eta,
                                                 r, d, loss, stream);
}
int tm_dense_glm_loss_grad_p_f64(const double *X, int64_t n, int64_t m, const double *u, int family, const double *param,
                                 const double *y, const double *wt, const double *t_add, const double *center,
                                 const double *shift, double *g, double *eta, double *r, double *d, double *loss,
                                 void *stream) {
    return tmh::dense_glm_loss_grad_entry<double>(X, n, m, u, family, param, y, wt, t_add, center, shift, g,
                                                  eta, r, d, loss, stream);
}

int tm_glm_rowfn_f32(int family, const float *eta, const float *y, const float *wt, int64_t n, float *r, float *d,
                     double *loss, void *stream) {
    return tmh::glm_rowfn_entry<float>(family, nullptr, eta, y, wt, n, r, d, loss, stream);
}
int tm_glm_rowfn_f64(int family, const double *eta, const double *y, const double *wt, int64_t n, double *r,
                     double *d, double *loss, void *stream) {
    return tmh::glm_rowfn_entry<double>(family, nullptr, eta, y, wt, n, r, d, loss, stream);
}
int tm_glm_rowfn_p_f32(int family, const double *param, const float *eta, const float *y, const float *wt, int64_t n,
                       float *r, float *d, double *loss, void *stream) {
    return tmh::glm_rowfn_entry<float>(family, param, eta, y, wt, n, r, d, loss, stream);
}
int tm_glm_rowfn_p_f64(int family, const double *param, const double *eta, const double *y, const double *wt, int64_t n,
                       double *r, double *d, double *loss, void *stream) {
    return tmh::glm_rowfn_entry<double>(family, param, eta, y, wt, n, r, d, loss, stream);
}

}  // extern "C"
