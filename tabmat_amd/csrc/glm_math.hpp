// float64 exp and log for the GLM row functions (glm.hip), written for a SMALL register footprint: K9 evaluates
// them while eight rows of X wait in registers, and the library routines take 30 .. 45 vector registers each
// (plus the rows: half of K8's waves per SIMD).  Horner chains whose coefficients are literals: a handful of
// live registers each.  About 1 ulp (checked against long double on the host: this header compiles
// there too).
#pragma once

#include <math.h>

#ifdef __HIPCC__
#define TM_HD __host__ __device__ __forceinline__
#else
#define TM_HD inline
#endif

namespace tmh {

// GLM_C(c): the float64 literal c, materialised in a scalar register pair right where it is used.  The vector
// float64 instructions of gfx950 take no 64-bit literal, and left alone the compiler parks every coefficient of
// the chains below in registers for the whole row loop (~60 vector registers, or the scalar file to its
// limit): that, not the arithmetic, is what costs the waves.  Two scalar moves per coefficient and
// evaluation instead; volatile keeps them from being hoisted back out of the loop.
#ifdef __HIP_DEVICE_COMPILE__
template <unsigned long long BITS>
__device__ __forceinline__ double glm_const_bits() {
    unsigned lo, hi;
    asm volatile("s_mov_b32 %0, %2\n\ts_mov_b32 %1, %3"
                 : "=s"(lo), "=s"(hi)
                 : "i"((unsigned)(BITS & 0xffffffffull)), "i"((unsigned)(BITS >> 32)));
    return __hiloint2double((int)hi, (int)lo);
}
#define GLM_C(c) tmh::glm_const_bits<__builtin_bit_cast(unsigned long long, (double)(c))>()
#else
#define GLM_C(c) ((double)(c))
#endif

// n / d for a d of moderate size (no scaling step: d neither overflows nor underflows its reciprocal): the
// hardware reciprocal, two Newton steps and one correction of the quotient -- fewer instructions and live
// registers than the general float64 division.
TM_HD double glm_div(double n, double d) {
#ifdef __HIP_DEVICE_COMPILE__
    double r = __builtin_amdgcn_rcp(d);
    r = fma(fma(-d, r, 1.0), r, r);
    r = fma(fma(-d, r, 1.0), r, r);
    const double q = n * r;
    return fma(fma(-d, q, n), r, q);
#else
    return n / d;
#endif
}

// exp(x): x = k ln2 + r with |r| <= ln2 / 2, the degree-13 Taylor polynomial of exp(r) (remainder 4e-18) and
// a scaling by 2^k that overflows to inf and underflows through the denormals to 0.  NaN stays NaN.
TM_HD double glm_exp(double x) {
    const double xc = fmin(fmax(x, -800.0), 800.0);    // beyond: inf / 0 anyway, and k stays a small integer
    const double k = rint(xc * GLM_C(1.4426950408889634074));
    double r = fma(k, GLM_C(-6.93147180369123816490e-01), xc);   // ln2 high part: 32 trailing zero bits
    r = fma(k, GLM_C(-1.90821492927058770002e-10), r);
    double p = GLM_C(1.6059043836821614599e-10);       // 1 / 13!
    p = fma(p, r, GLM_C(2.0876756987868098979e-09));
    p = fma(p, r, GLM_C(2.5052108385441718775e-08));
    p = fma(p, r, GLM_C(2.7557319223985890653e-07));
    p = fma(p, r, GLM_C(2.7557319223985890653e-06));
    p = fma(p, r, GLM_C(2.4801587301587301587e-05));
    p = fma(p, r, GLM_C(1.9841269841269841270e-04));
    p = fma(p, r, GLM_C(1.3888888888888888889e-03));
    p = fma(p, r, GLM_C(8.3333333333333333333e-03));
    p = fma(p, r, GLM_C(4.1666666666666666667e-02));
    p = fma(p, r, GLM_C(1.6666666666666666667e-01));
    p = fma(p, r, 0.5);
    p = fma(p, r, 1.0);
    p = fma(p, r, 1.0);
    const double v = ldexp(p, (int)k);
    return x != x ? x : v;
}

// log(x) for x > 0 (0 gives -inf; the GLM domains exclude x < 0): x = 2^k m with m in [sqrt(1/2), sqrt(2)),
// f = m - 1, s = f / (2 + f), log(m) = f - f^2/2 + s (f^2/2 + R(s^2)) with the degree-7 minimax R of fdlibm's
// e_log.c (|error| < 2^-58.45), plus k ln2 in two parts.
TM_HD double glm_log(double x) {
    int e;
    double m = frexp(x, &e);                           // [0.5, 1)
    const bool low = m < GLM_C(0.70710678118654752440);
    m = low ? m + m : m;
    const double k = (double)(low ? e - 1 : e);
    const double f = m - 1.0;
    const double s = glm_div(f, 2.0 + f);            // 2 + f in [1.7, 2.5)
    const double z = s * s;
    double R = GLM_C(1.479819860511658591e-01);
    R = fma(R, z, GLM_C(1.531383769920937332e-01));
    R = fma(R, z, GLM_C(1.818357216161805012e-01));
    R = fma(R, z, GLM_C(2.222219843214978396e-01));
    R = fma(R, z, GLM_C(2.857142874366239149e-01));
    R = fma(R, z, GLM_C(3.999999999940941908e-01));
    R = fma(R, z, GLM_C(6.666666666666735130e-01));
    R *= z;
    const double hfsq = 0.5 * f * f;
    const double v = k * GLM_C(6.93147180369123816490e-01) -
                     ((hfsq - (s * (hfsq + R) + k * GLM_C(1.90821492927058770002e-10))) - f);
    return x == 0.0 ? -HUGE_VAL : (x != x || x > 1.7976931348623157e308) ? x : v;
}

}  // namespace tmh
