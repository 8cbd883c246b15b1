// mp_math.h — deterministic fp64 exp/log shared by the gfx950 kernels and by the
// host-side checker.
//
// Why this exists: modppl's CPU path calls libm (`f64::exp`, `f64::ln`:
// modppl/src/lib.rs:41-43, modeling/dists/normal.rs:16,25).  glibc's exp/log and ROCm's
// ocml exp/log differ in the last ulp on a small fraction of inputs, and a one-ulp change in
// one weight can move a resample index.  Bit-exact resample indices between the device and a
// CPU checker therefore need ONE definition of exp and log that is evaluated with the same
// IEEE-754 operations, in the same order, on both sides.  Everything here uses only
// + - * / fma rint and integer bit manipulation; compile with -ffp-contract=off on both
// sides so that no other contraction happens.
//
// Accuracy (measured in tests/test_math.py against 80-bit long double): < 1 ulp.
//   mp_exp: Cody–Waite reduction by ln2 (hi/lo) + degree-13 Taylor polynomial, fma Horner.
//   mp_log: the classical fdlibm e_log.c scheme (argument reduced to [sqrt(2)/2, sqrt(2)),
//           s = f/(2+f), even/odd split minimax polynomial Lg1..Lg7).  fdlibm is
//           "Copyright (C) 1993 by Sun Microsystems, Inc. Permission to use, copy, modify,
//           and distribute this software is freely granted, provided that this notice is
//           preserved."  Only the published constants and the scheme are used.
#pragma once
#include <stdint.h>
#include <math.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define MP_HD __host__ __device__ __forceinline__
#else
#define MP_HD inline
#endif

MP_HD uint64_t mp_f2u(double x) { return __builtin_bit_cast(uint64_t, x); }
MP_HD double mp_u2f(uint64_t u) { return __builtin_bit_cast(double, u); }

#define MP_INF (mp_u2f(0x7FF0000000000000ull))
#define MP_NEG_INF (mp_u2f(0xFFF0000000000000ull))
#define MP_2PI 6.283185307179586      /* 2*pi as the reference computes it: 2.*PI */
#define MP_PI 3.141592653589793

// ---------------------------------------------------------------------------------------
// One fp64 operation with a compile-time constant C as an operand.  gfx950 has no 64-bit literal operand, and left to itself the
// compiler puts every such constant into a VGPR pair first (two v_mov_b32 in front of each Horner step: three VALU issues for one
// operation).  On the device the constant goes through an "s" constraint instead: two s_mov_b32 on the scalar unit (still
// rematerialisable: no live range grows) and ONE v_fma_f64 / v_add_f64 / v_mul_f64 with an SGPR-pair operand — the same IEEE
// operation on the same operands, so the same bits.  One scalar operand per instruction is what VOP3 allows here; a and b are
// run-time values.  On the host these are fma, + and * themselves.
//   mp_fma_c(a, b, C) = fma(a, b, C)     mp_fnma_c(a, C, c) = fma(-a, C, c)     mp_add_c(a, C) = C + a     mp_mul_c(a, C) = a * C
// C MUST be a literal (or a constexpr double): an "s" operand is one value per wave, so for a C that differs from lane to lane the
// compiler would take lane 0's (v_readfirstlane) for all 64 without a word.  The language gives no way to demand that of a double
// argument in C++17; every use is a named constant a few lines above it, and a new one has to be as well.  The results are ordinary
// VGPR values; the compiler pads the wait states between one of these and a DPP instruction of its own that reads the result.
// ---------------------------------------------------------------------------------------
#if defined(__HIP_DEVICE_COMPILE__)
__device__ __forceinline__ double mp_fma_c(double a, double b, double C) {
    double r;
    asm("v_fma_f64 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(C));
    return r;
}
__device__ __forceinline__ double mp_fnma_c(double a, double C, double c) {
    double r;
    asm("v_fma_f64 %0, -%1, %2, %3" : "=v"(r) : "v"(a), "s"(C), "v"(c));
    return r;
}
__device__ __forceinline__ double mp_add_c(double a, double C) {
    double r;
    asm("v_add_f64 %0, %1, %2" : "=v"(r) : "s"(C), "v"(a));
    return r;
}
__device__ __forceinline__ double mp_mul_c(double a, double C) {
    double r;
    asm("v_mul_f64 %0, %1, %2" : "=v"(r) : "v"(a), "s"(C));
    return r;
}
#else
MP_HD double mp_fma_c(double a, double b, double C) { return fma(a, b, C); }
MP_HD double mp_fnma_c(double a, double C, double c) { return fma(-a, C, c); }
MP_HD double mp_add_c(double a, double C) { return C + a; }
MP_HD double mp_mul_c(double a, double C) { return a * C; }
#endif
// ... or, SC = false, the plain expression (the compiler's own choice of registers).  Same operation either way.  The scalar form
// is for the hot per-particle chains only (mp_exp, mp_exp_nonpos, the logarithm of the narrow models' deviates).  mp_log's other
// uses — the one-thread folds of the tile scalars, model constants, the wide models' sixteen deviates per particle — keep the plain
// form: with inline assembly in them the compiler compiled k_propagate<mp_lgssm_band<16>, 512> into half as many instructions but
// with three times the SGPR spills (v_writelane 30 -> 93, v_readlane 62 -> 204), and it ran 438 -> 491 us per step.
template <bool SC> MP_HD double mp_add_cs(double a, double C) { if constexpr (SC) return mp_add_c(a, C); else return C + a; }
template <bool SC> MP_HD double mp_mul_cs(double a, double C) { if constexpr (SC) return mp_mul_c(a, C); else return a * C; }

// ---------------------------------------------------------------------------------------
// x / d with the reciprocal r = RN(1 / d) hoisted (d is a model constant: an observation noise, a drift width): the bits of the
// IEEE division without the division.  q0 = RN(x r) is within two ulps of x / d; one residual correction (rem = x - q0 d, exact
// in an fma) makes it faithful, a second one correctly rounded (Markstein's theorem: correct rounding from a faithful quotient
// and the correctly rounded reciprocal; the one exception, a divisor whose significand is all ones, is refused by the hoisting
// side: mp_rcp_hoistable).  mp_div_hoisted falls back to the division itself outside 2^-900 < |x| < 2^900 (zero, subnormal
// neighbourhoods, infinities, NaN); a log-density needs no fallback (mp_normal_logpdf_h): where the branch-free core is not the
// division's bits the quotient's SQUARE underflows to zero or overflows to infinity either way.
// 5 full-rate instructions against ~13 with a quarter-rate v_rcp_f64 (tools/func_cost.hip: 88 -> 25 cycles per wave).
// Checked bit for bit against `/` on 2^24 random numerators per divisor on host and device (tests/test_math.py, test_gpu_math.py).
// ---------------------------------------------------------------------------------------
// The corrected quotient, branch-free: exact (= RN(x / d)) for 2^-960 < |x| < 2^960; an infinite or NaN x r is passed through
// (x = +-inf gives +-inf, as the division does); below that range the last bits may differ from the division's and +-0 loses its sign.
MP_HD double mp_div_hoisted_core(double x, double d, double r) {
    const double q0 = x * r;
    const double q1 = fma(fma(-q0, d, x), r, q0);
    const double q2 = fma(fma(-q1, d, x), r, q1);
    return (fabs(q0) <= 1.7976931348623157e308) ? q2 : q0;
}
// ... and with the division itself outside the exact range: RN(x / d) for every x
MP_HD double mp_div_hoisted(double x, double d, double r) {
    const double ax = fabs(x);
    if (!(ax > 0x1p-900 && ax < 0x1p900)) return x / d;
    return mp_div_hoisted_core(x, d, r);
}
// whether a divisor may be hoisted: finite, well inside the exponent range, significand not all ones
MP_HD bool mp_rcp_hoistable(double d) {
    const uint64_t u = mp_f2u(fabs(d));
    return fabs(d) > 0x1p-100 && fabs(d) < 0x1p100 && (u & 0x000FFFFFFFFFFFFFull) != 0x000FFFFFFFFFFFFFull;
}
// the hoisted reciprocal, or 0 = "not hoisted" (mp_normal_logpdf_h then divides)
MP_HD double mp_rcp_hoist(double d) { return mp_rcp_hoistable(d) ? 1.0 / d : 0.0; }

// ---------------------------------------------------------------------------------------
// exp
// ---------------------------------------------------------------------------------------
MP_HD double mp_exp(double x) {
    if (x != x) return x;
    if (x > 709.782712893384) return MP_INF;
    if (x < -745.1332191019412) return 0.0;
    const double INV_LN2 = 1.4426950408889634;
    const double LN2_HI = 6.93147180369123816490e-01;  // 0x3FE62E42FEE00000
    const double LN2_LO = 1.90821492927058770002e-10;  // 0x3DEA39EF35793C76
    const double kf = rint(mp_mul_c(x, INV_LN2));
    double r = mp_fnma_c(kf, LN2_HI, x);
    r = mp_fnma_c(kf, LN2_LO, r);
    // P(r) = sum_{n=2..13} r^(n-2)/n!
    double p = 1.6059043836821613e-10;   // 1/13!
    p = mp_fma_c(p, r, 2.08767569878681e-09); // 1/12!
    p = mp_fma_c(p, r, 2.505210838544172e-08);   // 1/11!
    p = mp_fma_c(p, r, 2.755731922398589e-07);   // 1/10!
    p = mp_fma_c(p, r, 2.7557319223985893e-06);  // 1/9!
    p = mp_fma_c(p, r, 2.48015873015873e-05);    // 1/8!
    p = mp_fma_c(p, r, 1.984126984126984e-04);   // 1/7!
    p = mp_fma_c(p, r, 1.388888888888889e-03);   // 1/6!
    p = mp_fma_c(p, r, 8.333333333333333e-03);   // 1/5!
    p = mp_fma_c(p, r, 4.1666666666666664e-02);  // 1/4!
    p = mp_fma_c(p, r, 1.6666666666666666e-01);  // 1/3!
    p = fma(p, r, 0.5);
    const double y = 1.0 + fma(r * r, p, r);  // in [0.70, 1.42]
    const int k = (int)kf;
    if (k > 1023) {
        return y * mp_u2f((uint64_t)(k - 1 + 1023) << 52) * 2.0;
    }
    if (k < -1022) {
        // k >= -1075: y * 2^(k+54) is normal and exact, the last multiply rounds once.
        return y * mp_u2f((uint64_t)(k + 54 + 1023) << 52) * 5.551115123125783e-17;  // 2^-54
    }
    return y * mp_u2f((uint64_t)(k + 1023) << 52);
}

// ---------------------------------------------------------------------------------------
// log
// ---------------------------------------------------------------------------------------
// SC: the constants as scalar operands (mp_add_c / mp_mul_c above) or left to the compiler; mp_log(x) = mp_log_<false>(x)
template <bool SC> MP_HD double mp_log_(double x) {
    const double LN2_HI = 6.93147180369123816490e-01;
    const double LN2_LO = 1.90821492927058770002e-10;
    const double Lg1 = 6.666666666666735130e-01, Lg2 = 3.999999999940941908e-01,
                 Lg3 = 2.857142874366239149e-01, Lg4 = 2.222219843214978396e-01,
                 Lg5 = 1.818357216161805012e-01, Lg6 = 1.531383769920937332e-01,
                 Lg7 = 1.479819860511658591e-01;
    uint64_t u = mp_f2u(x);
    uint32_t hx = (uint32_t)(u >> 32);
    int k = 0;
    if (hx < 0x00100000u || (hx >> 31)) {
        if ((u << 1) == 0) return MP_NEG_INF;        // log(+-0) = -inf
        if (hx >> 31) return mp_u2f(0x7FF8000000000000ull);  // log(x<0) = NaN
        k -= 54;                                     // subnormal: scale up
        x *= 18014398509481984.0;                    // 2^54
        u = mp_f2u(x);
        hx = (uint32_t)(u >> 32);
    } else if (hx >= 0x7FF00000u) {
        return x;                                    // inf or NaN
    } else if (u == 0x3FF0000000000000ull) {
        return 0.0;
    }
    // x = 2^k * m, m in [sqrt(2)/2, sqrt(2))
    hx += 0x3FF00000u - 0x3FE6A09Eu;
    k += (int)(hx >> 20) - 0x3FF;
    hx = (hx & 0x000FFFFFu) + 0x3FE6A09Eu;
    u = ((uint64_t)hx << 32) | (u & 0xFFFFFFFFull);
    const double m = mp_u2f(u);
    const double f = m - 1.0;
    const double hfsq = 0.5 * f * f;
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double w = z * z;
    const double t1 = w * mp_add_cs<SC>(w * mp_add_cs<SC>(mp_mul_cs<SC>(w, Lg6), Lg4), Lg2);                         // w (Lg2 + w (Lg4 + w Lg6))
    const double t2 = z * mp_add_cs<SC>(w * mp_add_cs<SC>(w * mp_add_cs<SC>(mp_mul_cs<SC>(w, Lg7), Lg5), Lg3), Lg1);  // z (Lg1 + w (Lg3 + w (Lg5 + w Lg7)))
    const double R = t2 + t1;
    const double dk = (double)k;
    return s * (hfsq + R) + mp_mul_cs<SC>(dk, LN2_LO) - hfsq + f + mp_mul_cs<SC>(dk, LN2_HI);
}
MP_HD double mp_log(double x) { return mp_log_<false>(x); }

// sqrt and division are IEEE-754 correctly rounded for fp64 both in SSE2 and in the gfx950
// expansion hipcc emits without fast-math (checked bit-for-bit in tests/test_gpu_math.py).
MP_HD double mp_sqrt(double x) { return sqrt(x); }

// ---------------------------------------------------------------------------------------
// sin / cos / atan2 — same contract as mp_exp/mp_log: one definition, IEEE ops only, evaluated
// identically on host and device.  Classical fdlibm schemes (k_sin.c, k_cos.c, e_rem_pio2.c medium
// case, s_atan.c, e_atan2.c; Sun Microsystems notice above applies), constants as published.
// Domain of the argument reduction: |x| < 2^20 * pi/2 (~1.6e6); beyond that NaN is returned (the
// models on the path keep angles within a few turns).
// ---------------------------------------------------------------------------------------
MP_HD double mp_ksin(double x, double y) {  // |x| <= pi/4, y = tail
    const double S1 = -1.66666666666666324348e-01, S2 = 8.33333333332248946124e-03, S3 = -1.98412698298579493134e-04,
                 S4 = 2.75573137070700676789e-06, S5 = -2.50507602534068634195e-08, S6 = 1.58969099521155010221e-10;
    const double z = x * x;
    const double w = z * z;
    const double r = S2 + z * (S3 + z * S4) + z * w * (S5 + z * S6);
    const double v = z * x;
    return x - ((z * (0.5 * y - v * r) - y) - v * S1);
}
MP_HD double mp_kcos(double x, double y) {
    const double C1 = 4.16666666666666019037e-02, C2 = -1.38888888888741095749e-03, C3 = 2.48015872894767294178e-05,
                 C4 = -2.75573143513906633035e-07, C5 = 2.08757232129817482790e-09, C6 = -1.13596475577881948265e-11;
    const double z = x * x;
    const double w = z * z;
    const double r = z * (C1 + z * (C2 + z * C3)) + w * w * (C4 + z * (C5 + z * C6));
    const double hz = 0.5 * z;
    const double ww = 1.0 - hz;
    return ww + (((1.0 - ww) - hz) + (z * r - x * y));
}
// x = n*(pi/2) + (y0 + y1), |y0| <= pi/4 (+tiny); returns n mod 4 (non-negative), or -1 out of domain
MP_HD int mp_rem_pio2(double x, double* y0, double* y1) {
    const double INVPIO2 = 6.36619772367581382433e-01;
    const double P1 = 1.57079632673412561417e+00;   // first 33 bits of pi/2
    const double P1T = 6.07710050650619224932e-11;  // pi/2 - P1
    const double P2 = 6.07710050630396597660e-11;   // second 33 bits
    const double P2T = 2.02226624879595063154e-21;  // pi/2 - (P1 + P2)
    const double P3 = 2.02226624871116645580e-21;   // third 33 bits
    const double P3T = 8.47842766036889956997e-32;  // pi/2 - (P1 + P2 + P3)
    if (!(fabs(x) < 1647099.0)) return -1;           // also catches NaN / inf
    const double fn = rint(x * INVPIO2);
    double r = x - fn * P1;                          // exact: fn < 2^21, P1 has 33 bits
    double w = fn * P1T;
    double y = r - w;
    // second iteration when cancellation ate too many bits (difference of exponents > 16)
    const int ex = (int)((mp_f2u(x) >> 52) & 0x7FF);
    const int ey = (int)((mp_f2u(y) >> 52) & 0x7FF);
    if (ex - ey > 16) {
        double t = r;
        w = fn * P2;
        r = t - w;
        w = fn * P2T - ((t - r) - w);
        y = r - w;
        // third when even that left fewer than 4 significant bits of the tail (difference > 49): x within ~2^-50 |x| of a multiple
        // of pi/2 (413441.44719405076, n = 263205, cancels 70 bits; two iterations err by 1.06 ulp there)
        if (ex - (int)((mp_f2u(y) >> 52) & 0x7FF) > 49) {
            t = r;
            w = fn * P3;
            r = t - w;
            w = fn * P3T - ((t - r) - w);
            y = r - w;
        }
    }
    *y0 = y;
    *y1 = (r - y) - w;
    const long long n = (long long)fn;
    return (int)(n & 3);
}
MP_HD double mp_sin(double x) {
    if (fabs(x) <= 0.78539816339744828) return mp_ksin(x, 0.);
    double y0, y1;
    const int n = mp_rem_pio2(x, &y0, &y1);
    if (n < 0) return mp_u2f(0x7FF8000000000000ull);
    switch (n) {
    case 0: return mp_ksin(y0, y1);
    case 1: return mp_kcos(y0, y1);
    case 2: return -mp_ksin(y0, y1);
    default: return -mp_kcos(y0, y1);
    }
}
MP_HD double mp_cos(double x) {
    if (fabs(x) <= 0.78539816339744828) return mp_kcos(x, 0.);
    double y0, y1;
    const int n = mp_rem_pio2(x, &y0, &y1);
    if (n < 0) return mp_u2f(0x7FF8000000000000ull);
    switch (n) {
    case 0: return mp_kcos(y0, y1);
    case 1: return -mp_ksin(y0, y1);
    case 2: return -mp_kcos(y0, y1);
    default: return mp_ksin(y0, y1);
    }
}

MP_HD double mp_atan(double x) {
    const double atanhi[4] = {4.63647609000806093515e-01, 7.85398163397448278999e-01, 9.82793723247329054082e-01, 1.57079632679489655800e+00};
    const double atanlo[4] = {2.26987774529616870924e-17, 3.06161699786838301793e-17, 1.39033110312309984516e-17, 6.12323399573676603587e-17};
    const double aT[11] = {3.33333333333329318027e-01,  -1.99999999998764832476e-01, 1.42857142725034663711e-01,  -1.11111104054623557880e-01,
                           9.09088713343650656196e-02,  -7.69187620504482999495e-02, 6.66107313738753120669e-02,  -5.83357013379057348645e-02,
                           4.97687799461593236017e-02,  -3.65315727442169155270e-02, 1.62858201153657823623e-02};
    if (x != x) return x;
    const bool neg = (mp_f2u(x) >> 63) != 0;
    double ax = fabs(x);
    int id;
    if (ax >= 7.3786976294838206e19) {  // 2^66
        const double r = atanhi[3] + 7.52316384526264005100e-37;
        return neg ? -r : r;
    }
    if (ax < 0.4375) {
        if (ax < 3.7252902984619141e-09) return x;  // 2^-28
        id = -1;
    } else if (ax < 1.1875) {
        if (ax < 0.6875) { id = 0; ax = (2.0 * ax - 1.0) / (2.0 + ax); }
        else { id = 1; ax = (ax - 1.0) / (ax + 1.0); }
    } else {
        if (ax < 2.4375) { id = 2; ax = (ax - 1.5) / (1.0 + 1.5 * ax); }
        else { id = 3; ax = -1.0 / ax; }
    }
    const double z = ax * ax;
    const double w = z * z;
    const double s1 = z * (aT[0] + w * (aT[2] + w * (aT[4] + w * (aT[6] + w * (aT[8] + w * aT[10])))));
    const double s2 = w * (aT[1] + w * (aT[3] + w * (aT[5] + w * (aT[7] + w * aT[9]))));
    if (id < 0) {
        const double r = ax - ax * (s1 + s2);
        return neg ? -r : r;
    }
    const double r = atanhi[id] - ((ax * (s1 + s2) - atanlo[id]) - ax);
    return neg ? -r : r;
}
// atan2(y, x) with the usual IEEE special cases (f64::atan2 semantics)
MP_HD double mp_atan2(double y, double x) {
    const double PI = 3.1415926535897931160E+00, PI_LO = 1.2246467991473531772E-16;
    if (x != x || y != y) return x + y;
    const uint64_t ux = mp_f2u(x), uy = mp_f2u(y);
    const bool xneg = (ux >> 63) != 0, yneg = (uy >> 63) != 0;
    const double ax = fabs(x), ay = fabs(y);
    if (ux == 0x3FF0000000000000ull) return mp_atan(y);  // x == 1
    if (ay == 0.) return xneg ? (yneg ? -PI : PI) : y;   // y = +-0
    if (ax == 0.) return yneg ? -PI / 2 : PI / 2;
    if (ax == MP_INF) {
        if (ay == MP_INF) { const double r = xneg ? 3.0 * (PI / 4) : PI / 4; return yneg ? -r : r; }
        const double r = xneg ? PI : 0.0;
        return yneg ? -r : r;
    }
    if (ay == MP_INF) return yneg ? -PI / 2 : PI / 2;
    const int ex = (int)((ux >> 52) & 0x7FF), ey = (int)((uy >> 52) & 0x7FF);
    if (ey - ex > 60) {                                   // |y/x| > 2^60: +-pi/2 whatever the sign of x (e_atan2.c's m &= 1)
        const double r = PI / 2 + 0.5 * PI_LO;
        return yneg ? -r : r;
    }
    double z;
    if (xneg && (ex - ey) > 60) z = 0.0;                  // |y/x| < 2^-60, x < 0
    else z = mp_atan(fabs(y / x));
    if (!xneg) return yneg ? -z : z;
    const double r = PI - (z - PI_LO);
    return yneg ? -r : r;
}

// ---------------------------------------------------------------------------------------
// log1p / lgamma — same contract: one definition, IEEE ops only (+ - * / and integer bit work) plus mp_log, identical on host and
// device.  The classical fdlibm schemes (s_log1p.c; e_lgamma_r.c for x > 0 only, so no sin and no reflection; Sun Microsystems
// notice above applies), constants as published.  For the log-densities of mp_dists.h (poisson, gamma, beta, geometric).
// ---------------------------------------------------------------------------------------
// log(1 + x): x = -1 gives -inf, x < -1 NaN, +inf and NaN pass through
MP_HD double mp_log1p(double x) {
    const double LN2_HI = 6.93147180369123816490e-01, LN2_LO = 1.90821492927058770002e-10;
    const double Lp1 = 6.666666666666735130e-01, Lp2 = 3.999999999940941908e-01, Lp3 = 2.857142874366239149e-01,
                 Lp4 = 2.222219843214978396e-01, Lp5 = 1.818357216161805012e-01, Lp6 = 1.531383769920937332e-01,
                 Lp7 = 1.479819860511658591e-01;
    const uint64_t ux = mp_f2u(x);
    const int32_t hx = (int32_t)(uint32_t)(ux >> 32);
    const int32_t ax = hx & 0x7fffffff;
    int k = 1, hu = 0;
    double f = 0., c = 0.;
    if (hx < 0x3FDA827A) {                            // x < 0.41422
        if (ax >= 0x3ff00000) {                       // x <= -1
            if (x == -1.0) return MP_NEG_INF;
            return mp_u2f(0x7FF8000000000000ull);
        }
        if (ax < 0x3e200000) {                        // |x| < 2^-29
            if (ax < 0x3c900000) return x;            // |x| < 2^-54
            return x - x * x * 0.5;
        }
        if (hx > 0 || hx <= (int32_t)0xbfd2bec3u) {   // -0.2929 < x < 0.41422
            k = 0; f = x; hu = 1;
        }
    }
    if (hx >= 0x7ff00000) return x + x;               // +inf, NaN
    if (k != 0) {
        double u;
        if (hx < 0x43400000) {
            u = 1.0 + x;
            hu = (int)(mp_f2u(u) >> 32);
            k = (hu >> 20) - 1023;
            c = (k > 0) ? 1.0 - (u - x) : x - (u - 1.0);   // the rounding error of 1 + x
            c /= u;
        } else {
            u = x;
            hu = (int)(mp_f2u(u) >> 32);
            k = (hu >> 20) - 1023;
            c = 0.;
        }
        hu &= 0x000fffff;
        const uint64_t lo = mp_f2u(u) & 0xFFFFFFFFull;
        if (hu < 0x6a09e) {
            u = mp_u2f(((uint64_t)(uint32_t)(hu | 0x3ff00000) << 32) | lo);   // u in [1, sqrt 2)
        } else {
            k += 1;
            u = mp_u2f(((uint64_t)(uint32_t)(hu | 0x3fe00000) << 32) | lo);   // u / 2 in [sqrt 2 / 2, 1)
            hu = (0x00100000 - hu) >> 2;
        }
        f = u - 1.0;
    }
    const double hfsq = 0.5 * f * f;
    const double dk = (double)k;
    if (hu == 0) {                                    // |f| < 2^-20
        if (f == 0.) {
            if (k == 0) return 0.;
            c += dk * LN2_LO;
            return dk * LN2_HI + c;
        }
        const double R = hfsq * (1.0 - 0.66666666666666666 * f);
        if (k == 0) return f - R;
        return dk * LN2_HI - ((R - (dk * LN2_LO + c)) - f);
    }
    const double s = f / (2.0 + f);
    const double z = s * s;
    const double R = z * (Lp1 + z * (Lp2 + z * (Lp3 + z * (Lp4 + z * (Lp5 + z * (Lp6 + z * Lp7))))));
    if (k == 0) return f - (hfsq - s * (hfsq + R));
    return dk * LN2_HI - ((hfsq - (s * (hfsq + R) + (dk * LN2_LO + c))) - f);
}

// ln Gamma(x) for x > 0 (x <= 0 and NaN give NaN, +inf gives +inf).  mp_lgamma(1) = mp_lgamma(2) = 0 exactly.
//   x < 2^-70: -log x;  x < 2: one of three expansions around the minimum tc = 1.4616.. or the zeros 1, 2 (x < 0.9 through
//   lgamma(x + 1) - log x);  x < 8: the rational form on [2, 3) and log of the product of the shifts;  x < 2^58: Stirling's
//   series;  beyond: x (log x - 1).
MP_HD double mp_lgamma(double x) {
    const double a0 = 7.72156649015328655494e-02, a1 = 3.22467033424113591611e-01, a2 = 6.73523010531292681824e-02,
                 a3 = 2.05808084325167332806e-02, a4 = 7.38555086081402883957e-03, a5 = 2.89051383673415629091e-03,
                 a6 = 1.19270763183362067845e-03, a7 = 5.10069792153511336608e-04, a8 = 2.20862790713908385557e-04,
                 a9 = 1.08011567247583939954e-04, a10 = 2.52144565451257326939e-05, a11 = 4.48640949618915160150e-05;
    const double tc = 1.46163214496836224576e+00, tf = -1.21486290535849611461e-01, tt = -3.63867699703950536541e-18;
    const double t0 = 4.83836122723810047042e-01, t1 = -1.47587722994593911752e-01, t2 = 6.46249402391333854778e-02,
                 t3 = -3.27885410759859649565e-02, t4 = 1.79706750811820387126e-02, t5 = -1.03142241298341437450e-02,
                 t6 = 6.10053870246291332635e-03, t7 = -3.68452016781138256760e-03, t8 = 2.25964780900612472250e-03,
                 t9 = -1.40346469989232843813e-03, t10 = 8.81081882437654011382e-04, t11 = -5.38595305356740546715e-04,
                 t12 = 3.15632070903625950361e-04, t13 = -3.12754168375120860518e-04, t14 = 3.35529192635519073543e-04;
    const double u0 = -7.72156649015328655494e-02, u1 = 6.32827064025093366517e-01, u2 = 1.45492250137234768737e+00,
                 u3 = 9.77717527963372745603e-01, u4 = 2.28963728064692451092e-01, u5 = 1.33810918536787660377e-02;
    const double v1 = 2.45597793713041134822e+00, v2 = 2.12848976379893395361e+00, v3 = 7.69285150456672783825e-01,
                 v4 = 1.04222645593369134254e-01, v5 = 3.21709242282423911810e-03;
    const double s0 = -7.72156649015328655494e-02, s1 = 2.14982415960608852501e-01, s2 = 3.25778796408930981787e-01,
                 s3 = 1.46350472652464452805e-01, s4 = 2.66422703033638609560e-02, s5 = 1.84028451407337715652e-03,
                 s6 = 3.19475326584100867617e-05;
    const double r1 = 1.39200533467621045958e+00, r2 = 7.21935547567138069525e-01, r3 = 1.71933865632803078993e-01,
                 r4 = 1.86459191715652901344e-02, r5 = 7.77942496381893596434e-04, r6 = 7.32668430744625636189e-06;
    const double w0 = 4.18938533204672725052e-01, w1 = 8.33333333333329678849e-02, w2 = -2.77777777728775536470e-03,
                 w3 = 7.93650558643019558500e-04, w4 = -5.95187557450339963135e-04, w5 = 8.36339918996282139126e-04,
                 w6 = -1.63092934096575273989e-03;
    if (!(x > 0.)) return mp_u2f(0x7FF8000000000000ull);   // x <= 0, NaN: outside the domain here
    const uint64_t u = mp_f2u(x);
    const uint32_t ix = (uint32_t)(u >> 32), lx = (uint32_t)u;
    if (ix >= 0x7ff00000u) return x;                        // +inf
    if (ix < 0x3b900000u) return -mp_log(x);                // x < 2^-70
    if (((ix - 0x3ff00000u) | lx) == 0u || ((ix - 0x40000000u) | lx) == 0u) return 0.;   // x = 1, 2
    double r;
    if (ix < 0x40000000u) {                                 // x < 2
        double y;
        int i;
        if (ix <= 0x3feccccc) {                             // x < 0.9: lgamma(x) = lgamma(x + 1) - log(x)
            r = -mp_log(x);
            if (ix >= 0x3FE76944u) { y = 1.0 - x; i = 0; }
            else if (ix >= 0x3FCDA661u) { y = x - (tc - 1.0); i = 1; }
            else { y = x; i = 2; }
        } else {
            r = 0.;
            if (ix >= 0x3FFBB4C3u) { y = 2.0 - x; i = 0; }         // [1.7316, 2)
            else if (ix >= 0x3FF3B4C4u) { y = x - tc; i = 1; }     // [1.23, 1.73)
            else { y = x - 1.0; i = 2; }
        }
        if (i == 0) {
            const double z = y * y;
            const double p1 = a0 + z * (a2 + z * (a4 + z * (a6 + z * (a8 + z * a10))));
            const double p2 = z * (a1 + z * (a3 + z * (a5 + z * (a7 + z * (a9 + z * a11)))));
            const double p = y * p1 + p2;
            r += (p - 0.5 * y);
        } else if (i == 1) {
            const double z = y * y;
            const double w = z * y;
            const double p1 = t0 + w * (t3 + w * (t6 + w * (t9 + w * t12)));
            const double p2 = t1 + w * (t4 + w * (t7 + w * (t10 + w * t13)));
            const double p3 = t2 + w * (t5 + w * (t8 + w * (t11 + w * t14)));
            const double p = z * p1 - (tt - w * (p2 + y * p3));
            r += (tf + p);
        } else {
            const double p1 = y * (u0 + y * (u1 + y * (u2 + y * (u3 + y * (u4 + y * u5)))));
            const double p2 = 1.0 + y * (v1 + y * (v2 + y * (v3 + y * (v4 + y * v5))));
            r += (-0.5 * y + p1 / p2);
        }
    } else if (ix < 0x40200000u) {                          // 2 <= x < 8
        const int i = (int)x;
        const double y = x - (double)i;
        const double p = y * (s0 + y * (s1 + y * (s2 + y * (s3 + y * (s4 + y * (s5 + y * s6))))));
        const double q = 1.0 + y * (r1 + y * (r2 + y * (r3 + y * (r4 + y * (r5 + y * r6)))));
        r = 0.5 * y + p / q;
        double z = 1.0;                                     // lgamma(1 + s) = log(s) + lgamma(s)
        if (i >= 7) z *= (y + 6.0);
        if (i >= 6) z *= (y + 5.0);
        if (i >= 5) z *= (y + 4.0);
        if (i >= 4) z *= (y + 3.0);
        if (i >= 3) { z *= (y + 2.0); r += mp_log(z); }
    } else if (ix < 0x43900000u) {                          // 8 <= x < 2^58
        const double t = mp_log(x);
        const double z = 1.0 / x;
        const double y = z * z;
        const double w = w0 + z * (w1 + y * (w2 + y * (w3 + y * (w4 + y * (w5 + y * w6)))));
        r = (x - 0.5) * (t - 1.0) + w;
    } else {
        r = x * (mp_log(x) - 1.0);
    }
    return r;
}
