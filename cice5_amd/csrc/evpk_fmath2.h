/* evpk_fmath2.h -- log, atan and pow as FIXED algorithms in IEEE double arithmetic, on the footing of evpk_fmath.h and dev_exp: + - x /,
 * explicit fma() only where it is written out, no contraction by the compiler (-ffp-contract=off), no libm call beyond fma / floor /
 * ldexp, exponents handled with integer operations.  The HIP kernels of step_therm1 (csrc/evpk_therm1s.hip: atmo_boundary_layer takes
 * log and atan, frzmlt_bottom_lateral raises deltaT to the real power m2 = 1.36) and their CPU checker (tests/npfmath2.py, the same
 * operations in the same order) produce the same bits.  A header of its own: evpk_fmath.h is part of the oracle's build and stays as it is.
 *
 *   evpk_exp(x)         dev_exp (csrc/evpk_kernels.hip), operation for operation, so that the host can compile evpk_pow_pos: Cody-Waite
 *                       reduction and the degree-5 minimax in r^2 of fdlibm's e_exp.c.  Constants: fdlibm e_exp.c (ln2HI, ln2LO, invln2,
 *                       P1 .. P5), the literals dev_exp carries.
 *   evpk_log_hl(x, &lo) log x as hi + lo for x > 0 finite and normal.  fdlibm e_log's reduction x = 2^k m, sqrt(1/2) <= m < sqrt(2), by
 *                       integer operations on the high word (the offset 0x95f64 is fdlibm's); f = m - 1 (exact), s = f / (2 + f) carried
 *                       as s_hi + s_lo (the division's residual through one fma), log m = 2 s + s z P(z), z = s_hi^2, P the series
 *                       2/3 + 2 z/5 + ... + 2 z^9/21 of 2 atanh(s) (the next term is below 2^-60 of 2 s).  k ln2_hi is exact (ln2_hi
 *                       carries 32 bits), k ln2_hi + 2 s_hi is summed with its exact error, everything small goes to lo.
 *                       Constants (scripts/gen_fmath.py, exact rational arithmetic): ln 2 = 2 atanh(1/3) truncated to 32 bits and the
 *                       correctly rounded remainder; EVPK_LG[k] = 2 / (2 k + 3) correctly rounded.
 *   evpk_log(x)         the hi part.  Against glibc log over [2^-40, 2^40]: at most 1 ulp (tests/test_fmath2_host.py holds it to 2).
 *   evpk_atan(x)        IS evpk_atan2(x, 1.0) of evpk_fmath.h: its table atan(k/16) and its series, no code of its own.  For x > 1 that is
 *                       pi/2 - atan(1/x).  Against glibc atan over [0, 64]: at most 1 ulp (held to 2).
 *   evpk_pow_pos(x, y)  x^y for x >= 0 (0 or normal), y > 0; x = 0 gives 0 by a select.  NOT exp(y log x): with p = y * hi and
 *                       e = fma(y, hi, -p) its exact error, x^y = E + E * (e + y * lo), E = evpk_exp(p) -- the low part is applied after
 *                       the exp.  Against glibc pow over x in [2^-40, 64], y = 1.36 (400 000 arguments): at most 1 ulp measured, asserted
 *                       as 1 (tests/test_fmath2_host.py); the plain exp(y log x) with libm's own exp and log is up to 52 ulp away there.
 * Accuracy is measured on the CPU against glibc, never against the device.
 */
#ifndef EVPK_FMATH2_H
#define EVPK_FMATH2_H
#include "evpk_fmath.h"

/* ln 2 = HI + LO: HI = ln 2 truncated to 32 significant bits (k * HI exact for |k| < 2^21), LO the correctly rounded rest */
#define EVPK_LN2_HI 0.6931471803691238
#define EVPK_LN2_LO 1.9082149292705877e-10

/* dev_exp, operation for operation */
EVPK_HD double evpk_exp(double x) {
    const double ln2HI = 6.93147180369123816490e-01, ln2LO = 1.90821492927058770002e-10, invln2 = 1.44269504088896338700e+00;
    const double P1 = 1.66666666666666019037e-01, P2 = -2.77777777770155933842e-03, P3 = 6.61375632143793436117e-05,
                 P4 = -1.65339022054652515390e-06, P5 = 4.13813679705723846039e-08;
    const double ax = fabs(x);
    double hi = 0.0, lo = 0.0;
    int k = 0;
    if (ax > 0.34657359027997264) {
        if (ax < 1.0397207708399179) {
            k = x < 0.0 ? -1 : 1;
            hi = x - (double)k * ln2HI;
            lo = (double)k * ln2LO;
        } else {
            k = (int)(invln2 * x + (x < 0.0 ? -0.5 : 0.5));
            const double t = (double)k;
            hi = x - t * ln2HI;
            lo = t * ln2LO;
        }
        x = hi - lo;
    } else if (ax < 3.725290298461914e-09) {
        return 1.0 + x;
    }
    const double t = x * x;
    const double c = x - t * (P1 + t * (P2 + t * (P3 + t * (P4 + t * P5))));
    if (k == 0) return 1.0 - ((x * c) / (c - 2.0) - x);
    const double y = 1.0 - ((lo - (x * c) / (2.0 - c)) - hi);
    return ldexp(y, k);
}

/* log x = hi + lo, x > 0 finite and normal; |lo| <= ulp(hi) / 2 */
EVPK_HD double evpk_log_hl(double x, double *lo_out) {
    /* 2 atanh(s) = 2 s + s^3 (LG0 + s^2 (LG1 + ...)): LGk = 2 / (2 k + 3) */
    const double LG0 = 0.6666666666666666, LG1 = 0.4, LG2 = 0.2857142857142857, LG3 = 0.2222222222222222, LG4 = 0.18181818181818182,
                 LG5 = 0.15384615384615385, LG6 = 0.13333333333333333, LG7 = 0.11764705882352941, LG8 = 0.10526315789473684,
                 LG9 = 0.09523809523809523;
    long long ix;
    __builtin_memcpy(&ix, &x, 8);
    int hx = (int)(ix >> 32);
    int k = (hx >> 20) - 1023;
    hx &= 0x000fffff;
    const int i = (hx + 0x95f64) & 0x100000;              /* m >= sqrt(2): halve it and count one more power of two */
    ix = ((long long)(hx | (i ^ 0x3ff00000)) << 32) | (ix & 0xffffffffLL);
    k += i >> 20;
    double m;
    __builtin_memcpy(&m, &ix, 8);
    const double f = m - 1.0;                             /* exact */
    const double dh = 2.0 + f, dl = f - (dh - 2.0);       /* 2 + f = dh + dl exactly (|f| < 2) */
    const double sh = f / dh;
    const double r = fma(-sh, dh, f);                     /* the division's residual, exact */
    const double sl = (r - sh * dl) / dh;
    const double z = sh * sh;
    const double P = LG0 + z * (LG1 + z * (LG2 + z * (LG3 + z * (LG4 + z * (LG5 + z * (LG6 + z * (LG7 + z * (LG8 + z * LG9))))))));
    const double fk = (double)k;
    const double a = fk * EVPK_LN2_HI, b = 2.0 * sh;      /* both exact */
    const double h0 = a + b, bb = h0 - a;
    const double e = (a - (h0 - bb)) + (b - bb);          /* a + b = h0 + e exactly */
    const double l = e + (fk * EVPK_LN2_LO + (2.0 * sl + (sh * z) * P));
    const double H = h0 + l;
    *lo_out = l - (H - h0);
    return H;
}

EVPK_HD double evpk_log(double x) {
    double lo;
    return evpk_log_hl(x, &lo);
}

/* atan x, x finite: evpk_atan2(x, 1) */
EVPK_HD double evpk_atan(double x) { return evpk_atan2(x, 1.0); }

/* x^y, x = 0 or x > 0 normal, y > 0 (results that neither overflow nor fall below the normal range) */
EVPK_HD double evpk_pow_pos(double x, double y) {
    double lo;
    const double hi = evpk_log_hl(x, &lo);
    const double p = y * hi;
    const double e = fma(y, hi, -p);                      /* y * hi = p + e exactly */
    const double t = e + y * lo;
    const double E = evpk_exp(p);
    const double r = E + E * t;
    return x == 0.0 ? 0.0 : r;
}

#endif
