/* fgnn_math_ranged.h — routines of fgnn_math.h specialised to an argument range the caller guarantees.
 *
 * Same rules as fgnn_math.h (binary32 fma / add / mul, comparisons, 32-bit integer operations; compiled by hipcc for the kernels and by
 * gcc for the CPU tests), and every routine here returns the BITS of the fgnn_math.h routine it stands for on its whole range
 * (tests/test_math_ranged.py: exhaustive).  fgnn_math.h itself is what the CPU oracle compiles and does not change.
 *
 * What the range buys: fg_log turns the masked exponent word eb = e << 23 into a float with v_cvt_f32_i32, a half-rate instruction on
 * gfx950.  For x in [1, 2] the word is one of two values, 0 (x < 1.421875: e = 0) or 0x00800000 (e = 1), and reinterpreted as a float
 * that is +0 or 2^-126, the smallest normal number: no conversion.  With K = RN(ln 2) * 2^126 in place of FG_LN2_S23 = RN(ln 2) * 2^-23
 * the product inside the fma is exactly 0 or RN(ln 2) either way, so fma(fg_u2f(eb), K, s) == fma((float)(int32_t)eb, FG_LN2_S23, s).
 */
#ifndef FGNN_MATH_RANGED_H
#define FGNN_MATH_RANGED_H

#include "fgnn_math.h"

#define FG_LN2_S126 0x1.62e43p+125f      /* RN(ln 2) * 2^126 = 5.8966e37 (bits 0x7e317218): the exponent arrives as e * 2^-126 */

/* fg_log(x) for x in [1, 2]: the operations of fg_log in the same order, the exponent term without the int -> float conversion. */
FG_FN float fg_log_1to2(float x)
{
    const float* tab = fg_log_tab();
    const uint32_t b = fg_f2u(x);
    const uint32_t w = b - FG_LOG_OFFS;
    const uint32_t eb = w & 0xff800000u;              /* 0 or 0x00800000 */
    const float mm = fg_u2f(b - eb);
    const uint32_t j = (w >> 18) & 31u;
    const float rc = tab[j], lc = tab[32 + j];
    const float r = FG_FMA(mm, rc, -1.0f);
    return FG_FMA(fg_u2f(eb), FG_LN2_S126, lc + fg_log1p_small(r));
}

/* fg_lse2_corr / fg_lse2 of fgnn_math.h: y = exp(-min(|a - b|, 20)) is in (0, 1], so the log's argument 1 + y is in [1, 2]. */
FG_FN float fg_lse2_corr_ranged(float a, float b)
{
    float d = FG_ABS(a - b);
    float y = fg_exp(-FG_MIN(d, 20.0f));
    return fg_log_1to2(1.0f + y);
}
FG_FN float fg_lse2_ranged(float a, float b)
{
    float m = FG_MAX(a, b);
    return fg_lse2_corr_ranged(a, b) + m;
}

#endif /* FGNN_MATH_RANGED_H */
