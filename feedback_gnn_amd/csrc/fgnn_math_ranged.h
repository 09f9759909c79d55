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

/* ---- the selects of fg_phi / fg_softplus as one ordered-value instruction ------------------------------------------------------
 * Both routines end in "x above the softplus threshold ? x : computed value", a v_cmp + v_cndmask pair (and a VCC dependency) on
 * the device.  The computed value is ordered against x and against one constant in a way that lets a median / a maximum pick the
 * same float (tests/test_math_selects.py: exhaustive on the CPU; tests/math_selects_gpu.hip on the device):
 *   phi      : S = fg_log1p(fg_exp(FG_SOFTPLUS_THRESH)) is the float after the threshold.  For xc <= threshold the computed
 *              sp = log1p(exp(xc)) lies in [xc, S]; for xc > threshold (xc >= S) it is never in [S, xc).  med3(sp, xc, S) is therefore
 *              sp below and xc above.  max(sp, xc) alone is NOT enough: on 753 561 floats between 13.9423857 and 14.7666502 the
 *              computed log1p exceeds xc.
 *   softplus : r = exp(t) below -threshold (0 under -87), log1p(exp(min(t, threshold))) otherwise; r >= t wherever the result is r,
 *              and r = S <= t wherever it is t: max(t, r), written as (t < -threshold) ? exp : max(t, log1p).  The two LOW selects
 *              cannot go the same way: log1p(exp t) != exp t on 2 309 063 floats of [-16.2889576, -13.9423857].
 * No NaNs reach either routine and neither ordered value is a zero whose sign could matter. */
#define FG_SOFTPLUS_AT_THRESH 13.9423857f /* fg_log1p(fg_exp(FG_SOFTPLUS_THRESH)), bits 0x415f1403 = FG_SOFTPLUS_THRESH + 1 ulp */

/* median of three: one v_med3_f32 on the device (as FG_CLAMP), the min / max composition on the host */
#if defined(__HIP_DEVICE_COMPILE__)
#define FG_MED3(a, b, c) __builtin_amdgcn_fmed3f((a), (b), (c))
#else
#define FG_MED3(a, b, c) FG_MAX(FG_MIN((a), (b)), FG_MIN(FG_MAX((a), (b)), (c)))
#endif

/* the select of fg_phi on sp = fg_log1p(fg_exp(xc)), xc in [FG_PHI_MIN, FG_PHI_MAX] */
FG_FN float fg_phi_select_med(float sp, float xc) { return FG_MED3(sp, xc, FG_SOFTPLUS_AT_THRESH); }

/* fg_phi(x) for every x: the operations of fg_phi in the same order, the select as a median. */
FG_FN float fg_phi_med(float x)
{
    float xc = FG_CLAMP(x, FG_PHI_MIN, FG_PHI_MAX);
    float y = fg_exp(xc);
    float sp = fg_phi_select_med(fg_log1p(y), xc);
    return sp - fg_log(y - 1.0f);
}

/* fg_softplus(t) for every finite t: the operations of fg_softplus in the same order, the last select as a maximum. */
FG_FN float fg_softplus_max(float t)
{
    float tc = FG_CLAMP(t, -87.0f, FG_SOFTPLUS_THRESH);
    float y = fg_exp(tc);
    float l = fg_log1p(y);
    float small = (t < -87.0f) ? 0.0f : y;
    /* max(t, r) with r = (t < -thr) ? small : l, the maximum taken inside the select: below -thr it is small itself (small >= 0 > t).
     * This way both operands of the maximum are results of float arithmetic; with r as an operand the compiler puts a canonicalising
     * v_max_f32 r, r in front (small carries fg_exp's integer-built bits), which costs what the maximum saves. */
    float m = FG_MAX(t, l);
    return (t < -FG_SOFTPLUS_THRESH) ? small : m;
}

/* ---- arguments bounded by the launch --------------------------------------------------------------------------------------------
 * Two guards of the routines above exist for arguments the launch of a BP4 decoder can prove never occur (plan_bp4 in fgnn_bp4.hip
 * makes the proof from the launch arguments; a decode it cannot prove takes the routines above):
 *   log-sum-exp : min(d, 20) keeps fg_exp inside its domain, which ends at -87.  For 20 < d <= 87 the exponential is evaluated at -d
 *                 instead of -20 and y = fg_exp(-d) <= fg_exp(-20) = 2.06e-9 < 2^-24 either way: 1 + y == 1.0f, and the log of 1.0f is
 *                 +0.  Below 20 the minimum is d itself.
 *   softplus    : the lower bound of the clamp and the select on t < -87 act below -87 only.
 * With |t| and d at most FG_BOUNDED_MAX the guarded and the bounded forms return the same bits (tests/test_math_bounded.py:
 * exhaustive over the range).  The distance from 80 to the domain's edge at 87 is deliberate: the proof of the launch is made in exact
 * arithmetic and the float sums it speaks of round. */
#define FG_BOUNDED_MAX 80.0f

/* fg_softplus_max(t) for |t| <= FG_BOUNDED_MAX: the same operations in the same order, the clamp's upper bound alone, no flush */
FG_FN float fg_softplus_bounded(float t)
{
    float tc = FG_MIN(t, FG_SOFTPLUS_THRESH);
    float y = fg_exp(tc);
    float l = fg_log1p(y);
    float m = FG_MAX(t, l);
    return (t < -FG_SOFTPLUS_THRESH) ? y : m;
}

/* fg_lse2_corr_ranged / fg_lse2_ranged for |a - b| <= FG_BOUNDED_MAX: the exponential at -d itself */
FG_FN float fg_lse2_corr_bounded(float a, float b)
{
    float d = FG_ABS(a - b);
    float y = fg_exp(-d);
    return fg_log_1to2(1.0f + y);
}
FG_FN float fg_lse2_bounded(float a, float b)
{
    float m = FG_MAX(a, b);
    return fg_lse2_corr_bounded(a, b) + m;
}

#endif /* FGNN_MATH_RANGED_H */
