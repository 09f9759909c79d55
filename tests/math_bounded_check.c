/* Bit comparison of the bounded routines of feedback_gnn_amd/csrc/fgnn_math_ranged.h (fg_lse2_corr_bounded, fg_lse2_bounded,
 * fg_softplus_bounded: the range guards dropped) with the guarded ones they stand for, and the message bound the launch's proof
 * rests on (host code, no GPU; built and run by tests/test_math_bounded.py with the oracle's compiler flags plus -fopenmp).
 *   1. fg_lse2_corr_bounded == fg_lse2_corr_ranged and fg_lse2_bounded == fg_lse2_ranged for EVERY float d of [0, FG_BOUNDED_MAX],
 *      the first pair called with (a, b) = (d, 0) and (0, d), the second with (-d, 0) and (0, -d), the signs the qubit update passes.
 *   2. fg_softplus_bounded == fg_softplus_max for EVERY float t of [-FG_BOUNDED_MAX, FG_BOUNDED_MAX].
 *   3. Both again on the slack the launch leaves, (FG_BOUNDED_MAX, 87]: the guards act beyond 87 only.
 *   4. fg_phi_med(x) <= 16.6355324f for EVERY float of the clip range, for 0 of both signs and for values above the clip.
 * Prints one line per part and exits 1 at the first differing bit pattern. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "fgnn_math_ranged.h"

static int same(float a, float b) { return fg_f2u(a) == fg_f2u(b); }

static int lse_ok(float d)
{
    return same(fg_lse2_corr_bounded(d, 0.0f), fg_lse2_corr_ranged(d, 0.0f)) && same(fg_lse2_corr_bounded(0.0f, d), fg_lse2_corr_ranged(0.0f, d)) &&
           same(fg_lse2_bounded(-d, 0.0f), fg_lse2_ranged(-d, 0.0f)) && same(fg_lse2_bounded(0.0f, -d), fg_lse2_ranged(0.0f, -d));
}
static int softplus_ok(float t) { return same(fg_softplus_bounded(t), fg_softplus_max(t)); }
static int phi_ok(float x) { return fg_phi_med(x) <= 16.6355324f; }

/* first bit pattern of [lo, hi] at which `ok` fails, or -1; *n += the number of values walked */
static long long sweep(int (*ok)(float), uint32_t lo, uint32_t hi, unsigned long long* n)
{
    long long first = -1;
    unsigned long long cnt = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : cnt)
    for (long long c = lo >> 16; c <= (long long)(hi >> 16); ++c) {
        const uint64_t a = (uint64_t)c << 16, b = a + 0xffffu;
        for (uint64_t u = a < lo ? lo : a; u <= (b > hi ? hi : b); ++u) {
            ++cnt;
            if (!ok(fg_u2f((uint32_t)u))) {
#pragma omp critical
                if (first < 0 || (long long)u < first) first = (long long)u;
            }
        }
    }
    *n += cnt;
    return first;
}

static int report(const char* what, long long first)
{
    if (first < 0) return 0;
    printf("%s mismatch at bits 0x%08x (%a)\n", what, (unsigned)first, fg_u2f((uint32_t)first));
    return 1;
}

int main(void)
{
    const uint32_t top = fg_f2u(FG_BOUNDED_MAX), edge = fg_f2u(87.0f), neg = 0x80000000u;
    unsigned long long n;
    long long f;

    /* 1. log-sum-exp: every d of [0, FG_BOUNDED_MAX] */
    n = 0;
    f = sweep(lse_ok, 0u, top, &n);
    if (report("lse2", f)) return 1;
    printf("lse2 [0, %g]: %llu values, 0 mismatches\n", (double)FG_BOUNDED_MAX, n);

    /* 2. softplus: every t of [-FG_BOUNDED_MAX, FG_BOUNDED_MAX] */
    n = 0;
    f = sweep(softplus_ok, 0u, top, &n);
    if (f < 0) f = sweep(softplus_ok, neg, neg | top, &n);
    if (report("softplus", f)) return 1;
    printf("softplus [-%g, %g]: %llu values, 0 mismatches\n", (double)FG_BOUNDED_MAX, (double)FG_BOUNDED_MAX, n);

    /* 3. the slack up to the domain's edge */
    n = 0;
    f = sweep(lse_ok, top, edge, &n);
    if (report("lse2 (slack)", f)) return 1;
    f = sweep(softplus_ok, top, edge, &n);
    if (f < 0) f = sweep(softplus_ok, neg | top, neg | edge, &n);
    if (report("softplus (slack)", f)) return 1;
    printf("slack (%g, 87]: %llu values, 0 mismatches\n", (double)FG_BOUNDED_MAX, n);
    /* and the guards do act beyond it: the bounded softplus is NOT the guarded one at -88 (this is what a wrongly picked kernel shows) */
    if (softplus_ok(-88.0f)) {
        printf("softplus: the bounded form equals the guarded one at -88: the guard is dead and this file checks nothing\n");
        return 1;
    }

    /* 4. the message bound: phi never exceeds phi0 */
    n = 0;
    f = sweep(phi_ok, fg_f2u(FG_PHI_MIN), fg_f2u(FG_PHI_MAX), &n);
    if (report("phi bound", f)) return 1;
    printf("phi <= phi0 on the clip range: %llu values, 0 violations\n", n);
    const float pts[] = {0.0f, -0.0f, 1e-45f, 1e-30f, 8.49999999e-8f, 16.6355343f, 17.0f, 20.0f, 87.0f, 100.0f, 1e10f, 1e30f, 3.40282347e38f};
    for (unsigned i = 0; i < sizeof(pts) / sizeof(pts[0]); ++i)
        if (!phi_ok(pts[i])) {
            printf("phi bound violated at %a: %a\n", pts[i], fg_phi_med(pts[i]));
            return 1;
        }
    if (!same(fg_phi_med(0.0f), 16.6355324f)) {
        printf("phi(0) = %a is not phi0\n", fg_phi_med(0.0f));
        return 1;
    }
    printf("phi <= phi0 outside the clip range: %u points, 0 violations; phi(0) = phi0 = %.9g\n", (unsigned)(sizeof(pts) / sizeof(pts[0])),
           fg_phi_med(0.0f));
    return 0;
}
