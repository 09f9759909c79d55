/* Bit comparison of fg_phi_med / fg_softplus_max (feedback_gnn_amd/csrc/fgnn_math_ranged.h: the last select of the routine as one
 * median / maximum) with fg_phi / fg_softplus of fgnn_math.h (host code, no GPU; built and run by tests/test_math_selects.py with the
 * oracle's compiler flags plus -fopenmp).
 *   0. FG_SOFTPLUS_AT_THRESH is fg_log1p(fg_exp(FG_SOFTPLUS_THRESH)) and the float after the threshold.
 *   1. fg_phi_med(x) == fg_phi(x) for EVERY float of the clip range [8.5e-8, 16.635532] (231 640 148 values), and for unclamped x on
 *      both sides of it: zeros of both signs, subnormals, one ulp outside either clip point, negatives, magnitudes to 1e30.
 *   2. fg_softplus_max(t) == fg_softplus(t) for EVERY finite float of both signs (4 278 190 080 values).
 * Prints one line per part and exits 1 at the first differing bit pattern. */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

#include "fgnn_math_ranged.h"

static int same(float a, float b) { return fg_f2u(a) == fg_f2u(b); }

/* first bit pattern of [lo, hi] at which the two routines differ, or -1; *n += the number of values walked */
static long long sweep_phi(uint32_t lo, uint32_t hi, unsigned long long* n)
{
    long long first = -1;
    unsigned long long cnt = 0;
#pragma omp parallel for schedule(static) reduction(+ : cnt)
    for (long long c = lo >> 16; c <= (long long)(hi >> 16); ++c) {
        const uint64_t a = (uint64_t)c << 16, b = a + 0xffffu;
        for (uint64_t u = a < lo ? lo : a; u <= (b > hi ? hi : b); ++u) {
            const float x = fg_u2f((uint32_t)u);
            ++cnt;
            if (!same(fg_phi_med(x), fg_phi(x))) {
#pragma omp critical
                if (first < 0 || (long long)u < first) first = (long long)u;
            }
        }
    }
    *n += cnt;
    return first;
}

static long long sweep_softplus(uint32_t lo, uint32_t hi, unsigned long long* n)
{
    long long first = -1;
    unsigned long long cnt = 0;
#pragma omp parallel for schedule(dynamic, 16) reduction(+ : cnt)
    for (long long c = lo >> 16; c <= (long long)(hi >> 16); ++c) {
        const uint64_t a = (uint64_t)c << 16, b = a + 0xffffu;
        for (uint64_t u = a < lo ? lo : a; u <= (b > hi ? hi : b); ++u) {
            const float t = fg_u2f((uint32_t)u);
            ++cnt;
            if (!same(fg_softplus_max(t), fg_softplus(t))) {
#pragma omp critical
                if (first < 0 || (long long)u < first) first = (long long)u;
            }
        }
    }
    *n += cnt;
    return first;
}

static int report(const char* what, long long first, float got, float want)
{
    if (first < 0) return 0;
    printf("%s mismatch at bits 0x%08x (%a): %a vs %a\n", what, (unsigned)first, fg_u2f((uint32_t)first), got, want);
    return 1;
}

int main(void)
{
    /* 0. the constant */
    const float S = fg_log1p(fg_exp(FG_SOFTPLUS_THRESH));
    printf("S = fg_log1p(fg_exp(thr)) = %.9g (bits 0x%08x), FG_SOFTPLUS_AT_THRESH bits 0x%08x, thr bits 0x%08x\n", S, fg_f2u(S),
           fg_f2u(FG_SOFTPLUS_AT_THRESH), fg_f2u(FG_SOFTPLUS_THRESH));
    if (!same(S, FG_SOFTPLUS_AT_THRESH) || fg_f2u(S) != fg_f2u(FG_SOFTPLUS_THRESH) + 1u) {
        printf("constant mismatch\n");
        return 1;
    }

    /* 1. phi: the whole clip range */
    unsigned long long n_phi = 0;
    long long f = sweep_phi(fg_f2u(FG_PHI_MIN), fg_f2u(FG_PHI_MAX), &n_phi);
    if (report("phi", f, f < 0 ? 0.0f : fg_phi_med(fg_u2f((uint32_t)f)), f < 0 ? 0.0f : fg_phi(fg_u2f((uint32_t)f)))) return 1;
    printf("phi clip range: %llu values, 0 mismatches\n", n_phi);

    /* unclamped x on both sides of the clip range */
    unsigned long long n_out = 0;
    const float mags[] = {0.0f, 1e-45f, 1e-40f, 1.17549435e-38f, 1e-30f, 1e-10f, 8.49999999e-8f, 8.5e-8f, 16.635532f, 16.6355343f, 17.0f, 20.0f,
                          87.0f, 88.0f, 100.0f, 1e4f, 1e10f, 1e20f, 1e30f, 0.5f, 1.0f, 13.9423847f, 13.9423857f, 14.2f};
    for (unsigned i = 0; i < sizeof(mags) / sizeof(mags[0]); ++i)
        for (int s = 0; s < 2; ++s) {
            const float x = s ? -mags[i] : mags[i]; /* includes -0 */
            ++n_out;
            if (!same(fg_phi_med(x), fg_phi(x))) {
                printf("phi mismatch at %a: %a vs %a\n", x, fg_phi_med(x), fg_phi(x));
                return 1;
            }
        }
    /* every float one binade below the clip minimum and from the clip maximum to 32, every 4099th negative float */
    unsigned long long n_side = 0;
    f = sweep_phi(fg_f2u(FG_PHI_MIN) - 0x00800000u, fg_f2u(FG_PHI_MIN), &n_side);
    if (f < 0) f = sweep_phi(fg_f2u(FG_PHI_MAX), fg_f2u(32.0f), &n_side);
    if (report("phi", f, f < 0 ? 0.0f : fg_phi_med(fg_u2f((uint32_t)f)), f < 0 ? 0.0f : fg_phi(fg_u2f((uint32_t)f)))) return 1;
    for (uint64_t u = 0x80000000u; u <= 0xff7fffffu; u += 4099u) {
        const float x = fg_u2f((uint32_t)u);
        ++n_side;
        if (!same(fg_phi_med(x), fg_phi(x))) {
            printf("phi mismatch at %a: %a vs %a\n", x, fg_phi_med(x), fg_phi(x));
            return 1;
        }
    }
    for (uint64_t u = 0; u <= 0x7f7fffffu; u += 4099u) {
        const float x = fg_u2f((uint32_t)u);
        ++n_side;
        if (!same(fg_phi_med(x), fg_phi(x))) {
            printf("phi mismatch at %a: %a vs %a\n", x, fg_phi_med(x), fg_phi(x));
            return 1;
        }
    }
    printf("phi outside the clip range: %llu points of both signs and %llu swept values, 0 mismatches\n", n_out, n_side);

    /* 2. softplus: every finite float, positive then negative */
    unsigned long long n_sp = 0;
    f = sweep_softplus(0x00000000u, 0x7f7fffffu, &n_sp);
    if (f < 0) f = sweep_softplus(0x80000000u, 0xff7fffffu, &n_sp);
    if (report("softplus", f, f < 0 ? 0.0f : fg_softplus_max(fg_u2f((uint32_t)f)), f < 0 ? 0.0f : fg_softplus(fg_u2f((uint32_t)f)))) return 1;
    printf("softplus: %llu values, 0 mismatches\n", n_sp);
    return 0;
}
