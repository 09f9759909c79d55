/* Bit comparison of feedback_gnn_amd/csrc/fgnn_math_ranged.h with the fgnn_math.h routines it stands for (host code, no GPU;
 * built and run by tests/test_math_ranged.py with the oracle's compiler flags).
 *   1. fg_log_1to2(x) == fg_log(x) for EVERY float in [1, 2]: 2^23 + 1 values.
 *   2. fg_lse2_ranged / fg_lse2_corr_ranged == fg_lse2 / fg_lse2_corr on all ordered pairs of a grid: zeros of both signs, equal
 *      arguments, differences just below, at and just above 20 (where the exponential's argument is clamped), magnitudes to 1e4.
 * Prints one line per part and exits 1 on any mismatch. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "fgnn_math_ranged.h"

static int same(float a, float b) { return fg_f2u(a) == fg_f2u(b); }

int main(void)
{
    unsigned long bad_log = 0, n_log = 0;
    for (uint32_t u = fg_f2u(1.0f); u <= fg_f2u(2.0f); ++u) {
        const float x = fg_u2f(u);
        ++n_log;
        if (!same(fg_log_1to2(x), fg_log(x))) {
            if (bad_log < 5) printf("log mismatch at 0x%08x: %a vs %a\n", u, fg_log_1to2(x), fg_log(x));
            ++bad_log;
        }
    }
    printf("log_1to2: %lu values, %lu mismatches\n", n_log, bad_log);

    static float grid[4096];
    int n = 0;
    const float base[] = {0.0f, 1e-30f, 1e-7f, 0.5f, 1.0f, 3.3f, 13.9423847f, 16.635532f, 20.0f, 37.5f, 87.0f, 100.0f, 1e3f, 1e4f};
    const float d20lo = nextafterf(20.0f, 0.0f), d20hi = nextafterf(20.0f, 100.0f);
    const float diff[] = {0.0f, 1e-7f, 0.1f, 1.0f, 5.0f, 10.0f, 19.5f, d20lo, 20.0f, d20hi, 20.5f, 25.0f, 100.0f};
    for (unsigned i = 0; i < sizeof(base) / sizeof(base[0]); ++i)
        for (int s = 0; s < 2; ++s) {
            const float a = s ? -base[i] : base[i]; /* includes -0 */
            for (unsigned k = 0; k < sizeof(diff) / sizeof(diff[0]); ++k) {
                grid[n++] = a + diff[k];
                grid[n++] = a - diff[k];
            }
        }
    grid[n++] = -0.0f;
    unsigned long bad_lse = 0, n_lse = 0, near20 = 0, equal = 0;
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < n; ++j) {
            const float a = grid[i], b = grid[j];
            ++n_lse;
            equal += a == b;
            const float d = fabsf(a - b);
            near20 += d == d20lo || d == d20hi;
            if (!same(fg_lse2_ranged(a, b), fg_lse2(a, b)) || !same(fg_lse2_corr_ranged(a, b), fg_lse2_corr(a, b))) {
                if (bad_lse < 5) printf("lse2 mismatch at (%a, %a): %a vs %a\n", a, b, fg_lse2_ranged(a, b), fg_lse2(a, b));
                ++bad_lse;
            }
        }
    printf("lse2: %lu pairs (%lu equal, %lu one ulp from |a-b| = 20), %lu mismatches\n", n_lse, equal, near20, bad_lse);
    return (bad_log || bad_lse || near20 == 0) ? 1 : 0;
}
