/* Host evaluation of the check rules with one or two time-like inputs of feedback_gnn_amd/csrc/fgnn_cn_st.h (host code, no GPU;
 * built and run by tests/test_stbp4_reference_cpu.py with the oracle's compiler flags, and once more under the address and
 * undefined-behaviour sanitizers).  Reads float32 rows (deg, syndrome bit, number of extra inputs, factor, extra input 0, extra input
 * 1, 12 edge inputs) from stdin, deg in 0 .. 12, and prints one line per row of 5 groups of 14 words, the bits of the 12 slots after
 * the rule (a slot from deg on keeps its 0) and of the two outputs for the extra inputs (the second is 0 with one extra input):
 *   cn_st_update<boxplus>, cn_st_update<boxplus-phi>, cn_st_update<minsum>    the loop form
 *   cn_st_minsum_regular<12> with the row's deg                              the register form, guarded
 *   cn_st_minsum_regular<6> where deg is 6, else zeros                       the register form at its compile-time degree */
#include <stdio.h>

#include "fgnn_cn_st.h"

enum { DMAX = 12, HEAD = 6, ROW = HEAD + DMAX };

template <int CN_TYPE>
static void one(const float* r, const int* slot)
{
    const int deg = (int)r[0];
    const unsigned synd = r[1] != 0.0f;
    const float factor = r[3];
    float msg[DMAX], w[2] = {0.0f, 0.0f};
    for (int j = 0; j < DMAX; ++j) msg[j] = j < deg ? r[HEAD + j] : 0.0f;
    if ((int)r[2] == 1) {
        float x[1] = {r[4]};
        cn_st_update<CN_TYPE, 1, PhiSoft>(msg, slot, deg, synd, x, factor);
        w[0] = x[0];
    } else {
        float x[2] = {r[4], r[5]};
        cn_st_update<CN_TYPE, 2, PhiSoft>(msg, slot, deg, synd, x, factor);
        w[0] = x[0];
        w[1] = x[1];
    }
    for (int j = 0; j < DMAX; ++j) printf("%08x ", fg_f2u(msg[j]));
    printf("%08x %08x ", fg_f2u(w[0]), fg_f2u(w[1]));
}

// the register form of compile-time degree DC on the row's first `deg` inputs; zeros where `run` is false
template <int DC>
static void regular(const float* r, int deg, bool run)
{
    unsigned off[DC];
    for (int j = 0; j < DC; ++j) off[j] = 4u * (unsigned)j;
    float msg[DMAX], w[2] = {0.0f, 0.0f};
    for (int j = 0; j < DMAX; ++j) msg[j] = (run && j < deg) ? r[HEAD + j] : 0.0f;
    if (run) {
        const unsigned synd = r[1] != 0.0f;
        if ((int)r[2] == 1) {
            float x[1] = {r[4]};
            cn_st_minsum_regular<DC, 1>(msg, off, deg, synd, x, r[3]);
            w[0] = x[0];
        } else {
            float x[2] = {r[4], r[5]};
            cn_st_minsum_regular<DC, 2>(msg, off, deg, synd, x, r[3]);
            w[0] = x[0];
            w[1] = x[1];
        }
    }
    for (int j = 0; j < DMAX; ++j) printf("%08x ", fg_f2u(msg[j]));
    printf("%08x %08x ", fg_f2u(w[0]), fg_f2u(w[1]));
}

int main()
{
    float r[ROW];
    int slot[DMAX];
    for (int j = 0; j < DMAX; ++j) slot[j] = j;
    unsigned long rows = 0;
    while (fread(r, sizeof(float), ROW, stdin) == ROW) {
        const int deg = (int)r[0], nx = (int)r[2];
        if (deg < 0 || deg > DMAX || nx < 1 || nx > 2) return 2;
        one<FGNN_SOFT_BOXPLUS>(r, slot);
        one<FGNN_SOFT_BOXPLUS_PHI>(r, slot);
        one<FGNN_SOFT_MINSUM>(r, slot);
        regular<DMAX>(r, deg, true);
        regular<6>(r, 6, deg == 6);
        printf("\n");
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
