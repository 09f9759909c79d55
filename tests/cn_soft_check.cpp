/* Host evaluation of the soft check rules of feedback_gnn_amd/csrc/fgnn_cn_soft.h (host code, no GPU; built and run by
 * tests/test_dsbp4_reference_cpu.py with the oracle's compiler flags, and once more under the address and undefined-behaviour
 * sanitizers).  Reads float32 rows (deg, syndrome bit, gamma, factor, 12 inputs) from stdin, deg in 0 .. 12, and prints one line per
 * row of 5 groups of 13 words, the bits of the 12 slots after the rule (a slot from deg on keeps its 0) and of w:
 *   cn_soft_update<boxplus>, cn_soft_update<boxplus-phi>, cn_soft_update<minsum>    the loop form
 *   cn_soft_minsum_regular<12> with the row's deg                                   the register form, guarded
 *   cn_soft_minsum_regular<6> where deg is 6, else zeros                            the register form at its compile-time degree */
#include <stdio.h>
#include <string.h>

#include "fgnn_cn_soft.h"

enum { DMAX = 12, ROW = 4 + DMAX };

static void emit(const float* msg, float w)
{
    for (int j = 0; j < DMAX; ++j) printf("%08x ", fg_f2u(msg[j]));
    printf("%08x ", fg_f2u(w));
}

int main()
{
    float r[ROW];
    int slot[DMAX];
    unsigned off12[DMAX], off6[6];
    for (int j = 0; j < DMAX; ++j) {
        slot[j] = j;
        off12[j] = 4u * (unsigned)j;
    }
    for (int j = 0; j < 6; ++j) off6[j] = 4u * (unsigned)j;
    unsigned long rows = 0;
    while (fread(r, sizeof(float), ROW, stdin) == ROW) {
        const int deg = (int)r[0];
        if (deg < 0 || deg > DMAX) return 2;
        const unsigned synd = r[1] != 0.0f;
        const float gamma = r[2], factor = r[3];
        float msg[DMAX], w;
        auto load = [&]() {
            for (int j = 0; j < DMAX; ++j) msg[j] = j < deg ? r[4 + j] : 0.0f;
        };
        load();
        w = cn_soft_update<FGNN_SOFT_BOXPLUS, PhiSoft>(msg, slot, deg, synd, gamma, factor);
        emit(msg, w);
        load();
        w = cn_soft_update<FGNN_SOFT_BOXPLUS_PHI, PhiSoft>(msg, slot, deg, synd, gamma, factor);
        emit(msg, w);
        load();
        w = cn_soft_update<FGNN_SOFT_MINSUM, PhiSoft>(msg, slot, deg, synd, gamma, factor);
        emit(msg, w);
        load();
        w = cn_soft_minsum_regular<DMAX>(msg, off12, deg, synd, gamma, factor);
        emit(msg, w);
        if (deg == 6) {
            load();
            w = cn_soft_minsum_regular<6>(msg, off6, 6, synd, gamma, factor);
        } else {
            memset(msg, 0, sizeof msg);
            w = 0.0f;
        }
        emit(msg, w);
        printf("\n");
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
