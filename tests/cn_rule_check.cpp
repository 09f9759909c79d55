/* Host evaluation of the check rules of feedback_gnn_amd/csrc/fgnn_cn.h with no, one or two extra inputs (host code, no GPU; built
 * and run by tests/test_cn_rule_cpu.py, tests/test_dsbp4_reference_cpu.py and tests/test_stbp4_reference_cpu.py with the oracle's
 * compiler flags, and once more under the address and undefined-behaviour sanitizers).  Reads float32 rows (deg, syndrome bit, number
 * of extra inputs, factor, extra input 0, extra input 1, 12 edge inputs) from stdin, deg in 0 .. 12, and prints one line per row of 5
 * groups of 14 words, the bits of the 12 slots after the rule (a slot from deg on keeps its 0) and of the two outputs for the extra
 * inputs (0 for an extra input the row does not have):
 *   cn_update<boxplus>, cn_update<boxplus-phi>, cn_update<minsum>    the loop form
 *   cn_minsum_regular<12> with the row's deg                        the register form, guarded
 *   cn_minsum_regular<6> where deg is 6, else zeros                 the register form at its compile-time degree */
#include <stdio.h>

#include "fgnn_cn.h"

enum { DMAX = 12, HEAD = 6, ROW = HEAD + DMAX };

static void emit(const float* msg, const float* x, int nx)
{
    for (int j = 0; j < DMAX; ++j) printf("%08x ", fg_f2u(msg[j]));
    printf("%08x %08x ", nx > 0 ? fg_f2u(x[0]) : 0u, nx > 1 ? fg_f2u(x[1]) : 0u);
}

template <int CN_TYPE>
static void one(const float* r, const int* slot)
{
    const int deg = (int)r[0], nx = (int)r[2];
    const unsigned synd = r[1] != 0.0f;
    float msg[DMAX];
    for (int j = 0; j < DMAX; ++j) msg[j] = j < deg ? r[HEAD + j] : 0.0f;
    if (nx == 0) {  // x is the null pointer: the rule must not read it
        cn_update<CN_TYPE, PhiBp4>(msg, slot, deg, synd, r[3]);
        emit(msg, nullptr, 0);
    } else if (nx == 1) {
        float x[1] = {r[4]};
        cn_update<CN_TYPE, PhiBp4, 1>(msg, slot, deg, synd, r[3], x);
        emit(msg, x, 1);
    } else {
        float x[2] = {r[4], r[5]};
        cn_update<CN_TYPE, PhiBp4, 2>(msg, slot, deg, synd, r[3], x);
        emit(msg, x, 2);
    }
}

// the register form of compile-time degree DC on the row's first `deg` inputs; zeros where `run` is false
template <int DC>
static void regular(const float* r, int deg, bool run)
{
    const int nx = run ? (int)r[2] : 0;
    unsigned off[DC];
    for (int j = 0; j < DC; ++j) off[j] = 4u * (unsigned)j;
    const unsigned synd = r[1] != 0.0f;
    float msg[DMAX];
    for (int j = 0; j < DMAX; ++j) msg[j] = (run && j < deg) ? r[HEAD + j] : 0.0f;
    if (nx == 0) {
        if (run) cn_minsum_regular<DC>(msg, off, deg, synd, r[3]);
        emit(msg, nullptr, 0);
    } else if (nx == 1) {
        float x[1] = {r[4]};
        cn_minsum_regular<DC, 1>(msg, off, deg, synd, r[3], x);
        emit(msg, x, 1);
    } else {
        float x[2] = {r[4], r[5]};
        cn_minsum_regular<DC, 2>(msg, off, deg, synd, r[3], x);
        emit(msg, x, 2);
    }
}

int main()
{
    float r[ROW];
    int slot[DMAX];
    for (int j = 0; j < DMAX; ++j) slot[j] = j;
    unsigned long rows = 0;
    while (fread(r, sizeof(float), ROW, stdin) == ROW) {
        const int deg = (int)r[0], nx = (int)r[2];
        if (deg < 0 || deg > DMAX || nx < 0 || nx > 2) return 2;
        one<FGNN_CN_BOXPLUS>(r, slot);
        one<FGNN_CN_BOXPLUS_PHI>(r, slot);
        one<FGNN_CN_MINSUM>(r, slot);
        regular<DMAX>(r, deg, true);
        regular<6>(r, 6, deg == 6);
        printf("\n");
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
