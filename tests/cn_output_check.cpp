/* Host evaluation of the single-output check rule of feedback_gnn_amd/csrc/fgnn_cn1.h next to the rule it restates, cn_update of
 * fgnn_cn.h (host code, no GPU; built and run by tests/test_mbp4_serial_reference_cpu.py with the oracle's compiler flags, and once
 * more under the address and undefined-behaviour sanitizers).  Reads float32 rows (deg, syndrome bit, factor, 8 edge inputs) from
 * stdin, deg in 0 .. 8, and prints one line per row of 3 groups (boxplus, boxplus-phi, min-sum) of 16 words: the bits of the 8 slots
 * after cn_update (a slot from deg on keeps its 0), then the bits of cn_output for j = 0 .. 7 (0 from deg on).  The check's slots are
 * scattered over a longer array, so that an index taken for a slot shows; cn_output must leave that array as it found it. */
#include <stdio.h>
#include <string.h>

#include "fgnn_cn1.h"

enum { DMAX = 8, HEAD = 3, ROW = HEAD + DMAX, STRIDE = 3, LEN = DMAX * STRIDE };

template <int CN_TYPE>
static int one(const float* r, const int* slot)
{
    const int deg = (int)r[0];
    const unsigned synd = r[1] != 0.0f;
    float nu[LEN], before[LEN], msg[LEN];
    for (int i = 0; i < LEN; ++i) nu[i] = 0.0f;
    for (int j = 0; j < deg; ++j) nu[slot[j]] = r[HEAD + j];
    memcpy(before, nu, sizeof nu);
    memcpy(msg, nu, sizeof nu);
    cn_update<CN_TYPE, PhiBp4>(msg, slot, deg, synd, r[2]);
    for (int j = 0; j < DMAX; ++j) printf("%08x ", j < deg ? fg_f2u(msg[slot[j]]) : 0u);
    for (int j = 0; j < DMAX; ++j) printf("%08x ", j < deg ? fg_f2u(cn_output<CN_TYPE, PhiBp4>(nu, slot, deg, j, synd, r[2])) : 0u);
    return memcmp(before, nu, sizeof nu) != 0;
}

int main()
{
    float r[ROW];
    int slot[DMAX];
    for (int j = 0; j < DMAX; ++j) slot[j] = (j * 5) % DMAX * STRIDE + 1;  // a permutation of 8 distinct slots, none of them j
    unsigned long rows = 0;
    while (fread(r, sizeof(float), ROW, stdin) == ROW) {
        const int deg = (int)r[0];
        if (deg < 0 || deg > DMAX) return 2;
        int wrote = one<FGNN_CN_BOXPLUS>(r, slot);
        wrote |= one<FGNN_CN_BOXPLUS_PHI>(r, slot);
        wrote |= one<FGNN_CN_MINSUM>(r, slot);
        if (wrote) return 3;
        printf("\n");
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
