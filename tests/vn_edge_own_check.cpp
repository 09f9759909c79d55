/* Host evaluation of vn_edge_own of feedback_gnn_amd/csrc/fgnn_vn.h with the VnMath policy (host code, no GPU; built and run by
 * tests/test_mbp4_reference_cpu.py with the oracle's compiler flags, and once more under the address and undefined-behaviour
 * sanitizers).  Reads float32 rows (num, A, Y, mu, w) from stdin and prints one line per row: the bits of vn_edge_own, and the bits
 * of vn_edge on the same row without w (equal to the first whenever w is 1). */
#include <stdio.h>

#include "fgnn_vn.h"

int main()
{
    float r[5];
    unsigned long rows = 0;
    while (fread(r, sizeof(float), 5, stdin) == 5) {
        const float own = vn_edge_own<VnMath>(r[0], r[1], r[2], r[3], r[4]);
        const float plain = vn_edge<VnMath>(r[0], r[1], r[2], r[3]);
        printf("%08x %08x\n", fg_f2u(own), fg_f2u(plain));
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
