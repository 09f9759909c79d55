/* Host evaluation of the qubit rules of feedback_gnn_amd/csrc/fgnn_vn.h that need no elementary function (host code, no GPU; built and
 * run by tests/test_vn_rules_cpu.py with the oracle's compiler flags).  Reads float32 rows from stdin and prints one line per row:
 *   vn_rules_check totals   rows (Sz, Sx, lx, ly, lz)  ->  the bits of X, Y, Z of vn_totals and vn_decide of them
 *   vn_rules_check decide   rows (X, Y, Z)             ->  vn_decide
 * The softplus / log-sum-exp rules are held to the oracle by the exact GPU tests; instantiating them here only proves that the whole
 * header compiles for the host. */
#include <stdio.h>

#include "fgnn_vn.h"

int main(int argc, char** argv)
{
    const bool totals = argc > 1 && argv[1][0] == 't';
    float r[5];
    const size_t w = totals ? 5 : 3;
    unsigned long rows = 0;
    while (fread(r, sizeof(float), w, stdin) == w) {
        if (totals) {
            float X, Y, Z;
            vn_totals(r[0], r[1], r[2], r[3], r[4], X, Y, Z);
            printf("%08x %08x %08x %d\n", fg_f2u(X), fg_f2u(Y), fg_f2u(Z), vn_decide(X, Y, Z));
        } else {
            printf("%d\n", vn_decide(r[0], r[1], r[2]));
        }
        ++rows;
    }
    float llx, llz;
    vn_binary_llrs<VnMath>(1.0f, 2.0f, 3.0f, llx, llz);
    const float e = vn_edge<VnMath>(llx, 1.0f, 2.0f, 0.5f) + vn_edge_shared(llz, 0.0f, 1.0f, 2.0f, 0.5f);
    return (rows > 0 && e == e) ? 0 : 1;
}
