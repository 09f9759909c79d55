/* Host walk of vn_sums_dup of feedback_gnn_amd/csrc/fgnn_vn.h (host code, no GPU; built and run by
 * tests/test_bp4aug_reference_cpu.py with the oracle's compiler flags, and once more under the address and undefined-behaviour
 * sanitizers).  Reads records from stdin: int32 dx, int32 dz (each 0 .. 16), then dx + dz float32 messages (the hx run first, as in a
 * codeword's msg) and dx + dz mark bytes, indexed as the messages are.  The arrays of a record are heap blocks of exactly that size, so
 * a read past a run is the sanitizer's to find.  Prints one line per record: the bits of Sz and Sx of vn_sums_dup, and of vn_sums on
 * the same messages. */
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include "fgnn_vn.h"

int main()
{
    int32_t deg[2];
    unsigned long rows = 0;
    while (fread(deg, sizeof(int32_t), 2, stdin) == 2) {
        const int dx = deg[0], dz = deg[1];
        if (dx < 0 || dx > 16 || dz < 0 || dz > 16) return 2;
        const size_t E = (size_t)dx + (size_t)dz;
        float* msg = (float*)malloc(E ? E * sizeof(float) : 1);
        uint8_t* dup = (uint8_t*)malloc(E ? E : 1);
        if (!msg || !dup) return 3;
        if (fread(msg, sizeof(float), E, stdin) != E || fread(dup, 1, E, stdin) != E) return 4;
        float Sz, Sx, Pz, Px;
        vn_sums_dup(msg, dup, dx, dx + dz, 0, dx, Sz, Sx);
        vn_sums(msg, dx, dx + dz, 0, dx, Pz, Px);
        printf("%08x %08x %08x %08x\n", fg_f2u(Sz), fg_f2u(Sx), fg_f2u(Pz), fg_f2u(Px));
        free(msg);
        free(dup);
        ++rows;
    }
    return rows > 0 ? 0 : 1;
}
