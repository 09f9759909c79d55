/* Host walk of the per-sample sequential step of fgnn_lsd (feedback_gnn_amd/csrc/fgnn_lsd.h; host code, no GPU; built and run by
 * tests/test_lsd_reference_cpu.py, once plain and once under the address and undefined-behaviour sanitizers).  The rounds of the
 * contract in include/fgnn.h — validity, selection, the union of the clusters — are written out here in plain C++; every appended
 * column goes through the header's routines with a lane group of one (LsdOneLane: all W words in lane 0): lsd_column, lsd_reduce,
 * lsd_pivot, lsd_store_pivot, and lsd_readout at the end.
 * Input (argv[1], text): the number of cases; per case "m n max_pivots max_rounds B", then m rows "deg v0 v1 ..", then per sample m
 * syndrome bits and n sortable reliabilities (uint32).  Output: per sample one line "e_hat as n digits | found rounds columns pivots". */
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "fgnn_lsd.h"

constexpr int MAXW = 128;  // m <= 4096

static int read_int(FILE* f)
{
    long long v;
    if (fscanf(f, "%lld", &v) != 1) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return (int)v;
}

static unsigned read_u32(FILE* f)
{
    unsigned long long v;
    if (fscanf(f, "%llu", &v) != 1) {
        fprintf(stderr, "short input\n");
        exit(2);
    }
    return (unsigned)v;
}

int main(int argc, char** argv)
{
    if (argc != 2) return 2;
    FILE* f = fopen(argv[1], "r");
    if (!f) return 2;
    const int cases = read_int(f);
    for (int cs = 0; cs < cases; ++cs) {
        const int m = read_int(f), n = read_int(f), max_pivots = read_int(f), max_rounds = read_int(f), B = read_int(f);
        const int W = (m + 31) / 32;
        if (W > MAXW) return 3;
        const int cap = max_pivots ? max_pivots : std::min(m, n);
        std::vector<std::vector<int>> rows(m), cols(n);
        for (int c = 0; c < m; ++c) {
            const int deg = read_int(f);
            for (int i = 0; i < deg; ++i) {
                const int v = read_int(f);
                rows[c].push_back(v);
                cols[v].push_back(c);
            }
        }
        for (int b = 0; b < B; ++b) {
            std::vector<unsigned> t(W, 0u), isPivot(W, 0u), L((size_t)cap * W + 1, 0u);
            std::vector<int> lab(m, -1), piv(cap + 1, 0), col(cap + 1, 0);
            std::vector<char> inB(n, 0), dead(m, 0);
            std::vector<unsigned long long> key(n);
            for (int c = 0; c < m; ++c)
                if (read_int(f) & 1) {
                    t[c >> 5] |= 1u << (c & 31);
                    lab[c] = c;
                }
            for (int v = 0; v < n; ++v) key[v] = ((unsigned long long)read_u32(f) << 32) | (unsigned)v;
            int P = 0, rounds = 0, columns = 0;
            bool capped = false;
            for (;;) {
                std::vector<char> invalid(m, 0);
                for (int c = 0; c < m; ++c)
                    if (lab[c] >= 0 && ((t[c >> 5] & ~isPivot[c >> 5]) >> (c & 31)) & 1u) invalid[lab[c]] = 1;
                bool grow = false;
                for (int l = 0; l < m; ++l) grow = grow || (invalid[l] && !dead[l]);
                if (!grow || capped || (max_rounds && rounds >= max_rounds)) break;
                ++rounds;
                std::vector<unsigned long long> best(m, ~0ull), S;
                for (int c = 0; c < m; ++c) {
                    const int l = lab[c];
                    if (l < 0 || !invalid[l] || dead[l]) continue;
                    for (int v : rows[c])
                        if (!inB[v]) best[l] = std::min(best[l], key[v]);
                }
                for (int l = 0; l < m; ++l)
                    if (invalid[l] && !dead[l]) {
                        if (best[l] == ~0ull) dead[l] = 1;
                        else S.push_back(best[l]);
                    }
                std::sort(S.begin(), S.end());
                S.erase(std::unique(S.begin(), S.end()), S.end());
                for (unsigned long long k : S) {
                    const int v = (int)(unsigned)k;
                    inB[v] = 1;
                    int root = m;
                    for (int c : cols[v]) root = std::min(root, lab[c] < 0 ? c : lab[c]);
                    for (int c : cols[v]) {
                        const int old = lab[c];
                        if (old < 0) lab[c] = root;
                        else if (old != root)
                            for (int d = 0; d < m; ++d)
                                if (lab[d] == old) lab[d] = root;
                    }
                    ++columns;
                    unsigned x[MAXW];
                    lsd_column<MAXW, LsdOneLane>(x, cols[v].data(), (int)cols[v].size());
                    lsd_reduce<MAXW, LsdOneLane>(x, piv.data(), L.data(), P, W);
                    const int p = lsd_pivot<MAXW, LsdOneLane>(x, isPivot.data(), W);
                    if (p == LSD_NO_PIVOT) continue;
                    if (P == cap) {
                        capped = true;
                        break;
                    }
                    lsd_store_pivot<MAXW, LsdOneLane>(x, p, v, P, piv.data(), col.data(), L.data(), isPivot.data(), t.data(), W);
                    ++P;
                }
            }
            std::vector<uint8_t> e(n, 0);
            for (int k = 0; k < P; ++k) lsd_readout(k, piv.data(), col.data(), t.data(), e.data());
            bool bad = false;
            for (int w = 0; w < W; ++w) bad = bad || (t[w] & ~isPivot[w]);
            for (int v = 0; v < n; ++v) putchar('0' + e[v]);
            printf(" | %d %d %d %d\n", bad ? 0 : 1, rounds, columns, P);
        }
    }
    fclose(f);
    return 0;
}
