// layers_check.cpp — host-only check of feedback_gnn_amd/csrc/fgnn_layers.h (no HIP, no Python): on a hand-written irregular CSS graph
// it builds the greedy layering and one custom layering of every kind, the device tables of each, and asserts what the kernels rely on;
// then it offers the validator one colliding layering per kind and compares the message.  Built and run by
// tests/test_layers_host_cpu.py, plain and under -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>

#include "fgnn_layers.h"

#define CHECK(cond)                                                        \
    do {                                                                   \
        if (!(cond)) {                                                     \
            std::printf("line %d: %s does not hold\n", __LINE__, #cond);   \
            std::exit(1);                                                  \
        }                                                                  \
    } while (0)

namespace FL = fgnn_layers;
using Vec = std::vector<int>;

// n = 7, m_x = 3, m_z = 2: check degrees 4, 3, 1 and 2, 4; hx check 2 has a single edge, qubit 6 has no hz edge
const int N = 7, MX = 3, MZ = 2, M = MX + MZ;
const int H[M][N] = {{1, 1, 1, 1, 0, 0, 0}, {0, 0, 1, 0, 1, 1, 0}, {0, 0, 0, 0, 0, 0, 1}, {1, 0, 0, 0, 1, 0, 0}, {0, 1, 1, 1, 0, 1, 0}};

// the views fgnn_graph keeps: slots VN-major (hx slots sorted by (qubit, check), then the hz slots), a check's row by ascending qubit
struct Graph {
    Vec vptr_x, vptr_z, vchk, cptr, cslot, cvn;
    int E_x = 0, E = 0;
};

Graph build()
{
    Graph g;
    for (int side = 0; side < 2; ++side) {
        Vec& vptr = side ? g.vptr_z : g.vptr_x;
        for (int v = 0; v < N; ++v) {
            vptr.push_back((int)g.vchk.size());
            for (int c = side ? MX : 0; c < (side ? M : MX); ++c)
                if (H[c][v]) g.vchk.push_back(c);  // combined check numbers
        }
        vptr.push_back((int)g.vchk.size());
        if (!side) g.E_x = (int)g.vchk.size();
    }
    g.E = (int)g.vchk.size();
    g.cptr.push_back(0);
    for (int c = 0; c < M; ++c) {
        for (int v = 0; v < N; ++v) {
            const Vec& vptr = c < MX ? g.vptr_x : g.vptr_z;
            for (int e = vptr[v]; e < vptr[v + 1]; ++e)
                if (g.vchk[e] == c) {
                    g.cslot.push_back(e);
                    g.cvn.push_back(v);
                }
        }
        g.cptr.push_back((int)g.cslot.size());
    }
    return g;
}

// ptr is non-decreasing from 0 and ends at `end`
void check_ptr(const Vec& ptr, int num_layers, size_t end)
{
    CHECK((int)ptr.size() == num_layers + 1 && ptr[0] == 0 && (size_t)ptr.back() == end);
    for (size_t l = 0; l + 1 < ptr.size(); ++l) CHECK(ptr[l] <= ptr[l + 1]);
}

// list is a permutation of 0..items-1, ascending inside a layer, and every item stands in its own layer
void check_buckets(const Vec& ptr, const Vec& list, int items, int num_layers, const int32_t* layer_of)
{
    check_ptr(ptr, num_layers, items);
    CHECK((int)list.size() == items);
    Vec seen(items, 0);
    for (int l = 0; l < num_layers; ++l)
        for (int i = ptr[l]; i < ptr[l + 1]; ++i) {
            CHECK(list[i] >= 0 && list[i] < items && !seen[list[i]]++ && layer_of[list[i]] == l);
            CHECK(i == ptr[l] || list[i - 1] < list[i]);
        }
}

void check_kind(const Graph& g, fgnn_layer_kind kind, int num_layers, const std::vector<int32_t>& lay)
{
    const int m = kind == LAYER_BITS ? MX : M, items = FL::item_count(kind, N, m);
    CHECK((int)lay.size() == items);
    CHECK(FL::validate(kind, N, MX, m, g.cptr, g.cvn, num_layers, lay.data()).empty());
    Vec ptr, list, eptr, edge, slot, cj;
    FL::bucket_by_layer(items, num_layers, lay.data(), ptr, list);
    check_buckets(ptr, list, items, num_layers, lay.data());
    if (kind == LAYER_CHECKS) {
        FL::check_layer_tables(ptr, list, g.cptr, g.cslot, g.cvn, eptr, edge);
        CHECK((int)edge.size() == 2 * g.E);
        check_ptr(eptr, num_layers, edge.size() / 2);
        int e = 0;
        for (int l = 0; l < num_layers; ++l) {
            for (int i = ptr[l]; i < ptr[l + 1]; ++i)
                for (int k = 0; k < g.cptr[list[i] + 1] - g.cptr[list[i]]; ++k, ++e) {
                    const int s = edge[2 * e], v = edge[2 * e + 1];
                    CHECK(s >= 0 && s < g.E && g.vchk[s] == list[i] && H[list[i]][v]);
                    const Vec& vptr = s < g.E_x ? g.vptr_x : g.vptr_z;
                    CHECK(vptr[v] <= s && s < vptr[v + 1]);      // the slot is one of qubit v's
                    CHECK(k == 0 || edge[2 * e - 1] < v);        // a check's edges by ascending qubit
                }
            CHECK(eptr[l + 1] == e);
        }
    }
    if (kind == LAYER_QUBITS) {
        FL::qubit_layer_tables(ptr, list, g.vptr_x, g.vptr_z, g.cptr, g.cslot, eptr, slot, cj);
        CHECK((int)slot.size() == g.E && (int)cj.size() == 2 * g.E);
        check_ptr(eptr, num_layers, slot.size());
        int e = 0;
        for (int l = 0; l < num_layers; ++l) {
            for (int i = ptr[l]; i < ptr[l + 1]; ++i) {
                const int v = list[i];
                for (int s = g.vptr_x[v]; s < g.vptr_x[v + 1]; ++s) CHECK(slot[e++] == s);  // its hx slots,
                for (int s = g.vptr_z[v]; s < g.vptr_z[v + 1]; ++s) CHECK(slot[e++] == s);  // then its hz slots
            }
            CHECK(eptr[l + 1] == e);
        }
        for (int s = 0; s < g.E; ++s) {
            const int c = cj[2 * s], j = cj[2 * s + 1];
            CHECK(c == g.vchk[s] && j >= 0 && j < g.cptr[c + 1] - g.cptr[c] && g.cslot[g.cptr[c] + j] == s);
        }
    }
}

void check_greedy(const Graph& g, fgnn_layer_kind kind, int want_layers, const std::vector<int32_t>& want)
{
    const int m = kind == LAYER_BITS ? MX : M;
    std::vector<int32_t> lay(FL::item_count(kind, N, m), -1);
    int32_t num = -1;
    FL::greedy(kind, N, m, g.cptr, g.cvn, lay.data(), &num);
    CHECK(num == want_layers && lay == want);
    check_kind(g, kind, num, lay);
}

void check_refused(const Graph& g, fgnn_layer_kind kind, int num_layers, const std::vector<int32_t>& lay, const std::string& want)
{
    const std::string got = FL::validate(kind, N, MX, kind == LAYER_BITS ? MX : M, g.cptr, g.cvn, num_layers, lay.data());
    if (got != want) std::printf("got  \"%s\"\nwant \"%s\"\n", got.c_str(), want.c_str());
    CHECK(got == want);
}

int main()
{
    const Graph g = build();
    CHECK(g.E_x == 8 && g.E == 14 && g.vptr_z[0] == g.E_x && g.vptr_z[6] == g.vptr_z[7]);
    // the greedy layerings, worked out by hand: an item goes into the first layer that holds no item sharing a node with it
    check_greedy(g, LAYER_CHECKS, 3, {0, 1, 0, 2, 2});
    check_greedy(g, LAYER_BITS, 2, {0, 1, 0});
    check_greedy(g, LAYER_QUBITS, 4, {0, 1, 2, 3, 1, 0, 0});
    // a custom layering per kind
    check_kind(g, LAYER_CHECKS, 5, {4, 3, 2, 1, 0});
    check_kind(g, LAYER_BITS, 2, {1, 0, 1});
    check_kind(g, LAYER_QUBITS, 7, {6, 5, 4, 3, 2, 1, 0});
    // a colliding layering per kind, and the other refusals
    check_refused(g, LAYER_CHECKS, 3, {0, 1, 0, 2, 1}, "hx check 1 and hz check 1 (number 4) of layer 1 share qubit 2");
    check_refused(g, LAYER_BITS, 2, {0, 0, 1}, "check 0 and check 1 of layer 0 share bit 2");
    check_refused(g, LAYER_QUBITS, 4, {0, 1, 2, 3, 1, 2, 0}, "qubit 2 and qubit 5 of layer 2 share hx check 1");
    check_refused(g, LAYER_CHECKS, 3, {0, 1, 0, 2, 3}, "hz check 1 (number 4) has layer 3, outside [0, 3)");
    check_refused(g, LAYER_QUBITS, 8, {7, 5, 4, 3, 2, 1, 0}, "layer 6 is empty");
    check_refused(g, LAYER_BITS, 0, {0, 1, 0}, "num_layers = 0 must be >= 1");
    CHECK(FL::validate(LAYER_BITS, N, MX, MX, g.cptr, g.cvn, 2, nullptr) == "layer_of is NULL");
    std::printf("ok\n");
    return 0;
}
