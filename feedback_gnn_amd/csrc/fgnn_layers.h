// fgnn_layers.h — the layerings of the serial schedules on the host: the greedy layering, the validation of a caller's one and the
// tables the kernels read, for the three kinds fgnn_graph carries (fgnn_internal.h).  Vectors in, vectors out: no HIP header and no
// device call, so a host compiler builds it alone (tests/layers_check.cpp).
//
// A layering gives every ITEM a layer such that no two items of a layer share a NODE:
//   LAYER_CHECKS  items = all checks (hx checks 0..m_x-1, then hz checks m_x..m-1), nodes = qubits   fgnn_bp4_decode_layered
//   LAYER_BITS    items = the hx checks alone,                                      nodes = bits     fgnn_bp2_decode_layered, fgnn_relay_decode_layered
//   LAYER_QUBITS  items = qubits,                                                   nodes = checks   fgnn_mbp4_decode_serial
// Every function takes the graph check-major: the qubits of check c = cvn[cptr[c] .. cptr[c+1]), of which a kind reads the rows of its
// own checks (LAYER_BITS: rows 0..m_x-1 of the combined view).
#pragma once
#include <stdint.h>

#include <string>
#include <vector>

enum fgnn_layer_kind { LAYER_CHECKS, LAYER_BITS, LAYER_QUBITS };

namespace fgnn_layers {

// rows -> columns becomes columns -> rows, every column's rows ascending (so transposing twice sorts every row)
inline void transpose(int rows, int cols, const std::vector<int>& ptr, const std::vector<int>& idx, std::vector<int>& tptr,
                      std::vector<int>& tidx)
{
    tptr.assign(cols + 1, 0);
    for (int p = 0; p < ptr[rows]; ++p) tptr[idx[p] + 1]++;
    for (int c = 0; c < cols; ++c) tptr[c + 1] += tptr[c];
    tidx.resize(ptr[rows]);
    std::vector<int> fill(tptr.begin(), tptr.end() - 1);
    for (int r = 0; r < rows; ++r)
        for (int p = ptr[r]; p < ptr[r + 1]; ++p) tidx[fill[idx[p]]++] = r;
}

// items in ascending order, each into the first layer that holds no item sharing a node with it; nodes of item i = idx[ptr[i] .. ptr[i+1])
inline void greedy_layers(int nodes, int items, const std::vector<int>& ptr, const std::vector<int>& idx, int32_t* layer_of,
                          int32_t* num_layers)
{
    std::vector<std::vector<int>> at(nodes);  // the layers that hold an item of node v
    std::vector<int> seen;                    // seen[l] == i + 1: layer l holds an item that shares a node with item i
    int L = 0;
    for (int i = 0; i < items; ++i) {
        for (int p = ptr[i]; p < ptr[i + 1]; ++p)
            for (int l : at[idx[p]]) seen[l] = i + 1;
        int l = 0;
        while (l < L && seen[l] == i + 1) ++l;
        if (l == L) {
            ++L;
            seen.push_back(0);
        }
        layer_of[i] = l;
        for (int p = ptr[i]; p < ptr[i + 1]; ++p) at[idx[p]].push_back(l);
    }
    *num_layers = L;
}

// "" for a valid layering, else the message that names the first offender: nodes ascending, the items of node v = idx[ptr[v] ..
// ptr[v+1]) ascending; stamp[l] = the last node with an item in layer l, owner[l] = that item: two at one node in one layer collide
template <typename ItemName, typename NodeName>
std::string validate_layers(int items, int nodes, const std::vector<int>& ptr, const std::vector<int>& idx, int num_layers,
                            const int32_t* layer_of, ItemName item, NodeName node)
{
    if (!layer_of) return "layer_of is NULL";
    if (num_layers < 1) return "num_layers = " + std::to_string(num_layers) + " must be >= 1";
    std::vector<int> count(num_layers, 0);
    for (int i = 0; i < items; ++i) {
        if (layer_of[i] < 0 || layer_of[i] >= num_layers)
            return item(i) + " has layer " + std::to_string(layer_of[i]) + ", outside [0, " + std::to_string(num_layers) + ")";
        count[layer_of[i]]++;
    }
    for (int l = 0; l < num_layers; ++l)
        if (!count[l]) return "layer " + std::to_string(l) + " is empty";
    std::vector<int> owner(num_layers, -1), stamp(num_layers, -1);
    for (int v = 0; v < nodes; ++v)
        for (int p = ptr[v]; p < ptr[v + 1]; ++p) {
            const int i = idx[p], l = layer_of[i];
            if (stamp[l] == v && owner[l] != i)
                return item(owner[l]) + " and " + item(i) + " of layer " + std::to_string(l) + " share " + node(v);
            stamp[l] = v;
            owner[l] = i;
        }
    return "";
}

inline std::string check_name(int c, int m_x)
{
    return c < m_x ? "hx check " + std::to_string(c) : "hz check " + std::to_string(c - m_x) + " (number " + std::to_string(c) + ")";
}

inline int item_count(fgnn_layer_kind kind, int n, int m) { return kind == LAYER_QUBITS ? n : m; }

// the greedy layering of a kind; m = the kind's checks (LAYER_BITS: m_x), layer_of [item_count]
inline void greedy(fgnn_layer_kind kind, int n, int m, const std::vector<int>& cptr, const std::vector<int>& cvn, int32_t* layer_of,
                   int32_t* num_layers)
{
    if (kind != LAYER_QUBITS) return greedy_layers(n, m, cptr, cvn, layer_of, num_layers);
    std::vector<int> vptr, vchk;
    transpose(m, n, cptr, cvn, vptr, vchk);
    greedy_layers(m, n, vptr, vchk, layer_of, num_layers);  // the check layering with the two kinds of node exchanged
}

// validates a caller's layering of a kind; the rows of cvn need not be sorted
inline std::string validate(fgnn_layer_kind kind, int n, int m_x, int m, const std::vector<int>& cptr, const std::vector<int>& cvn,
                            int num_layers, const int32_t* layer_of)
{
    const auto number = [](const char* what) { return [what](int i) { return what + std::to_string(i); }; };
    const auto check = [m_x](int c) { return check_name(c, m_x); };
    std::vector<int> vptr, vchk, sptr, svn;
    transpose(m, n, cptr, cvn, vptr, vchk);
    if (kind == LAYER_CHECKS) return validate_layers(m, n, vptr, vchk, num_layers, layer_of, check, number("qubit "));
    if (kind == LAYER_BITS) return validate_layers(m, n, vptr, vchk, num_layers, layer_of, number("check "), number("bit "));
    transpose(n, m, vptr, vchk, sptr, svn);
    return validate_layers(n, m, sptr, svn, num_layers, layer_of, number("qubit "), check);
}

// the items of layer l = list[ptr[l] .. ptr[l+1]) ascending
inline void bucket_by_layer(int items, int num_layers, const int32_t* layer_of, std::vector<int>& ptr, std::vector<int>& list)
{
    ptr.assign(num_layers + 1, 0);
    for (int i = 0; i < items; ++i) ptr[layer_of[i] + 1]++;
    for (int l = 0; l < num_layers; ++l) ptr[l + 1] += ptr[l];
    list.resize(items);
    std::vector<int> fill(ptr.begin(), ptr.end() - 1);
    for (int i = 0; i < items; ++i) list[fill[layer_of[i]]++] = i;
}

// LAYER_CHECKS: the edges of the checks of layer l, in the order of lay_chk and of the graph's check rows (ascending qubit), =
// lay_edge[lay_eptr[l] .. lay_eptr[l+1]) as (slot, qubit) pairs
inline void check_layer_tables(const std::vector<int>& lay_cptr, const std::vector<int>& lay_chk, const std::vector<int>& cptr,
                               const std::vector<int>& cslot, const std::vector<int>& cvn, std::vector<int>& lay_eptr,
                               std::vector<int>& lay_edge)
{
    lay_eptr.assign(lay_cptr.size(), 0);
    lay_edge.clear();
    for (size_t l = 0; l + 1 < lay_cptr.size(); ++l) {
        for (int i = lay_cptr[l]; i < lay_cptr[l + 1]; ++i)
            for (int p = cptr[lay_chk[i]]; p < cptr[lay_chk[i] + 1]; ++p) {
                lay_edge.push_back(cslot[p]);
                lay_edge.push_back(cvn[p]);
            }
        lay_eptr[l + 1] = (int)(lay_edge.size() / 2);
    }
}

// LAYER_QUBITS: the slots of the qubits of layer l, in the order of lay_qub (a qubit's hx slots, then its hz slots), = lay_slot[lay_eptr[l]
// .. lay_eptr[l+1]), and for every slot e its check and its place in the check's row: slot_cj[e] = (c, j) with cslot[cptr[c] + j] = e.
// vptr_x / vptr_z as the graph keeps them: the first hx / hz slot of a qubit, the hz slots already offset by E_x
inline void qubit_layer_tables(const std::vector<int>& lay_qptr, const std::vector<int>& lay_qub, const std::vector<int>& vptr_x,
                               const std::vector<int>& vptr_z, const std::vector<int>& cptr, const std::vector<int>& cslot,
                               std::vector<int>& lay_eptr, std::vector<int>& lay_slot, std::vector<int>& slot_cj)
{
    lay_eptr.assign(lay_qptr.size(), 0);
    lay_slot.clear();
    for (size_t l = 0; l + 1 < lay_qptr.size(); ++l) {
        for (int i = lay_qptr[l]; i < lay_qptr[l + 1]; ++i) {
            const int v = lay_qub[i];
            for (int e = vptr_x[v]; e < vptr_x[v + 1]; ++e) lay_slot.push_back(e);
            for (int e = vptr_z[v]; e < vptr_z[v + 1]; ++e) lay_slot.push_back(e);
        }
        lay_eptr[l + 1] = (int)lay_slot.size();
    }
    slot_cj.resize(2 * cslot.size());
    for (size_t c = 0; c + 1 < cptr.size(); ++c)
        for (int p = cptr[c]; p < cptr[c + 1]; ++p) {
            slot_cj[2 * (size_t)cslot[p]] = (int)c;
            slot_cj[2 * (size_t)cslot[p] + 1] = p - cptr[c];
        }
}

}  // namespace fgnn_layers
