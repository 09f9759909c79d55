// fgnn_layer.h — one check of a layer in the layered (serial) schedule of the binary decoders on side 0 (hx), stated once for
// bp2_layered_kernel (fgnn_bp2_layered.hip) and relay_layered_kernel (fgnn_relay_layered.hip).
//
// The codeword keeps, next to the messages mu_e, the running posteriors P_v.  A layer holds checks that share no bit
// (fgnn_graph_set_bit_layers validates it), so the thread of check c reads and writes only c's slots and the posteriors of c's bits,
// and no other thread of the layer touches either:
//     nu_e = P_v - mu_e   (one subtraction per edge, written into the slot)
//     mu_e = the check rule of fgnn_cn.h / fgnn_cn2.h on the slots, in place, unchanged
//     P_v  = nu_e + mu_e  (one addition per edge)
// The compile-time-degree forms keep nu in registers across the rule; the loop form parks it in P[v], which nobody else reads until
// the layer's barrier.
#ifndef FGNN_LAYER_H
#define FGNN_LAYER_H

#include "fgnn_step.h"
#include "fgnn_cn.h"
#include "fgnn_cn2.h"

// DV/DC as bit_dispatch deals them: DV > 0 the packed rows of a (DV,DC)-regular hx; DV = 0, DC > 0 min-sum on runtime degrees up to
// DC, predicated; DV = DC = 0 the loop over the CSR tables.  sy: the check's syndrome bit; f1: factor == 1.0f (the phi rule's)
template <int CN_TYPE, int DV, int DC>
__device__ __forceinline__ void layer_check(const GraphDev& g, float* msg, float* P, const int c, const unsigned sy, const float factor,
                                            const bool f1)
{
    if constexpr (DV > 0) {
        unsigned off[DC];
        row_unpack(g, c, off);
        float nu[DC];
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            nu[j] = P[row_qubit<DV>(off[j], 0u)] - slot_ref(msg, off[j]);
            slot_ref(msg, off[j]) = nu[j];
        }
        if constexpr (CN_TYPE == FGNN_CN_MINSUM) cn_minsum_regular<DC>(msg, off, DC, sy, factor);
        else cn2_phi_regular<DC>(msg, off, sy, factor, f1);
#pragma unroll
        for (int j = 0; j < DC; ++j) P[row_qubit<DV>(off[j], 0u)] = nu[j] + slot_ref(msg, off[j]);
    } else if constexpr (DC > 0 && CN_TYPE == FGNN_CN_MINSUM) {
        // runtime degrees up to DC: edge j is masked out where j >= deg (bp2_kernel's predicated form)
        const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
        unsigned off[DC];
        int vn[DC];
        float nu[DC];
#pragma unroll
        for (int j = 0; j < DC; ++j) {
            off[j] = (j < deg) ? 4u * (unsigned)g.cslot[c0 + j] : 0u;
            vn[j] = (j < deg) ? g.cvn[c0 + j] : 0;
        }
#pragma unroll
        for (int j = 0; j < DC; ++j)
            if (j < deg) {
                nu[j] = P[vn[j]] - slot_ref(msg, off[j]);
                slot_ref(msg, off[j]) = nu[j];
            }
        cn_minsum_regular<DC>(msg, off, deg, sy, factor);
#pragma unroll
        for (int j = 0; j < DC; ++j)
            if (j < deg) P[vn[j]] = nu[j] + slot_ref(msg, off[j]);
    } else {
        // the loop: nu waits in P[v] while the rule works on the slots
        const int c0 = g.cptr[c], deg = g.cptr[c + 1] - c0;
        const int* slot = g.cslot + c0;
        const int* vn = g.cvn + c0;
        for (int j = 0; j < deg; ++j) {
            const int s = slot[j], v = vn[j];
            const float nu = P[v] - msg[s];
            msg[s] = nu;
            P[v] = nu;
        }
        cn_update<CN_TYPE, PhiGnn>(msg, slot, deg, sy, factor);
        for (int j = 0; j < deg; ++j) {
            const int v = vn[j];
            P[v] = P[v] + msg[slot[j]];
        }
    }
}

#endif
