// fgnn_vn.h — qubit (variable-node) rules of quaternary BP shared by BP4 (fgnn_bp4.hip), Relay-BP4 (fgnn_relay4.hip), the reverse
// passes (fgnn_backward.hip, fgnn_gnnbp4_backward.hip), GNN_BP4 (fgnn_gnnbp4.hip) and OSD (fgnn_osd.hip).
//
// Each rule is the oracle's float operation sequence in the oracle's order (oracle/fgnn_oracle.c restates them independently): the
// association of the adds and the tie order of the decision are part of the rule.  The rules that evaluate a softplus or a
// log-sum-exp are parameterised by a policy MX with static MX::softplus(t) and MX::lse2(a, b), as the check rules of fgnn_cn.h are by
// PHI: BP4 passes its Mx<HWT> (the ranged log-sum-exp, or the opt-in hardware transcendentals), every other kernel passes VnMath
// (fg_softplus, fg_lse2).  Line numbers: decoding_q.py.  Host and device (FG_FN): tests/vn_rules_check.cpp runs the totals and the
// decision on the CPU.
#ifndef FGNN_VN_H
#define FGNN_VN_H

#include "fgnn_math.h"

struct VnMath {
    FG_FN float softplus(float t) { return fg_softplus(t); }
    FG_FN float lse2(float a, float b) { return fg_lse2(a, b); }
};

// sums of a qubit's c->v messages over its CSR runs, the hz run [z0,z1) first, then the hx run [x0,x1), each ascending from 0
FG_FN void vn_sums(const float* msg, int z0, int z1, int x0, int x1, float& Sz, float& Sx)
{
    Sz = 0.0f;
    Sx = 0.0f;
    for (int e = z0; e < z1; ++e) Sz = Sz + msg[e];
    for (int e = x0; e < x1; ++e) Sx = Sx + msg[e];
}

// the same sums on the code with some check rows written a second time, each copy directly after its original (augmented BP4,
// fgnn_bp4aug.hip): in flooding BP from zero messages a copy's message equals its original's bit for bit, so slot e with dup[e] != 0
// adds msg[e] twice in a row, the second a separate add.  dup is indexed as msg is.  With no mark set this is vn_sums
FG_FN void vn_sums_dup(const float* msg, const uint8_t* dup, int z0, int z1, int x0, int x1, float& Sz, float& Sx)
{
    Sz = 0.0f;
    Sx = 0.0f;
    for (int e = z0; e < z1; ++e) {
        Sz = Sz + msg[e];
        if (dup[e]) Sz = Sz + msg[e];
    }
    for (int e = x0; e < x1; ++e) {
        Sx = Sx + msg[e];
        if (dup[e]) Sx = Sx + msg[e];
    }
}

// totals (:244-248): hz messages carry X-or-Y evidence, hx messages Z-or-Y; Y = (Sz + Sx) + ly in this association
FG_FN void vn_totals(float Sz, float Sx, float lx, float ly, float lz, float& X, float& Y, float& Z)
{
    Y = (Sz + Sx) + ly;
    X = Sz + lx;
    Z = Sx + lz;
}

// v->c message of one edge (:254-273), literal form: num = softplus(-X) and A = Z on an hx edge, num = softplus(-Z) and A = X on an hz
// edge, mu = the edge's own c->v message
template <typename MX>
FG_FN float vn_edge(float num, float A, float Y, float mu)
{
    const float Ae = A - mu, Ye = Y - mu;
    return num - MX::lse2(-Ae, -Ye);
}

// the same edge with its own c->v message taken out at strength w (MBP4's inhibition term, fgnn_mbp4.hip): own = w * mu is one
// product, then the two subtractions (never an fma: the library is built with -ffp-contract=off).  w = 1.0f: own = mu bit for bit, so
// this is vn_edge
template <typename MX>
FG_FN float vn_edge_own(float num, float A, float Y, float mu, float w)
{
    const float own = w * mu;
    const float Ae = A - own, Ye = Y - own;
    return num - MX::lse2(-Ae, -Ye);
}

// the same edge in the shared form (FGNN_OPT_BP4_SHARED_LSE): (A - mu) - (Y - mu) = A - Y for every edge of a side, so the part of the
// log-sum-exp that depends on the difference alone, c = lse2_corr(-A, -Y), comes once per qubit and side
FG_FN float vn_edge_shared(float num, float c, float A, float Y, float mu)
{
    const float Ae = A - mu, Ye = Y - mu;
    return num - (c + FG_MAX(-Ae, -Ye));
}

// hard decision (:783-790): the smallest of X, Z, Y below 0, compared in that order with a strict '<' (a tie keeps the earlier one),
// else the identity.  d = 1 X, 2 Z, 3 Y: x_hat = d & 1, z_hat = d >> 1
FG_FN int vn_decide(float X, float Y, float Z)
{
    int d = 0;
    float best = 0.0f;
    if (X < best) { best = X; d = 1; }
    if (Z < best) { best = Z; d = 2; }
    if (Y < best) { best = Y; d = 3; }
    return d;
}

// binary LLRs of cal_logit (:455-464): llr_z = log P(no Z component) / P(Z component), the one the hx rows read, and llr_x for the hz rows
template <typename MX>
FG_FN float vn_llr_z(float X, float Y, float Z)
{
    return MX::softplus(-X) - MX::lse2(-Z, -Y);
}
template <typename MX>
FG_FN float vn_llr_x(float X, float Y, float Z)
{
    return MX::softplus(-Z) - MX::lse2(-X, -Y);
}
template <typename MX>
FG_FN void vn_binary_llrs(float X, float Y, float Z, float& llx, float& llz)
{
    llz = vn_llr_z<MX>(X, Y, Z);
    llx = vn_llr_x<MX>(X, Y, Z);
}

#endif
