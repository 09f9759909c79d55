// fgnn_lsd.h — the per-sample sequential step of localized statistics decoding (fgnn_lsd, include/fgnn.h): the reduction of one column
// against the pivot list, the pivot choice, the syndrome update and the read-out, as __host__ __device__ routines over word arrays.
//
// A vector over the m checks is W = ceil(m / 32) words.  The routines are written for a group of LANES cooperating lanes: word w of the
// vector a group holds in registers sits in lane w % LANES, slot w / LANES (x[WPL], WPL >= ceil(W / LANES)); every word of the LDS /
// host arrays t, isPivot and L[k] is read and written by the lane that owns it and by no other, and piv[k] / col[k] by lane k % LANES,
// so the lanes of one wave need no fence between the steps.  `Lanes` says how the group talks:
//   LANES, lane()            the group size and this lane's index
//   fetch(v, src)            the value `v` of lane `src` (src uniform), uniform
//   min_all(v)               the least `v` of the group, uniform
// lsd_kernel runs them on one wave (LsdWave, fgnn_lsd.hip: v_readlane and a cross-lane minimum); a host program walks them with a
// group of one (LsdOneLane below: WPL = W words, all in lane 0), which is what tests/lsd_check.cpp holds to the NumPy restatement.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define LSD_HD __host__ __device__ __forceinline__
#else
#define LSD_HD inline
#endif

constexpr int LSD_NO_PIVOT = 0x7fffffff;

struct LsdOneLane {
    static constexpr int LANES = 1;
    static LSD_HD int lane() { return 0; }
    static LSD_HD unsigned fetch(unsigned v, int) { return v; }
    static LSD_HD int min_all(int v) { return v; }
};

// order-preserving float bits -> uint32 (the sort key of fgnn_osd.hip, step 1) of a reliability whose -0 has been made +0
LSD_HD unsigned lsd_sortable(unsigned float_bits) { return (float_bits & 0x80000000u) ? ~float_bits : (float_bits | 0x80000000u); }

LSD_HD int lsd_ctz(unsigned w)
{
#if defined(__HIP_DEVICE_COMPILE__)
    return __ffs((int)w) - 1;
#else
    return __builtin_ctz(w);
#endif
}

// word w (uniform) of the vector the group holds in x, uniform
template <int WPL, class Lanes>
LSD_HD unsigned lsd_word(const unsigned (&x)[WPL], int w)
{
    const int slot = w / Lanes::LANES;
    unsigned v = 0u;
#pragma unroll
    for (int j = 0; j < WPL; ++j)
        if (j == slot) v = x[j];
    return Lanes::fetch(v, w % Lanes::LANES);
}

// x = 0 with the bits of `checks[0..deg)` set (column v of H)
template <int WPL, class Lanes>
LSD_HD void lsd_column(unsigned (&x)[WPL], const int* checks, int deg)
{
    const int lane = Lanes::lane();
#pragma unroll
    for (int j = 0; j < WPL; ++j) x[j] = 0u;
    for (int i = 0; i < deg; ++i) {
        const int c = checks[i], w = c >> 5;
#pragma unroll
        for (int j = 0; j < WPL; ++j)
            if (w == lane + j * Lanes::LANES) x[j] |= 1u << (c & 31);
    }
}

// For k = 0 .. P-1 in order: if x[piv[k]] is set, x ^= L[k].  L[k] is stored with its own piv[k] bit cleared (lsd_store_pivot), so
// x[piv[k]] stays set.  At most P dependent steps, each one uniform bit test and, when it hits, one W-word XOR.
template <int WPL, class Lanes>
LSD_HD void lsd_reduce(unsigned (&x)[WPL], const int* piv, const unsigned* L, int P, int W)
{
    const int lane = Lanes::lane();
    for (int base = 0; base < P; base += Lanes::LANES) {
        const unsigned mine = base + lane < P ? (unsigned)piv[base + lane] : 0u;  // piv[base .. base + LANES) a lane each
        const int cnt = P - base < Lanes::LANES ? P - base : Lanes::LANES;
        for (int i = 0; i < cnt; ++i) {
            const int pk = (int)Lanes::fetch(mine, i);
            if ((lsd_word<WPL, Lanes>(x, pk >> 5) >> (pk & 31)) & 1u) {
                const unsigned* Lk = L + (size_t)(base + i) * W;
#pragma unroll
                for (int j = 0; j < WPL; ++j) {
                    const int w = lane + j * Lanes::LANES;
                    if (w < W) x[j] ^= Lk[w];
                }
            }
        }
    }
}

// the lowest non-pivot check set in x, or LSD_NO_PIVOT when x is zero on every non-pivot check (a dependent column)
template <int WPL, class Lanes>
LSD_HD int lsd_pivot(const unsigned (&x)[WPL], const unsigned* isPivot, int W)
{
    const int lane = Lanes::lane();
    int best = LSD_NO_PIVOT;
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        const int w = lane + j * Lanes::LANES;
        if (w < W && best == LSD_NO_PIVOT) {
            const unsigned f = x[j] & ~isPivot[w];
            if (f) best = w * 32 + lsd_ctz(f);
        }
    }
    return Lanes::min_all(best);
}

// Pivot P = (check p, bit v, vector x): piv[P] = p, col[P] = v, p marked in isPivot, L[P] = x with bit p cleared, and, if t[p] is
// set, t ^= x with bit p left out.
template <int WPL, class Lanes>
LSD_HD void lsd_store_pivot(const unsigned (&x)[WPL], int p, int v, int P, int* piv, int* col, unsigned* L, unsigned* isPivot,
                            unsigned* t, int W)
{
    const int lane = Lanes::lane();
    unsigned tw[WPL];
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        const int w = lane + j * Lanes::LANES;
        tw[j] = w < W ? t[w] : 0u;
    }
    const unsigned tp = (lsd_word<WPL, Lanes>(tw, p >> 5) >> (p & 31)) & 1u;
    if (lane == P % Lanes::LANES) {
        piv[P] = p;
        col[P] = v;
    }
    unsigned* LP = L + (size_t)P * W;
#pragma unroll
    for (int j = 0; j < WPL; ++j) {
        const int w = lane + j * Lanes::LANES;
        if (w < W) {
            unsigned xv = x[j];
            if (w == (p >> 5)) {
                xv &= ~(1u << (p & 31));
                isPivot[w] |= 1u << (p & 31);
            }
            LP[w] = xv;
            if (tp) t[w] = tw[j] ^ xv;
        }
    }
}

// read-out of pivot k: e[col[k]] = t[piv[k]] (every other bit of e is 0, written before)
LSD_HD void lsd_readout(int k, const int* piv, const int* col, const unsigned* t, uint8_t* e)
{
    const int p = piv[k];
    if ((t[p >> 5] >> (p & 31)) & 1u) e[col[k]] = 1;
}
