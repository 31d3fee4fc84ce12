// seed_window.h — "which of 32 consecutive seed-window starts may be a seed hit", written once (no HIP in here: the filters of
// k34_filter.h and k4_device.h instantiate it with the device's primitives, tests/sanitize/seed_window_check.cc with the host's).
//
// The input is a bit plane of mismatching columns n (two words, n0 = the lower 32 columns) and, for the exact rule, the plane of
// transversions d.  The window that starts at column BASE + i covers the columns BASE + i + c of the care positions c of CARE;
// start i is POSSIBLE when
//     transitions:     at most one of its care columns mismatches (and, TV, none of them is a transversion),
//     no transitions:  none of its care columns mismatches.
// Bit i of the result is set for a possible start.  CARE = all twelve care positions + TV: the exact 12of19 rule with one
// transition; fewer positions / no TV: a superset of it.
//
// The count is a carry-save adder over the K shifted copies of n, never a serial ones / twos counter: every three words give a
// sum word (XOR3) and a carry word (MAJ3), the sum words and the words left over are counted again the same way, and
//     "two or more"  = any carry, or two of the last two or three words;
//     "one or more"  = "two or more", or any of the last words (a full adder loses no set input: it shows in the sum or the carry).
// Every step is ONE three-input boolean function, which the traits struct P evaluates from its truth table (gfx950: one
// v_bitop3_b32 / v_or3_b32 each); K = 10 costs 12 of them instead of 24 two-input ones, K = 12 with the plane of
// transversions 20 instead of 33.  P has
//     static uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh);          // bits sh .. sh + 31 of hi:lo, sh = 0 .. 31
//     template <uint32_t TT> static uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c);
//         // bit j of the result = bit (4 a_j + 2 b_j + c_j) of TT
#pragma once
#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SEED_WINDOW_FN __host__ __device__ __forceinline__
#define SEED_WINDOW_UNROLL _Pragma("unroll")
#else
#define SEED_WINDOW_FN inline
#define SEED_WINDOW_UNROLL
#endif

namespace mimeo {
namespace seed_window {

// truth tables (a = 0xF0, b = 0xCC, c = 0xAA)
constexpr uint32_t TT_XOR3 = 0x96u, TT_MAJ3 = 0xE8u, TT_OR3 = 0xFEu, TT_A_OR_BC = 0xF8u;

// the host's primitives: 64-bit shifts and a loop over the rows of the truth table
struct HostOps {
    static inline uint32_t funnel(uint32_t lo, uint32_t hi, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u)); }
    template <uint32_t TT>
    static inline uint32_t bitop3(uint32_t a, uint32_t b, uint32_t c) {
        uint32_t r = 0;
        for (uint32_t row = 0; row < 8; row++)   // the columns whose (a, b, c) is this row of the table
            if ((TT >> row) & 1u) r |= (row & 4u ? a : ~a) & (row & 2u ? b : ~b) & (row & 1u ? c : ~c);
        return r;
    }
};

constexpr int popcount32(uint32_t x) { return x ? (int)(x & 1u) + popcount32(x >> 1) : 0; }

// OR of x[0 .. M), M >= 1, three words at a time
template <class P, int M>
SEED_WINDOW_FN uint32_t or_all(const uint32_t *x) {
    uint32_t r = x[0];
SEED_WINDOW_UNROLL
    for (int i = 1; i + 1 < M; i += 2) r = P::template bitop3<TT_OR3>(r, x[i], x[i + 1]);
    if (M % 2 == 0) r |= x[M - 1];
    return r;
}

// the M words x[0 ..) still to be counted and the NC carry words cy[0 ..) found so far -> two = "two or more of the inputs",
// one = "one or more"; x and cy are scratch (x: M words, cy: room for every carry of the network)
template <class P, int M, int NC>
SEED_WINDOW_FN void count2(uint32_t *x, uint32_t *cy, uint32_t &two, uint32_t &one) {
    if constexpr (M > 3) {
        constexpr int G = M / 3, REST = M % 3;
SEED_WINDOW_UNROLL
        for (int g = 0; g < G; g++) {
            const uint32_t a = x[3 * g], b = x[3 * g + 1], c = x[3 * g + 2];
            cy[NC + g] = P::template bitop3<TT_MAJ3>(a, b, c);
            x[g] = P::template bitop3<TT_XOR3>(a, b, c);
        }
SEED_WINDOW_UNROLL
        for (int j = 0; j < REST; j++) x[G + j] = x[3 * G + j];
        count2<P, G + REST, NC + G>(x, cy, two, one);
    } else if constexpr (M == 3) {
        cy[NC] = P::template bitop3<TT_MAJ3>(x[0], x[1], x[2]);
        two = or_all<P, NC + 1>(cy);
        one = two | P::template bitop3<TT_XOR3>(x[0], x[1], x[2]);
    } else if constexpr (M == 2) {
        if constexpr (NC > 0) {
            cy[NC - 1] = P::template bitop3<TT_A_OR_BC>(cy[NC - 1], x[0], x[1]);
            two = or_all<P, NC>(cy);
        } else {
            two = x[0] & x[1];
        }
        one = P::template bitop3<TT_OR3>(two, x[0], x[1]);
    } else {
        static_assert(M == 1, "at least one care position");
        if constexpr (NC > 0) two = or_all<P, NC>(cy);
        else two = 0u;
        one = two | x[0];
    }
}

// bit i = the window that starts at column BASE + i may be a seed hit (above).  n0 / n1: columns 0 .. 63 of the mismatch plane,
// d0 / d1: the same of the transversion plane (TV only); BASE + the highest care position <= 31.
template <class P, uint32_t CARE, bool TV, int BASE>
SEED_WINDOW_FN uint32_t starts32(uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, int transitions) {
    constexpr int K = popcount32(CARE);
    static_assert(K >= 1 && ((uint64_t)CARE >> (32 - BASE)) == 0u, "every shift stays inside the two words");
    uint32_t x[K], t[K + 1], cy[K];
    int k = 0;
SEED_WINDOW_UNROLL
    for (int c = 0; c + BASE < 32; c++) {
        if (!((CARE >> c) & 1u)) continue;
        x[k] = BASE + c ? P::funnel(n0, n1, BASE + c) : n0;
        t[k] = !TV ? 0u : (BASE + c ? P::funnel(d0, d1, BASE + c) : d0);
        k++;
    }
    uint32_t two, one;
    count2<P, K, 0>(x, cy, two, one);
    if (TV) {   // (no transitions: a transversion is a mismatch, `one` holds it already)
        t[K] = two;
        two = or_all<P, K + 1>(t);
    }
    return ~(transitions ? two : one);
}

}  // namespace seed_window
}  // namespace mimeo
