// k34_filter.h — the three frame predicates of K34 (k34_fused.hip): the cheap pre-filter of every pair (pair_needs_walk), the sharp
// filter at the first pass's walk-queue flush (pair_needs_walk_sharp) and the split pass's run test (run_interior).  Pure functions
// of two seed frames (three uint4 each, K2's layout) and the scoring parameters.
#pragma once
#include "k4_device.h"

namespace mimeo {

constexpr uint32_t CARE10 = 0x1A997u;  // offsets 0 1 2 4 7 8 11 13 15 16 of CARE19

// ---- pre-filter on two frames in the common alignment ------------------------------------------------------
// left walk = frame bits 127 .. 32 (four 24-step blocks), right walk = bits 128 .. 191 (24 + 24 + 16); the seed windows
// that END where left step s arrives start at bit 108 - s.  A pair is dismissed when (i) both walks provably stop
// inside the frame, (ii) no earlier seed hit of the diagonal can end at a boundary the left walk reaches before its
// proven stop, so the hit is a head, and (iii) an upper bound of best(left) + best(right) is below hspthresh: the exact
// walk would then find an isolated head that scores too little, and emit nothing.  Everything else goes to the batch's
// walk queue (k4_walk_queue: the exact walk).  The proofs use the CHEAP bounds — two popcounts per block: n =
// mismatching columns, v = transversions; a match scores 91..100, a transition -31, a transversion -125..-114 — and
// a seed test on ten of the twelve care positions without the transition rule: 4.1 % of random hits are walked
// instead of 1.4 % with the sharpest bounds, for half the instructions per pair (scripts/dev_filter_mc.py; the
// kernel is bound by VALU issue, and popcounts, funnel shifts, compares and max issue at half rate).
struct Bound2 {
    int32_t up, lomax, ub;   // upper bound of the prefix score; best lower bound at an earlier checkpoint; bound of the best prefix
    bool stop;
};
// one block of W columns: v = its transversion bits, n = its mismatch bits
template <int W>
__device__ __forceinline__ void bound_block2(Bound2 &B, uint32_t v, uint32_t n, int32_t &lo, int xdrop) {
    const int32_t pv = __popc(v), pn = __popc(n);
    B.ub = max(B.ub, B.up + 100 * W - 100 * pn);
    B.up += 100 * W - 131 * pn - 83 * pv;
    lo += 91 * W - 122 * pn - 94 * pv;
    B.stop = B.stop || (B.up + xdrop < B.lomax);
    B.lomax = max(B.lomax, lo);
}

// "a seed hit of this diagonal may start at frame bit B + i" for i = 0 .. 31 (bit i of the result), B = 13 + 32 k.
// n0 / n1: the words of nm = dl | dh that hold bits B - 13 .. B + 50; d0 / d1: the same of dl.  CARE = the care
// positions looked at (all twelve + TV: the exact 12of19 rule with one transition; fewer / no TV: a superset).  The count itself
// is seed_window.h's carry-save network: 12 three-input functions per CARE10 word, 20 per CARE19 word with the transversion plane.
template <uint32_t CARE, bool TV>
__device__ __forceinline__ uint32_t seed_starts32(uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, int transitions) {
    return seed_window::starts32<SeedOps, CARE, TV, 13>(n0, n1, d0, d1, transitions);
}

// true = the pair is walked exactly.  Blocks of 24 columns (left: four, right: 24 + 24 + 16): seven blocks instead of
// the ten 16-column ones pass 4.1 % of random hits on instead of 3.8 % (scripts/dev_filter_mc.py) for 15 % fewer
// instructions per pair.
__device__ __forceinline__ bool pair_needs_walk(const uint4 t0, const uint4 t1, const uint4 t2, const uint4 q0, const uint4 q1,
                                                const uint4 q2, int xdrop, int hspthresh, int transitions) {
    // planes: lo = {0.x 0.y 0.z 0.w 1.x 1.y}, hi = {1.z 1.w 2.x 2.y 2.z 2.w}
    const uint32_t dl0 = t0.x ^ q0.x, dl1 = t0.y ^ q0.y, dl2 = t0.z ^ q0.z, dl3 = t0.w ^ q0.w, dl4 = t1.x ^ q1.x, dl5 = t1.y ^ q1.y;
    const uint32_t n0 = dl0 | (t1.z ^ q1.z), n1 = dl1 | (t1.w ^ q1.w), n2 = dl2 | (t2.x ^ q2.x), n3 = dl3 | (t2.y ^ q2.y),
                   n4 = dl4 | (t2.z ^ q2.z), n5 = dl5 | (t2.w ^ q2.w);
    // earlier seed hits: starts 77..108 <-> left steps 31..0, 45..76 <-> steps 63..32, 13..44 <-> steps 95..64
    const uint32_t h0 = seed_starts32<CARE10, false>(n2, n3, 0u, 0u, transitions);   // bit 31 - s  <-> step s      (s = 0..31)
    const uint32_t h1 = seed_starts32<CARE10, false>(n1, n2, 0u, 0u, transitions);   // bit 63 - s  <-> step s      (s = 32..63)
    const uint32_t h2 = seed_starts32<CARE10, false>(n0, n1, 0u, 0u, transitions);   // bit 95 - s  <-> step s      (s = 64..95)
    Bound2 L{0, 0, 0, false}, R{0, 0, 0, false};
    int32_t llo = 0, rlo = 0;
    uint32_t veto;
    constexpr uint32_t M24 = 0xFFFFFFu;
    // left walk: columns 127 downwards; a boundary only counts while the walk is not yet proven to have stopped
    veto = h0 >> 8;                                                   // steps 0 .. 23
    bound_block2<24>(L, dl3 >> 8, n3 >> 8, llo, xdrop);                                                               // columns 104 .. 127
    veto |= L.stop ? 0u : ((h0 & 0xFFu) | (h1 >> 16));                // steps 24 .. 47
    bound_block2<24>(L, __builtin_amdgcn_alignbit(dl3, dl2, 16) & M24, __builtin_amdgcn_alignbit(n3, n2, 16) & M24, llo, xdrop);   // 80 .. 103
    veto |= L.stop ? 0u : ((h1 & 0xFFFFu) | (h2 >> 24));              // steps 48 .. 71
    bound_block2<24>(L, __builtin_amdgcn_alignbit(dl2, dl1, 24) & M24, __builtin_amdgcn_alignbit(n2, n1, 24) & M24, llo, xdrop);   // 56 .. 79
    veto |= L.stop ? 0u : (h2 & M24);                                 // steps 72 .. 95
    bound_block2<24>(L, dl1 & M24, n1 & M24, llo, xdrop);                                                              // 32 .. 55
    // right walk: columns 128 upwards
    bound_block2<24>(R, dl4 & M24, n4 & M24, rlo, xdrop);                                                              // 128 .. 151
    bound_block2<24>(R, __builtin_amdgcn_alignbit(dl5, dl4, 24) & M24, __builtin_amdgcn_alignbit(n5, n4, 24) & M24, rlo, xdrop);   // 152 .. 175
    bound_block2<16>(R, dl5 >> 16, n5 >> 16, rlo, xdrop);                                                              // 176 .. 191
    return !(L.stop && R.stop && L.ub + R.ub < hspthresh && veto == 0);
}

// The SHARP filter on two frames: the three proofs of hit_needs_walk<16> (k4_device.h) restated in frame coordinates, run by the
// first pass where it flushes a wavefront of staged pairs (k34_fused.hip: walk_flush) so that the walk-queue kernel neither gathers a
// neighbourhood nor shifts it for a pair that comes to nothing.  The 16-step blocks are half-words at compile-time
// positions — left steps 0 .. 79 = word 3, word 2 and the upper half of word 1 from bit 31 downwards, right steps
// 0 .. 63 = words 4 and 5 from bit 0 upwards — with the class-exact bounds of bound_window (transversions, transitions,
// C/G matches from dl, dh and the target's lo ^ hi).  The earlier-seed-hit test is the exact 12of19 rule with the
// transition plane on steps 0 .. 63, and on steps 64 .. 79 (word 0 holds their windows) unless the left stop was proven within 64
// steps: no seed-validity planes, so still a superset.  true = the pair is walked exactly.
__device__ __forceinline__ bool pair_needs_walk_sharp(const uint4 t0, const uint4 t1, const uint4 t2, const uint4 q0, const uint4 q1,
                                                      const uint4 q2, int xdrop, int hspthresh, int transitions) {
    // planes: lo = {0.x 0.y 0.z 0.w 1.x 1.y}, hi = {1.z 1.w 2.x 2.y 2.z 2.w}
    const uint32_t dl0 = t0.x ^ q0.x, dl1 = t0.y ^ q0.y, dl2 = t0.z ^ q0.z, dl3 = t0.w ^ q0.w, dl4 = t1.x ^ q1.x, dl5 = t1.y ^ q1.y;
    const uint32_t dh0 = t1.z ^ q1.z, dh1 = t1.w ^ q1.w, dh2 = t2.x ^ q2.x, dh3 = t2.y ^ q2.y, dh4 = t2.z ^ q2.z, dh5 = t2.w ^ q2.w;
    const uint32_t n0 = dl0 | dh0, n1 = dl1 | dh1, n2 = dl2 | dh2, n3 = dl3 | dh3;
    // earlier seed hits: starts 77..108 <-> left steps 31..0, 45..76 <-> steps 63..32, 29..44 <-> steps 79..64 (bits 31..16 of h2)
    const uint32_t h0 = seed_starts32<CARE19, true>(n2, n3, dl2, dl3, transitions);
    const uint32_t h1 = seed_starts32<CARE19, true>(n1, n2, dl1, dl2, transitions);
    const uint32_t h2 = seed_starts32<CARE19, true>(n0, n1, dl0, dl1, transitions) & 0xFFFF0000u;
    Bound L{0, 0, 0, 0, false}, R{0, 0, 0, 0, false};
    bound_window<16, true>(L, dl3, dh3, t0.w ^ t2.y, xdrop);      // left steps 0 .. 31
    bound_window<16, true>(L, dl2, dh2, t0.z ^ t2.x, xdrop);      // 32 .. 63
    const bool stop64 = L.stop;
    bound_window<16, true, 1>(L, dl1, dh1, t0.y ^ t1.w, xdrop);   // 64 .. 79: their boundaries only matter when no stop was proven before
    bound_window<16, false>(R, dl4, dh4, t1.x ^ t2.z, xdrop);     // right steps 0 .. 31
    bound_window<16, false>(R, dl5, dh5, t1.y ^ t2.w, xdrop);     // 32 .. 63
    const uint32_t veto = h0 | h1 | (stop64 ? 0u : h2);
    return !(L.stop && R.stop && L.ub + R.ub < hspthresh && veto == 0);
}

// Split pass only (the tiles microsatellites and high-copy repeats fill): is this pair an INTERIOR member of a run of consecutive
// seed hits of its diagonal — exact seed hits one and two positions back and one ahead (k4_device.h, "runs of consecutive seed
// hits")?  Such a hit leaves no record anywhere, so it is dropped here, before the pre-filter and the walk queue.  The three
// 19-windows start at frame bits 107, 108 and 110 (the hit's own at 109): words 3 and 4 of the planes.  Exact for frames
// without N of a unit whose target has no soft-masked bases, with the windows inside both scaffolds (the caller checks):
// the same predicate seed_hit_at() evaluates on the planes for the members that do reach the walk kernel.
__device__ __forceinline__ bool run_interior(const uint4 t0, const uint4 t1, const uint4 t2, const uint4 q0, const uint4 q1, const uint4 q2,
                                             int transitions) {
    // planes: lo = {0.x 0.y 0.z 0.w 1.x 1.y}, hi = {1.z 1.w 2.x 2.y 2.z 2.w}
    const uint32_t dl3 = t0.w ^ q0.w, dl4 = t1.x ^ q1.x;
    const uint32_t n3 = dl3 | (t2.y ^ q2.y), n4 = dl4 | (t2.z ^ q2.z);
    bool all = true;
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int off = k == 0 ? 11 : (k == 1 ? 12 : 14);   // frame bit of the window start - 96
        const uint32_t wn = __builtin_amdgcn_alignbit(n4, n3, off) & CARE19, wd = __builtin_amdgcn_alignbit(dl4, dl3, off) & CARE19;
        all = all && (transitions ? (wd == 0u && __popc(wn) <= 1) : (wn == 0u));
    }
    return all;
}

}  // namespace mimeo
