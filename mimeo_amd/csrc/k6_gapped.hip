// K6 — lastz `--gapped` (reference call site src/mimeo/wrappers.py:1031):
// every chained HSP becomes an anchor (centre of its best 31-column window); anchors are taken
// by decreasing HSP score, an anchor that lies inside the box of an earlier alignment is
// skipped, every other anchor is extended in both directions by a y-drop affine-gap DP
// (gap open 400 / extend 30, y-drop 9400) and the two halves are joined.
//
// Decomposition:
//   * a half extension is one JOB.  The DP is evaluated row by row; pruning: a cell scoring below
//     (best of the rows above) - ydrop is dead.  Cells carry (score, matches, mismatches), so
//     identity needs no traceback.  Inside a row the only horizontal dependency is the insertion
//     state, a max-plus prefix scan along the row (in-lane over a strip, then one cross-lane scan).
//     Three kernels (k6_dp.hip), each taking the jobs the one before could not hold (dp_round):
//       - k6_dp1, the lean kernel: one wavefront, lane l owns the 14-column strip (j / 14) % 64 == l
//         of an 896-column window that slides with the first live column, all state in registers,
//         counts packed into 16 bits each (65 535 rows at most); a half starts at 7-column strips (448
//         columns) and moves to 14 when its band reaches the last strip but one (k6_dp.hip);
//       - k6_dp_wide, the second chance: the same layout with 32-column strips (2048 columns),
//         unpacked counts and no row limit;
//       - k6_dp_any, the last resort: one workgroup, the rows in global memory, bands up to 2^16
//         columns, cells rebased when the score nears 2^31.
//   * exact shortcut (identical_suffix): if the two sequences are identical and N-free from the
//     anchor to the end of the shorter one, the diagonal is optimal (every column already scores its
//     maximum) and the DP is skipped — this is what makes the trivial (A,A) self alignment cheap.
//   * jobs of different anchors are independent, only the skip rule is ordered: each round takes
//     the next unskipped anchors of every group, up to the take (k6_pick), extends them all (dp_round),
//     then replays the skip rule in order over the batch (k6_resolve).  Every accepted alignment needs
//     its DP, so a group ends in one round only if the take exceeds what it accepts: the take is the
//     round's budget of K6_ROUND_ANCHORS over the groups, at most MAX_BATCH = 128 (a C4 group accepts
//     ~30, at most 39 in a measured row; a C5MID group ~57, at most 72), and k6_pick's window of PICK_SCAN
//     ranks is longer than their chains.  Anchors near a pending one wait (fragments of one
//     copy), and past its first 32 of a round a group takes no anchor on a band of diagonals that several
//     pending ones share (the HSPs of one long collinear alignment): scheduling only, results do not depend on it.
//   * path rule (mimeo_params.anchor_rule = MIMEO_ANCHOR_PATH, opt-in): an anchor is skipped iff it is a diagonal step of
//     the path of an earlier alignment.  After a round's DP kernels k6_trace (k6_trace.hip) re-runs the round's halves with a traceback,
//     checks them against the first run and leaves each path as gap-free blocks; k6_pick / k6_resolve<true> test the
//     blocks of the alignments whose box holds the anchor.  The box-rule kernels are unchanged.
//   * bounded extensions (mimeo_params.bound_extensions = 1, opt-in, path rule only; parity unpinned): a DP cell on or beyond the
//     nearest earlier path on either side of the anchor's diagonal is dead (alignment specification v1, rule 7; the specification is
//     tests/bounded_oracle.c).  k6_dp1_bounded / k6_dp_any<true> / k6_trace<true> look the bounds up row range by row range
//     (bounds_at); k6_resolve<true, true> sends an anchor back when an alignment accepted after its DP ran reaches into what it swept.
//   * paths out (mimeo_align_units_paths, under every rule; a call that does not ask launches what it launched before): the blocks of
//     the two halves of every returned alignment, merged at the anchor, in the dense order of k6_dense_copy (k6_path_count, a
//     scan, k6_path_write; k6_paths.hip).  Under the box rule one trace pass after the last round makes the blocks (paths_pass).
//   * the two workgroup kernels, k6_dp_any and k6_trace, are ONE band DP (band_dp, k6_band.h): the row loop is written once and computes scores and decisions;
//     k6_dp_any's payload carries match / mismatch counts, k6_trace's writes traceback bytes.  The path rule, the bounded rule and the paths out need them to agree.
// This file: anchors, the ordered skip rule (k6_pick, k6_resolve), the finishing kernels, the host driver.  k6.h: what the files share.
#include "k6.h"

namespace mimeo {

// Anchor = centre of the best 31-column window of the HSP (first maximum).  Windows are cut into
// chunks of ANCHOR_CHUNK starts; a wave scans one chunk (each lane slides over 64 consecutive
// starts) and folds its best (sum, start) into a packed 64-bit word with atomicMax — high half
// = biased sum, low half = ~start, so the maximum is the highest sum at the smallest start.
constexpr uint32_t ANCHOR_W = 31, ANCHOR_CHUNK = 4096;
constexpr int ANCHOR_THREADS = 1024;

__device__ void wave_anchor_chunk(const GStrandView &T, const GStrandView &Q, const mimeo_hsp &h, uint32_t chunk,
                                  unsigned long long *packed) {
    const uint32_t lane = threadIdx.x & 63u, nw = h.length - ANCHOR_W + 1;
    const int32_t d = (int32_t)h.tstart - (int32_t)h.qstart;
    const uint32_t w0 = chunk * ANCHOR_CHUNK + lane * (ANCHOR_CHUNK / 64u), w1 = min(nw, w0 + ANCHOR_CHUNK / 64u);
    int32_t bs = INT32_MIN;
    uint32_t bw = 0xFFFFFFFFu;
    if (w0 < w1) {
        int32_t sum = 0;
        bool m;
        for (uint32_t k = 0; k < ANCHOR_W; k++) {
            int32_t pt = (int32_t)(h.tstart + w0 + k);
            sum += pair_score(T, Q, pt, pt - d, &m);
        }
        bs = sum; bw = w0;
        for (uint32_t w = w0 + 1; w < w1; w++) {
            int32_t add = (int32_t)(h.tstart + w + ANCHOR_W - 1), sub = (int32_t)(h.tstart + w - 1);
            sum += pair_score(T, Q, add, add - d, &m) - pair_score(T, Q, sub, sub - d, &m);
            if (sum > bs) { bs = sum; bw = w; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        int32_t ob = __shfl_xor(bs, o);
        uint32_t ow = __shfl_xor(bw, o);
        if (ob > bs || (ob == bs && ow < bw)) { bs = ob; bw = ow; }
    }
    if (lane == 0 && bw != 0xFFFFFFFFu)
        atomicMax(packed, ((unsigned long long)(uint32_t)(bs + 8192) << 32) | (unsigned long long)(0xFFFFFFFFu - bw));
}

// packed[b0 + r] = best window of the r-th chained HSP of the group.  ANCHOR_SPLIT workgroups of 16
// wavefronts share the (HSP, chunk) items of a group round-robin (the 5 Mbp self HSP alone has 1220
// chunks); k6_anchor_final turns the packed maxima into anchor points.
constexpr uint32_t ANCHOR_SPLIT = 16;
__global__ __launch_bounds__(ANCHOR_THREADS) void k6_anchor_points(const Group *__restrict__ groups,
                                                                   const mimeo_hsp *__restrict__ hs,
                                                                   const uint32_t *__restrict__ order,
                                                                   unsigned long long *__restrict__ packed) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nw = gridDim.y * (ANCHOR_THREADS / 64), me = blockIdx.y * (ANCHOR_THREADS / 64) + (threadIdx.x >> 6);
    uint32_t item = 0;
    for (uint32_t r = 0; r < G.nchain; r++) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        if (h.length <= ANCHOR_W) continue;
        const uint32_t nch = (h.length - ANCHOR_W + 1 + ANCHOR_CHUNK - 1) / ANCHOR_CHUNK;
        // my chunks of this HSP: c = first, first + nw, ...
        const uint32_t first = (me + nw - item % nw) % nw;
        for (uint32_t c = first; c < nch; c += nw) wave_anchor_chunk(G.T, G.Q, h, c, &packed[b0 + r]);
        item += nch;
    }
}
__global__ __launch_bounds__(256) void k6_anchor_final(const Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs,
                                                       const uint32_t *__restrict__ order,
                                                       const unsigned long long *__restrict__ packed,
                                                       uint2 *__restrict__ anchors) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    for (uint32_t r = threadIdx.x; r < G.nchain; r += blockDim.x) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        uint32_t off = h.length / 2;
        if (h.length > ANCHOR_W) off = (0xFFFFFFFFu - (uint32_t)packed[b0 + r]) + ANCHOR_W / 2;
        anchors[b0 + r] = make_uint2(h.tstart + off, h.qstart + off);
    }
}

__device__ __forceinline__ bool in_boxes(const mimeo_alignment *aln, uint32_t n, uint2 a) {
    // wave-cooperative: is the anchor inside the box of any of the n earlier alignments?
    bool inside = false;
    for (uint32_t e = threadIdx.x & 63u; e < n; e += 64u) {
        const mimeo_alignment &o = aln[e];
        if (a.x >= o.tstart && a.x < o.tend && a.y >= o.qstart && a.y < o.qend) inside = true;
    }
    return __ballot(inside) != 0;
}

// ---- path rule (MIMEO_ANCHOR_PATH) ------------------------------------------------------------------------------
// The path of an alignment = its diagonal (match / mismatch) steps from both halves, kept as gap-free blocks (t, q, len)
// sorted by t.  A half's diagonal steps have distinct t (each consumes one target base) and the left half lies below the
// anchor's t, the right half at or above it, so one binary search per half decides whether (t, q) is on the path.
__device__ __forceinline__ bool on_half_path(const PathBlock *blk, uint32_t n, uint2 a) {
    const uint32_t lo = blocks_upto(blk, n, a.x);
    if (!lo) return false;
    const PathBlock b = blk[lo - 1];
    return a.x - b.t < b.len && a.y >= b.q && a.y - b.q == a.x - b.t;
}
// is anchor a on the path of the alignment of the anchor of rank `rank` (group hsp_begin b0)?
__device__ __forceinline__ bool on_path(const PathView &P, const uint2 *anchors, uint64_t b0, uint32_t rank, uint2 a) {
    const uint2 an = anchors[b0 + rank];
    const uint2 ix = P.pidx[2u * (b0 + rank) + (a.x >= an.x ? 1u : 0u)];
    if (ix.x == PATH_UNTRACED) return false;
    return on_half_path(P.blk + ix.x, ix.y, a);
}
// the skip test of the rule in force against the n accepted alignments aln[b0 ..]: the box is a prefilter of the path
template <bool PATH>
__device__ __forceinline__ bool skip_test(const mimeo_alignment *aln, uint32_t n, uint2 a, const PathView &P,
                                          const uint2 *anchors, uint64_t b0) {
    if (!PATH) return in_boxes(aln + b0, n, a);
    bool on = false;
    for (uint32_t e = threadIdx.x & 63u; e < n; e += 64u) {
        const mimeo_alignment &o = aln[b0 + e];
        if (a.x >= o.tstart && a.x < o.tend && a.y >= o.qstart && a.y < o.qend && on_path(P, anchors, b0, P.accrank[b0 + e], a))
            on = true;
    }
    return __ballot(on) != 0;
}

// Anchor states.  The skip rule is ordered (an anchor is skipped iff it lies in the box of an ACCEPTED
// anchor of lower rank), so anchors are finalised strictly in rank order by k6_resolve; what k6_pick
// may choose freely is which unfinalised anchors get their DP in this round.  Fragments of one repeat
// copy sit on neighbouring diagonals within a few kb and only the best-ranked one survives, so an
// anchor that is NEAR a lower-ranked anchor whose DP is pending is deferred (twice at most): in the
// next round it is normally inside that anchor's accepted box and never costs a DP.
enum : uint8_t { A_NEW = 0, A_DONE = 1, A_SKIPPED = 2, A_ACCEPTED = 3 };
// ranks looked at per round, from the first unfinalised one: one wavefront walks them in turn, so a group of 10^6 anchors must not be
// walked whole every round.  Whatever lies beyond the window costs a round of its own: the groups of a C4 row chain 480 HSPs on
// average and up to 628 (C5MID: up to 596) and accept anchors of rank 512 and beyond (4 in a C4 row, 31 in C5MID)
constexpr uint32_t PICK_SCAN = 2048;
constexpr uint32_t NEAR_DIAG = 256, NEAR_POS = 8192, MAX_DEFER = 2;
// The take of a round (bmax) is sized so that a group of unrelated repeat copies finishes in ONE round.  What the near test does not
// see are the far-apart HSPs of one long collinear alignment (synteny, a self pair): every one of them scheduled runs the whole long
// DP and is swallowed afterwards.  The first GUARD_FREE anchors a group schedules in a round are taken as ever; a further one waits
// when GUARD_COUNT or more pending or scheduled anchors of the group lie within GUARD_DIAG diagonals of its own, at any distance.
// A count, not one neighbour: the chained HSPs of unrelated copies are collinear too, and in a C4 row one in ten of the anchors past
// a group's 32nd has ONE scheduled anchor within 4096 diagonals (none has three), while a collinear alignment puts most of the 32
// there.  A band with fewer members than the count costs at most that many DPs more.  A round still schedules a group's first
// GUARD_FREE free anchors, so the guard keeps no count of waits (MAX_DEFER bounds the near deferral only).
constexpr uint32_t GUARD_FREE = 32, GUARD_DIAG = 4096, GUARD_COUNT = 4;

// bit 0: b is near a (a fragment of the same repeat copy); bit 1: b's diagonal is within the guard's band of a's
__device__ __forceinline__ uint32_t anchor_relation(uint2 a, uint2 b) {
    int32_t da = (int32_t)a.x - (int32_t)a.y, db = (int32_t)b.x - (int32_t)b.y;
    uint32_t dd = (uint32_t)abs(da - db), dp = a.x > b.x ? a.x - b.x : b.x - a.x;
    return ((dd <= NEAR_DIAG && dp <= NEAR_POS) ? 1u : 0u) | (dd <= GUARD_DIAG ? 2u : 0u);
}

// one wave per group; PATH: the skip test is the path rule (P is unused otherwise)
template <bool PATH>
__global__ __launch_bounds__(64) void k6_pick(Group *__restrict__ groups, const uint2 *__restrict__ anchors,
                                              const mimeo_alignment *__restrict__ aln, uint32_t bmax,
                                              uint8_t *__restrict__ astate, uint8_t *__restrict__ adefer,
                                              DpJob *__restrict__ jobs, unsigned int *__restrict__ njobs, PathView P) {
    __shared__ uint32_t sb[MAX_BATCH];  // ranks scheduled in this round
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t first = G.next, lane = threadIdx.x;
    uint32_t nb = 0;
    for (uint32_t r = first; r < G.nchain && nb < bmax && r - first < PICK_SCAN; r++) {
        if (astate[b0 + r] != A_NEW) continue;  // wave-uniform; states of earlier rounds only
        const uint2 a = anchors[b0 + r];
        if (skip_test<PATH>(aln, G.nacc, a, P, anchors, b0)) {
            if (lane == 0) astate[b0 + r] = A_SKIPPED;
            continue;
        }
        // near an unfinalised lower-ranked anchor whose DP is done (earlier rounds) or scheduled (this round)?
        uint32_t near = 0, band = 0;   // per lane: any near one, how many within the guard's band
        for (uint32_t r2 = first + lane; r2 < r; r2 += 64)
            if (astate[b0 + r2] == A_DONE) { const uint32_t x = anchor_relation(a, anchors[b0 + r2]); near |= x & 1u; band += x >> 1; }
        for (uint32_t k = lane; k < nb; k += 64) { const uint32_t x = anchor_relation(a, anchors[b0 + sb[k]]); near |= x & 1u; band += x >> 1; }
        if (__ballot(near) && adefer[b0 + r] < MAX_DEFER) {
            if (lane == 0) adefer[b0 + r]++;
            continue;
        }
        if (nb >= GUARD_FREE) {   // the guard: a later round takes it, if it is not swallowed by then
            for (int o = 32; o > 0; o >>= 1) band += __shfl_xor(band, o);
            if (band >= GUARD_COUNT) continue;
        }
        if (lane == 0) sb[nb] = r;
        nb++;
        __syncthreads();
    }
    if (lane == 0) {
        G.nbatch = nb;
        unsigned int j0 = nb ? atomicAdd(njobs, 2u * nb) : 0u;
        G.job0 = j0;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t r = sb[k];
            astate[b0 + r] = A_DONE;
            const uint2 a = anchors[b0 + r];
            const uint32_t slot = 2u * (uint32_t)(b0 + r);
            jobs[j0 + 2 * k] = DpJob{blockIdx.x, a.x, a.y, -1, slot, 0};
            jobs[j0 + 2 * k + 1] = DpJob{blockIdx.x, a.x, a.y, +1, slot + 1, 0};
        }
    }
}

// one wave per group: finalise anchors in rank order as far as DP results exist
constexpr uint32_t RESOLVE_NEW = 256;  // boxes accepted per invocation that fit the LDS list
// a round's take fits one invocation; with anchors left pending by earlier rounds an invocation may stop at the list's end, and the
// next round (possibly one without jobs) goes on from there
static_assert(RESOLVE_NEW >= (uint32_t)MAX_BATCH, "k6_resolve accepts a full take in one invocation");

// bounded extensions: does the alignment of the anchor of rank `rank` (box o: tstart, tend, qstart, qend) put a bound
// into the cells that the halves L / R of anchor a looked at?  Yes iff one of its blocks covers an evaluated row of a half
// and its diagonal lies within the k that half swept.  Wave-cooperative (lanes over the blocks).
__device__ __forceinline__ bool bounds_touch(const PathView &P, const uint2 *anchors, uint64_t b0, uint32_t rank, uint4 o, uint2 a,
                                             const HalfResult &L, const HalfResult &R, const HalfSweep &sL, const HalfSweep &sR) {
    const uint32_t rowsL = L.rows ? L.rows : L.i, rowsR = R.rows ? R.rows : R.i;   // rows == 0, i > 0: the shortcut's diagonal
    const long long tlo = (long long)a.x - rowsL, thi = (long long)a.x + rowsR;    // target bases the two halves consumed
    if ((long long)o.y <= tlo || (long long)o.x >= thi) return false;
    const long long d0 = (long long)a.y - (long long)a.x;
    bool hit = false;
    for (uint32_t side = 0; side < 2; side++) {
        const uint2 ix = P.pidx[2u * (b0 + rank) + side];
        if (ix.x == PATH_UNTRACED) continue;
        for (uint32_t k = threadIdx.x & 63u; k < ix.y; k += 64u) {
            const PathBlock b = P.blk[ix.x + k];
            const long long t0 = b.t, t1 = (long long)b.t + b.len, d = (long long)b.q - (long long)b.t;
            if (t0 < thi && t1 > (long long)a.x && d - d0 >= sR.klo && d - d0 <= sR.khi) hit = true;
            if (t0 < (long long)a.x && t1 > tlo && d0 - d >= sL.klo && d0 - d <= sL.khi) hit = true;
        }
    }
    return __ballot(hit) != 0;
}

// BOUND (mimeo_params.bound_extensions, with PATH): the rule is sequential — rank r is bounded by everything accepted
// below r — but a round's DPs ran against the alignments accepted when the round began (HalfSweep.nacc).  Before rank r
// is accepted, every alignment accepted since is tested against what r's halves swept (bounds_touch); if one touches,
// the result is stale: the anchor goes back to A_NEW and the group's resolve stops there, so the next round runs it
// again as the group's lowest unfinalised anchor, which is always bounded by exactly the alignments below it.
// RANK (box rule, paths asked for): the rank of every accepted anchor is recorded as under the path rule (k6_kept_jobs).
template <bool PATH, bool BOUND = false, bool RANK = false>
__global__ __launch_bounds__(64) void k6_resolve(Group *__restrict__ groups, const uint2 *__restrict__ anchors,
                                                 const HalfResult *__restrict__ res, mimeo_alignment *__restrict__ aln,
                                                 uint8_t *__restrict__ astate, unsigned int *__restrict__ remaining, PathView P,
                                                 const HalfSweep *__restrict__ sweep) {
    __shared__ uint4 sbox[RESOLVE_NEW];  // boxes accepted in this invocation (tstart, tend, qstart, qend)
    __shared__ uint32_t srank[PATH ? RESOLVE_NEW : 1];  // ... and the ranks of their anchors (path rule)
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nacc0 = G.nacc;
    uint32_t nnew = 0, overflow = 0, r = G.next;
    for (; r < G.nchain; r++) {
        const uint8_t st = astate[b0 + r];
        if (st == A_SKIPPED || st == A_ACCEPTED) continue;
        if (nnew == RESOLVE_NEW) break;
        const uint2 a = anchors[b0 + r];
        bool inside = skip_test<PATH>(aln, nacc0, a, P, anchors, b0);  // alignments of earlier invocations (global memory)
        if (!inside) {
            bool in2 = false;
            for (uint32_t e = threadIdx.x; e < nnew; e += 64) {
                uint4 o = sbox[e];
                if (a.x >= o.x && a.x < o.y && a.y >= o.z && a.y < o.w && (!PATH || on_path(P, anchors, b0, srank[PATH ? e : 0], a)))
                    in2 = true;
            }
            inside = __ballot(in2) != 0;
        }
        if (inside) {  // also for an anchor without DP result: a deferred anchor swallowed by now never needs one
            if (threadIdx.x == 0) astate[b0 + r] = A_SKIPPED;
            continue;
        }
        if (st == A_NEW) break;  // not swallowed and no DP result yet: it is scheduled in the next round
        const uint32_t slot = 2u * (uint32_t)(b0 + r);
        HalfResult L = res[slot], R = res[slot + 1];
        if (BOUND && !(L.overflow | R.overflow)) {
            const HalfSweep sL = sweep[slot], sR = sweep[slot + 1];
            bool stale = false;
            for (uint32_t e = sL.nacc; e < nacc0 && !stale; e++) {
                const mimeo_alignment &o = aln[b0 + e];
                stale = bounds_touch(P, anchors, b0, P.accrank[b0 + e], make_uint4(o.tstart, o.tend, o.qstart, o.qend), a, L, R, sL, sR);
            }
            for (uint32_t e = 0; e < nnew && !stale; e++)
                stale = bounds_touch(P, anchors, b0, srank[PATH ? e : 0], sbox[e], a, L, R, sL, sR);
            if (stale) {
                if (threadIdx.x == 0) { astate[b0 + r] = A_NEW; atomicAdd(remaining + 2, 1u); }
                break;
            }
        }
        overflow |= L.overflow | R.overflow;
        // path rule: a half without a traceback (larger than the trace pool) fails the group like a band beyond the limit
        if (PATH && (P.pidx[slot].x == PATH_UNTRACED || P.pidx[slot + 1].x == PATH_UNTRACED)) overflow = 1;
        if (threadIdx.x == 0) {
            mimeo_alignment m;
            m.tid = G.tid; m.qid = G.qid; m.qstrand = G.minus; m.reserved = 0;
            m.tstart = a.x - L.i; m.tend = a.x + R.i; m.qstart = a.y - L.j; m.qend = a.y + R.j;
            m.score = half_score(L) + half_score(R);
            m.id_n = L.nm + R.nm;
            m.id_d = L.nm + R.nm + L.nx + R.nx;
            aln[b0 + nacc0 + nnew] = m;
            sbox[nnew] = make_uint4(m.tstart, m.tend, m.qstart, m.qend);
            if (PATH) srank[PATH ? nnew : 0] = r;
            if (PATH || RANK) P.accrank[b0 + nacc0 + nnew] = r;
            astate[b0 + r] = A_ACCEPTED;
        }
        nnew++;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        G.next = r;
        G.nacc = nacc0 + nnew;
        G.nbatch = 0;
        if (overflow) G.overflow = 1;
        if (r < G.nchain) atomicAdd(remaining, 1u);
    }
}

// gap-free mode (--gapped off): every chained HSP is reported as is; identity by popcount
__global__ __launch_bounds__(256) void k6_ungapped(Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs,
                                                   const uint32_t *__restrict__ order, mimeo_alignment *__restrict__ aln) {
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = threadIdx.x >> 6; r < G.nchain; r += 4) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        const int32_t d = (int32_t)h.tstart - (int32_t)h.qstart;
        uint32_t nmatch = 0;
        for (uint32_t w0 = lane * 32u; w0 < h.length; w0 += 64u * 32u) {
            int32_t pt = (int32_t)(h.tstart + w0), pq = pt - d;
            const Win32 tw = win32(G.T, pt), qw = win32(G.Q, pq);
            uint32_t mm = ~((tw.lo ^ qw.lo) | (tw.hi ^ qw.hi)) & ~(tw.nm | qw.nm);
            uint32_t rem = h.length - w0;
            if (rem < 32) mm &= (1u << rem) - 1u;
            nmatch += __popc(mm);
        }
        for (int o = 32; o > 0; o >>= 1) nmatch += __shfl_xor(nmatch, o);
        if (lane == 0) {
            mimeo_alignment m;
            m.tid = G.tid; m.qid = G.qid; m.qstrand = G.minus; m.reserved = 0;
            m.tstart = h.tstart; m.tend = h.tstart + h.length; m.qstart = h.qstart; m.qend = h.qstart + h.length;
            m.score = h.score; m.id_n = nmatch; m.id_d = h.length;
            aln[b0 + r] = m;
        }
    }
    if (threadIdx.x == 0) G.nacc = G.nchain;
}

// threshold, minus-strand coordinates -> query plus strand (start2+/end2+), compaction
__global__ void k6_finish(Group *__restrict__ groups, uint32_t ngroups, mimeo_alignment *__restrict__ aln,
                          int32_t thresh) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    Group &G = groups[g];
    const uint64_t b0 = G.hsp_begin;
    uint32_t k = 0;
    for (uint32_t e = 0; e < G.nacc; e++) {
        mimeo_alignment a = aln[b0 + e];
        if (a.score < thresh) continue;
        if (G.minus) { uint32_t s = G.Q.len - a.qend, t2 = G.Q.len - a.qstart; a.qstart = s; a.qend = t2; }
        aln[b0 + k++] = a;
    }
    G.naln = k;
}

// The alignments of group g sit at d_aln[hsp_begin .. hsp_begin + naln): a few thousand records scattered over an array of
// one slot per HSP (70 MB on a C4 row).  Packed densely before the read-back: job0 = the group's first dense slot.
__global__ __launch_bounds__(1024) void k6_dense_offsets(Group *__restrict__ groups, uint32_t ngroups) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t g0 = 0; g0 < ngroups; g0 += 1024) {
        const uint32_t g = g0 + threadIdx.x, n = g < ngroups ? groups[g].naln : 0u;
        part[threadIdx.x] = n;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {
            const uint32_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        if (g < ngroups) groups[g].job0 = carry + part[threadIdx.x] - n;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void k6_dense_copy(const Group *__restrict__ groups, const mimeo_alignment *__restrict__ aln,
                                                    mimeo_alignment *__restrict__ dense) {
    const Group &G = groups[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < G.naln; k += 64) dense[G.job0 + k] = aln[G.hsp_begin + k];
}
void dense_alignments_device(Group *d_groups, uint32_t ngroups, const mimeo_alignment *d_aln, mimeo_alignment *d_dense) {
    hipLaunchKernelGGL(k6_dense_offsets, dim3(1), dim3(1024), 0, stream(), d_groups, ngroups);
    hipLaunchKernelGGL(k6_dense_copy, dim3(ngroups), dim3(64), 0, stream(), (const Group *)d_groups, d_aln, d_dense);
}

// before k6_finish: accrank[hsp_begin + k] = anchor rank of the k-th alignment that k6_finish keeps; a kept alignment with a
// half whose traceback did not fit the trace pool fails its group (what k6_resolve<true> does under the path rule)
__global__ void k6_kept_ranks(Group *__restrict__ groups, uint32_t ngroups, const mimeo_alignment *__restrict__ aln,
                              uint32_t *__restrict__ accrank, const uint2 *__restrict__ pidx, int32_t thresh) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    Group &G = groups[g];
    const uint64_t b0 = G.hsp_begin;
    uint32_t k = 0;
    for (uint32_t e = 0; e < G.nacc; e++) {
        if (aln[b0 + e].score < thresh) continue;
        const uint32_t rank = accrank[b0 + e];
        const uint32_t slot = 2u * (uint32_t)(b0 + rank);
        if (pidx[slot].x == PATH_UNTRACED || pidx[slot + 1].x == PATH_UNTRACED) G.overflow = 1;
        accrank[b0 + k++] = rank;   // k <= e
    }
}

// gap-free mode, after k6_ungapped: alignment r of a group is one block, kept as the left half of "anchor" r
__global__ __launch_bounds__(256) void k6_ungapped_paths(const Group *__restrict__ groups, const mimeo_alignment *__restrict__ aln,
                                                         PathBlock *__restrict__ arena, uint2 *__restrict__ pidx,
                                                         uint32_t *__restrict__ accrank) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    for (uint32_t r = threadIdx.x; r < G.nacc; r += 256) {
        const mimeo_alignment a = aln[b0 + r];
        arena[b0 + r] = PathBlock{a.tstart, a.qstart, a.tend - a.tstart};
        pidx[2u * (b0 + r)] = make_uint2((uint32_t)(b0 + r), 1u);
        pidx[2u * (b0 + r) + 1u] = make_uint2(0u, 0u);
        accrank[b0 + r] = r;
    }
}

K6Buffers g_k6;

// MIMEO_K6_STATS: what the DP kernels made of the round's n jobs, on stderr; bounded mode: *bound_jobs counts those that met a bound
static int round_stats(uint32_t n, uint64_t nhsps, bool bounded, unsigned long long *bound_jobs, const unsigned int *nrestart) {
    std::vector<DpJob> hj(n);
    std::vector<HalfResult> hall((size_t)nhsps * 2), hr(n);
    HIP_TRY(hipStreamSynchronize(stream()));
    HIP_TRY(hipMemcpy(hj.data(), g_k6.jobs.p, (size_t)n * sizeof(DpJob), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hall.data(), g_k6.res.p, hall.size() * sizeof(HalfResult), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < hr.size(); k++) hr[k] = hall[hj[k].slot];
    unsigned long long hist[9] = {0}, rows = 0, maxr = 0, shortcut = 0;
    for (auto &r : hr) {
        if (!r.rows) { shortcut++; continue; }
        hist[std::min<uint32_t>(8, r.maxcols / 128)]++; rows += r.rows; maxr = std::max<unsigned long long>(maxr, r.rows);
    }
    unsigned long long rebased = 0;
    for (auto &r : hr) if (r.base_lo | r.base_hi) rebased++;
    unsigned int wide[2] = {0, 0};   // k6_dp1: halves whose band outgrew the first, narrower window: run again at the full width, gone on at it
    HIP_TRY(hipMemcpy(wide, nrestart, 8, hipMemcpyDeviceToHost));
    fprintf(stderr, "[k6] full strip width: restarted %u widened %u of %u\n", wide[0], wide[1], n);
    fprintf(stderr, "[k6] jobs %u shortcut %llu (rebased in k6_dp_any: %llu) rows total %llu max %llu band<128..>=1024:", n, shortcut, rebased, rows, maxr);
    for (int b = 0; b < 9; b++) fprintf(stderr, " %llu", hist[b]);
    fprintf(stderr, "\n");
    {
        unsigned long long fine[34] = {0};
        for (auto &r : hr) if (r.rows) fine[std::min<uint32_t>(33, r.maxcols / 32)]++;
        fprintf(stderr, "[k6] widest band, buckets of 32 columns from 448:");
        for (int b = 14; b < 34; b++) fprintf(stderr, " %llu", fine[b]);
        fprintf(stderr, "\n");
    }
    // a round of a few jobs: what each half came back with, in job order — the band width tells the kernel that finished it (a
    // multiple of 14 up to 882: k6_dp1; of 32 up to 2016: k6_dp_wide; the exact width: k6_dp_any)
    if (n <= 8)
        for (size_t k = 0; k < hr.size(); k++)
            fprintf(stderr, "  [k6] job %zu: dir %d rows %u maxcols %u i %u j %u rebased %d\n", k, hj[k].dir, hr[k].rows, hr[k].maxcols, hr[k].i, hr[k].j,
                    (hr[k].base_lo | hr[k].base_hi) ? 1 : 0);
    int shown = 0;
    for (auto &r : hr)
        if (!r.rows && shown < 8) { fprintf(stderr, "  [k6] zero-row job: score %d i %u j %u nm %u nx %u ovf %u\n", r.score, r.i, r.j, r.nm, r.nx, r.overflow); shown++; }
    if (bounded) {
        std::vector<HalfSweep> hs((size_t)nhsps * 2);
        HIP_TRY(hipMemcpy(hs.data(), g_k6.sweep.p, hs.size() * sizeof(HalfSweep), hipMemcpyDeviceToHost));
        for (auto &j : hj) *bound_jobs += hs[j.slot].nbound ? 1u : 0u;
    }
    return 0;
}

// MIMEO_K6_STATS, after the last round: alignments accepted per group, which is what sizes MAX_BATCH (every accepted alignment needs its DP,
// so a group that accepts more than the take cannot finish in one round)
static int accepted_stats(const Group *d_groups, uint32_t ngroups, uint32_t bmax) {
    std::vector<Group> hg(ngroups);
    HIP_TRY(hipStreamSynchronize(stream()));
    HIP_TRY(hipMemcpy(hg.data(), d_groups, (size_t)ngroups * sizeof(Group), hipMemcpyDeviceToHost));
    unsigned long long hist[11] = {0}, sum = 0, over = 0;   // 0, 1, 2, 3-4, 5-8, ... 129-256, more
    uint32_t mx = 0;
    for (const Group &g : hg) {
        uint32_t b = 0;
        while (b < 10 && (b ? 1u << (b - 1) : 0u) < g.nacc) b++;
        hist[b]++; sum += g.nacc; mx = std::max(mx, g.nacc); over += g.nacc > bmax ? 1u : 0u;
    }
    fprintf(stderr, "[k6] accepted per group: max %u mean %.2f of %u groups, %llu above the take of %u; 0 1 2 <=4 <=8 .. <=256 more:", mx,
            (double)sum / ngroups, ngroups, over, bmax);
    for (int b = 0; b < 11; b++) fprintf(stderr, " %llu", hist[b]);
    fprintf(stderr, "\n");
    return 0;
}

struct K6Call {   // what a gapped call runs with; gapped_device sets the mode, gapped_setup reads the development switches, once per call
    // bmax: anchors per group and round, MIMEO_K6_BMAX.  The default is the round's budget over the groups, up to MAX_BATCH: above what any group
    // of a C4 row or of C5MID accepts, so their rounds end with the groups' anchors, not with the take
    uint32_t bmax, rounds;
    bool stats, path, bounded, box_paths;   // box_paths: the anchors' ranks are recorded; the halves are traced after the last round
    int32_t cap;             // of a score in 32-bit DP cells (below)
    uint64_t pool_budget;
    unsigned long long bound_jobs, rescheduled;   // statistics of the bounded mode,
    TraceStats ts;                                // of the path rule's traces
};

// switches, the buffers of a gapped call, the anchors
static int gapped_setup(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_sorted, const uint32_t *d_order, uint64_t nhsps, K6Call &c) {
    // the take: the round's anchor budget shared among the groups, at least 1 (thousands of small groups take few anchors each), at most
    // the size of k6_pick's list.  200 groups of a C4 row: 163 -> MAX_BATCH
    c.bmax = getenv("MIMEO_K6_BMAX") ? (uint32_t)atoi(getenv("MIMEO_K6_BMAX")) : K6_ROUND_ANCHORS / ngroups;
    c.bmax = c.bmax < 1 ? 1 : (c.bmax > MAX_BATCH ? MAX_BATCH : c.bmax);
    c.stats = getenv("MIMEO_K6_STATS") != nullptr;
    if (c.stats) fprintf(stderr, "[k6] take %u anchors per group and round (%u groups, limit %d, budget %u)\n", c.bmax, ngroups, MAX_BATCH, K6_ROUND_ANCHORS);
    // 32-bit DP cells: beyond this score a half extension goes to (or, in k6_dp_any and k6_trace, rebases its cells in) the last kernel;
    // MIMEO_K6_SCORE_CAP lowers it so that tests of ordinary size take that road
    c.cap = getenv("MIMEO_K6_SCORE_CAP") ? std::max(100000, atoi(getenv("MIMEO_K6_SCORE_CAP"))) : 2000000000;
    hipStream_t st = stream();
    int rc;
    if ((rc = g_k6.anchors.reserve(nhsps * sizeof(uint2)))) return rc;
    if ((rc = g_k6.packed.reserve(nhsps * 8))) return rc;
    HIP_TRY(hipMemsetAsync(g_k6.packed.p, 0, nhsps * 8, st));
    if ((rc = g_k6.jobs.reserve((size_t)ngroups * c.bmax * 2 * sizeof(DpJob)))) return rc;
    if ((rc = g_k6.res.reserve((size_t)nhsps * 2 * sizeof(HalfResult)))) return rc;
    if ((rc = g_k6.astate.reserve((size_t)nhsps * 2))) return rc;  // state | defer count
    HIP_TRY(hipMemsetAsync(g_k6.astate.p, 0, (size_t)nhsps * 2, st));
    if ((rc = g_k6.cnt.reserve(32))) return rc;
    if ((rc = g_k6.ovf_list.reserve((size_t)ngroups * c.bmax * 2 * sizeof(unsigned int)))) return rc;
    // many small groups (scaffold pairs of a packed fragmented assembly): one workgroup each will do
    const uint32_t asplit = ngroups > 4096 ? 1u : ANCHOR_SPLIT;
    hipLaunchKernelGGL(k6_anchor_points, dim3(ngroups, asplit), dim3(ANCHOR_THREADS), 0, st, (const Group *)d_groups,
                       d_sorted, d_order, (unsigned long long *)g_k6.packed.p);
    hipLaunchKernelGGL(k6_anchor_final, dim3(ngroups), dim3(256), 0, st, (const Group *)d_groups, d_sorted, d_order,
                       (const unsigned long long *)g_k6.packed.p, (uint2 *)g_k6.anchors.p);
    if (c.path || c.box_paths) {
        if ((rc = g_k6.tctr.reserve(16))) return rc;
        if ((rc = arena_reserve(1024, 0))) return rc;
        HIP_TRY(hipMemsetAsync(g_k6.tctr.p, 0, 16, st));
        // bytes of traceback held at once: a share of the free device memory (like the queue arenas of K4); MIMEO_K6_TRACE_POOL_MB
        // sets it (tests: force slices, or a pool too small for one half)
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        c.pool_budget = std::min<uint64_t>(((uint64_t)free_b + g_k6.pool.cap) / 4, 16ull << 30);
        if (getenv("MIMEO_K6_TRACE_POOL_MB")) c.pool_budget = (uint64_t)atol(getenv("MIMEO_K6_TRACE_POOL_MB")) << 20;
    }
    if (c.bounded && (rc = g_k6.sweep.reserve((size_t)nhsps * 2 * sizeof(HalfSweep)))) return rc;
    return 0;
}

// rounds of k6_pick, dp_round, trace_round under the path rule, k6_resolve until every group is through its anchors
static int gapped_rounds(Group *d_groups, uint32_t ngroups, uint64_t nhsps, const mimeo_params *p, mimeo_alignment *d_aln, K6Call &c) {
    hipStream_t st = stream();
    int rc;
    PathView pv{nullptr, nullptr, nullptr};
    if (c.path || c.box_paths) pv = PathView{(const uint2 *)g_k6.pidx.p, nullptr, (uint32_t *)g_k6.accrank.p};
    const auto pick = c.path ? k6_pick<true> : k6_pick<false>;
    const auto resolve = c.bounded ? k6_resolve<true, true> : c.path ? k6_resolve<true, false>
                         : c.box_paths ? k6_resolve<false, false, true> : k6_resolve<false, false>;
    const HalfSweep *sweep = c.bounded ? (const HalfSweep *)g_k6.sweep.p : nullptr;
    for (;;) {
        HIP_TRY(hipMemsetAsync(g_k6.cnt.p, 0, 32, st));
        unsigned int *njobs = (unsigned int *)g_k6.cnt.p, *remaining = njobs + 1, *novf = njobs + 2, *nrestart = njobs + 4;
        pv.blk = (const PathBlock *)g_k6.arena.p;   // the arena may have grown in the last round
        hipLaunchKernelGGL(pick, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint2 *)g_k6.anchors.p, (const mimeo_alignment *)d_aln,
                           c.bmax, (uint8_t *)g_k6.astate.p, (uint8_t *)g_k6.astate.p + nhsps, (DpJob *)g_k6.jobs.p, njobs, pv);
        unsigned int h0 = 0;   // jobs of the round
        HIP_TRY(hipMemcpyAsync(&h0, njobs, 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h0) {
            const BoundCtx bc{(const mimeo_alignment *)d_aln, (const uint2 *)g_k6.anchors.p, pv};
            if ((rc = dp_round(d_groups, h0, p, c.cap, c.bounded, bc, novf, nrestart))) return rc;
            if (c.stats && (rc = round_stats(h0, nhsps, c.bounded, &c.bound_jobs, nrestart))) return rc;
            if (c.path) {
                c.rounds++;
                if ((rc = trace_round(d_groups, (const DpJob *)g_k6.jobs.p, h0, p, c.cap, c.pool_budget, c.ts, c.bounded, bc))) return rc;
                pv.blk = (const PathBlock *)g_k6.arena.p;
            }
        }
        hipLaunchKernelGGL(resolve, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint2 *)g_k6.anchors.p, (const HalfResult *)g_k6.res.p,
                           d_aln, (uint8_t *)g_k6.astate.p, remaining, pv, sweep);
        unsigned int h4[4] = {0, 0, 0, 0};
        HIP_TRY(hipMemcpyAsync(h4, g_k6.cnt.p, 16, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        c.rescheduled += h4[3];
        if (!h4[1]) return 0;
    }
}

static void path_rule_stats(const K6Call &c) {
    fprintf(stderr, "[k6] path rule: traceback %.3f ms, rounds %u slices %u, %llu path blocks, pool %.1f MB, largest half %.3f MB", c.ts.ms,
            c.rounds, c.ts.slices, (unsigned long long)c.ts.arena_used, g_k6.pool.cap / 1048576.0, c.ts.largest / 1048576.0);
    if (c.bounded) fprintf(stderr, ", bounded jobs %llu, rescheduled %llu", c.bound_jobs, c.rescheduled);
    fprintf(stderr, "\n");
}

int gapped_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_sorted, const uint32_t *d_order,
                  uint64_t nhsps, const mimeo_params *p, mimeo_alignment *d_aln, bool want_paths) {
    if (!ngroups || !nhsps) return 0;
    hipStream_t st = stream();
    int rc;
    const bool path = p->gapped && p->anchor_rule == MIMEO_ANCHOR_PATH;
    if (want_paths && nhsps >= (1ull << 31)) { set_error("paths: more than 2^31 HSPs in one batch"); return MIMEO_ERR_LIMIT; }
    if (want_paths || path) {   // per half slot its blocks, per alignment slot its anchor's rank (the path rule's tables, under every rule)
        if ((rc = g_k6.pidx.reserve((size_t)nhsps * 2 * sizeof(uint2)))) return rc;
        if ((rc = g_k6.accrank.reserve((size_t)nhsps * 4))) return rc;
    }
    if (!p->gapped) {
        hipLaunchKernelGGL(k6_ungapped, dim3(ngroups), dim3(256), 0, st, d_groups, d_sorted, d_order, d_aln);
        if (want_paths) {
            if ((rc = arena_reserve(nhsps, 0))) return rc;
            hipLaunchKernelGGL(k6_ungapped_paths, dim3(ngroups), dim3(256), 0, st, (const Group *)d_groups, (const mimeo_alignment *)d_aln,
                               (PathBlock *)g_k6.arena.p, (uint2 *)g_k6.pidx.p, (uint32_t *)g_k6.accrank.p);
        }
    } else {
        K6Call c{};
        c.path = path; c.box_paths = want_paths && !path; c.bounded = path && p->bound_extensions;   // api.hip: bound_extensions needs the path rule
        if ((rc = gapped_setup(d_groups, ngroups, d_sorted, d_order, nhsps, c))) return rc;
        if ((rc = gapped_rounds(d_groups, ngroups, nhsps, p, d_aln, c))) return rc;
        if (c.stats && (rc = accepted_stats(d_groups, ngroups, c.bmax))) return rc;
        if (c.path && c.stats) path_rule_stats(c);
        if (c.box_paths && (rc = paths_pass(d_groups, ngroups, p, c.cap, d_aln, c.pool_budget, c.stats))) return rc;
    }
    if (want_paths)
        hipLaunchKernelGGL(k6_kept_ranks, dim3((ngroups + 63) / 64), dim3(64), 0, st, d_groups, ngroups, (const mimeo_alignment *)d_aln,
                           (uint32_t *)g_k6.accrank.p, (const uint2 *)g_k6.pidx.p, p->hspthresh);
    hipLaunchKernelGGL(k6_finish, dim3((ngroups + 63) / 64), dim3(64), 0, st, d_groups, ngroups, d_aln, p->hspthresh);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mimeo
