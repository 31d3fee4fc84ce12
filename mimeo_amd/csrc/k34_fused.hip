// K34 — seed scan and pre-filter of one unit in ONE kernel (SURVEY §8a A7 + A8: lastz's query scan with 13 probes per
// base and the first look at every seed hit; reference call site src/mimeo/wrappers.py:1025-1037,
// `--step=1 --strand=both --gfextend --entropy --hspthresh=H`).
//
// Round 1 materialised the hit flood: K3 wrote 77.8 M (tpos, qpos) records per 10 Mbp x 10 Mbp unit (0.9 GB of
// stores for 0.62 GB of records), K4 read them back and gathered 13 eight-byte words around every hit through L2
// — to prove for 95 % of them that nothing comes of them.  Here no hit is stored unless it matters:
//   * both seed indexes are CSR in the transition-closed key layout (common.h): a workgroup owns one tile of 4096
//     keys, stages the query tile's offsets in LDS (relative to the tile, 16 bits each: 8 KiB) and resolves all 13 probes of a
//     word there (K3's join);
//   * every index entry carries its seed FRAME (K2: 192 bases around the seed start, both planes, one common
//     alignment), so a tile's frames are contiguous: the query frames are STREAMED into LDS, coalesced, in segments
//     of QSEG entries, and each wavefront keeps the frames of 64 target entries in registers (one entry per lane,
//     the next chunk's already in flight);
//   * a wavefront enumerates the (target entry, query entry) pairs of its chunk into a small LDS queue of
//     descriptors — first pass: probe by probe and level by level (a ballot and v_mbcnt per level) into a ring of 128;
//     split pass: lane-major behind a prefix sum of the per-entry counts, long ranges densely — so that the rounds are
//     full wavefronts whatever the per-entry fan-out, which is Poisson(7.8) on a C4 unit; a lane takes one pair, fetches
//     the target frame from its owner lane
//     (ds_bpermute) and the query frame from LDS, and runs the pre-filter: twelve XORs bring the two frames
//     together, every shift of the popcount bounds and of the earlier-seed-hit test is a compile-time constant;
//   * the ~4 % of the pairs the filter cannot dismiss are staged per wavefront (ballot + prefix count); at the flush the
//     first pass runs the SHARP filter on the 64 staged pairs (both frames fetched by entry number: pair_needs_walk_sharp)
//     and only the third that survives goes to the unit's walk queue (k4_walk_batch: the exact walk, right behind
//     this kernel; the split pass leaves the sharp filter to that kernel).
// HBM traffic per unit: the two offset arrays, positions + frames of both sides once (52 bytes per entry), and the target
// frames of a tile once more per further query segment (Infinity Cache).
#include <cstdio>
#include <algorithm>
#include <cstdlib>

#include "k34.h"
#include "k34_filter.h"

namespace mimeo {

constexpr uint32_t TCH = 64;      // target entries per wavefront and chunk: one per lane
constexpr uint32_t DQ = 192;      // pair descriptors per wavefront and round
constexpr unsigned long long HEAVY_HITS = 262144;   // hits of a tile beyond which it is split (a tile of a 10 Mbp x 10 Mbp unit averages 19 000)
// The split pass works the listed tiles off in PARTS of about PART_HITS seed hits each (k34_plan: a tile's parts = shares of its
// target chunk groups x ranges of its query entries), dealt to persistent workgroups by an atomic counter: a poly-A tile of
// 6000 x 6000 entries (3.6e7 hits) is 280 parts, a tile just above the threshold two — the static 8 x 8 split of round 2 left the
// machine to the 64 workgroups of the largest tile (C5: 55 ps per seed hit in this pass against 13.5 in the first).
constexpr unsigned long long PART_HITS = 131072;
constexpr uint32_t HEAVY_GRID = 2048;  // persistent workgroups of the split pass (four per workgroup slot of the device)

// One launch works off EVERY unit of a batch (grid.y = the batch's units that have seed hits to look for): the machine never
// drains between units (a launch per unit left ~6 % of it idle in the tails of 4096 workgroups over 512 slots, and cost three
// launches per unit).  A unit's own things come from a device table (FusedUnit, k4_device.h): its two seed indexes, its
// number in the batch, and its region of the walk queue.
struct FusedArgs {
    const FusedUnit *units;
    ExtQueues q;
    HeavyPlan plan;
    int xdrop, hspthresh, transitions;
    uint32_t dbg;  // switch word (MIMEO_K34_DEBUG, the two test witnesses): 16 = the split pass does not drop run members, 32 = no sharp
                   // filter at the first pass's walk-queue flush (entries go out unmarked, the walk kernel filters them)
};

constexpr uint32_t DENSE_MIN = 48;   // split pass: a probe's range of this many entries or more is enumerated densely
__device__ __forceinline__ uint4 readlane4(const uint4 v, int lane) {   // lane: wave-uniform
    return make_uint4((uint32_t)__builtin_amdgcn_readlane((int)v.x, lane), (uint32_t)__builtin_amdgcn_readlane((int)v.y, lane),
                      (uint32_t)__builtin_amdgcn_readlane((int)v.z, lane), (uint32_t)__builtin_amdgcn_readlane((int)v.w, lane));
}
__device__ __forceinline__ uint4 bperm4(uint32_t src_lane, const uint4 v) {
    const int a = (int)(src_lane << 2);
    return make_uint4((uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)v.x), (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)v.y),
                      (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)v.z), (uint32_t)__builtin_amdgcn_ds_bpermute(a, (int)v.w));
}

// LDS of a workgroup: the query tile's offsets RELATIVE TO THE CURRENT SEGMENT and clamped to it (16 bits each: a key's
// range inside the segment is sQ[w] .. sQ[w + 1] whatever the size of the tile — one code path for tiles of one segment
// and of many, in both passes; rewritten from the offset array, L2-resident, for every segment), QSEG query frames
// (three 16-byte parts), one descriptor queue and one walk staging area per wavefront, the N flags of the segment.  First pass: 512 threads, two
// workgroups per CU, QSEG = 1280 (79 KiB each): the 2441 entries of an average C4 tile are two segments — every target
// chunk is visited once per segment (frames, key, 13 probes, prefix sum, descriptors: ~530 instructions for the
// visit), so three segments of 1024 cost a third more visits for the same pairs.
// The ONE statement of the layout: the areas' byte offsets, one behind the other; BYTES goes to the launch, the typed pointers
// to the kernel.
template <int THREADS, uint32_t QSEG>
struct K34Lds {
    static constexpr int WAVES = THREADS / 64;
    static constexpr size_t AT_Q = 0;                                                      // TILE_WORDS + 1 offsets of 16 bits
    static constexpr size_t AT_QF = ((TILE_WORDS + 1) * 2 + 15) / 16 * 16;                 // 3 parts of QSEG frames
    static constexpr size_t AT_D = AT_QF + (size_t)QSEG * 48;                              // WAVES * DQ descriptors
    static constexpr size_t AT_WALK = AT_D + (size_t)WAVES * DQ * 4;                       // WAVES * 64 staged pairs
    static constexpr size_t AT_QN = AT_WALK + (size_t)WAVES * 64 * 8;                      // QSEG flags
    static constexpr size_t AT_TOTAL = AT_QN + QSEG;                                       // the count prologue's sum
    static constexpr size_t BYTES = AT_TOTAL + 16;
    uint16_t *sQ;
    uint4 *sQF;
    uint32_t *sD;       // this wavefront's descriptor queue
    uint2 *s_walk;      // this wavefront's walk staging area
    uint8_t *sQN;
    unsigned long long *s_total;
    __device__ __forceinline__ K34Lds(uint8_t *smem, uint32_t wv)
        : sQ(reinterpret_cast<uint16_t *>(smem + AT_Q)), sQF(reinterpret_cast<uint4 *>(smem + AT_QF)),
          sD(reinterpret_cast<uint32_t *>(smem + AT_D) + wv * DQ), s_walk(reinterpret_cast<uint2 *>(smem + AT_WALK) + wv * 64),
          sQN(smem + AT_QN), s_total(reinterpret_cast<unsigned long long *>(smem + AT_TOTAL)) {}
    // the count prologue's view of the frame area: the tile's two offset arrays (TILE_WORDS + 1 words each), staged whole
    static_assert((size_t)QSEG * 48 >= 2 * (TILE_WORDS + 4) * 4, "the count prologue stages both offset arrays in the frame area");
    __device__ __forceinline__ uint32_t *count_toff() const { return reinterpret_cast<uint32_t *>(sQF); }
    __device__ __forceinline__ uint32_t *count_qoff() const { return reinterpret_cast<uint32_t *>(sQF) + TILE_WORDS + 4; }
};

// What a wavefront carries through a pass: who it is, the unit it works on (by value: wave-uniform registers, not a reload through
// the pointer at every use; its pointers come out of a table: held in global address space, device_util.h; split pass: set per
// part), and the pairs it has staged for the walk queue.
struct K34Wave {
    uint32_t lane, wv;
    uint64_t lt_mask;
    uint32_t ai;        // the unit's number in the launch
    GFusedUnit U;
    uint32_t part_no;   // split pass: the number of my part in its tile
    uint32_t n_walk;    // pairs staged in s_walk
};
__device__ __forceinline__ K34Wave wave_open(const FusedArgs &A, const uint32_t ai) {
    K34Wave W;
    W.lane = threadIdx.x & 63u; W.wv = threadIdx.x >> 6;
    W.lt_mask = (1ull << W.lane) - 1ull;
    W.ai = ai;
    W.U = A.units[ai];
    W.part_no = 0;
    W.n_walk = 0;
    return W;
}
// one tile of a unit's two seed indexes
struct K34Tile {
    uint32_t tile, t0, nT, q0, nQ;   // its number; first entry and entry count, target and query
    gptr<uint32_t> toff, qoff;
    gptr<uint4> tF0, tF1, tF2;       // the target entries' frames, three parts
};
// the frames and positions of 64 target entries, one per lane
struct K34Chunk {
    uint4 f0, f1, f2;
    uint32_t pos;
};

// ---- the wavefront's walk staging ---------------------------------------------------------------------------
// the pairs the filter passed on go to the batch's walk queue, 64 at a time (one atomic per flush).  A staged pair names its two
// index ENTRIES: the positions of all 64 are fetched here, one gather per flush instead of one per round, and — first pass —
// so are the two frames (six 16-byte loads per lane from arrays this workgroup has just streamed) for the sharp filter: the
// staged pairs are a full wavefront of compacted work, the other wavefronts of the CU hide the gather, and only the
// survivors are appended, marked in bit 31 of x (WALK_SHARP_DONE: the walk kernel does not filter them again)
template <bool HEAVY>
__device__ __forceinline__ void walk_flush(const FusedArgs &A, const K34Wave &W, const uint2 *s_walk, const uint32_t n) {
    __builtin_amdgcn_wave_barrier();
    // (split pass: the 64 workgroups that share a tile have one blockIdx.x — spread them, or a microsatellite tile fills one shard)
    const uint32_t shard = (HEAVY ? blockIdx.x + W.part_no : blockIdx.x) & 7u;
    uint2 e = make_uint2(0, 0);
    bool keep = W.lane < n;
    if (keep) {
        const uint2 s = s_walk[W.lane];
        const uint32_t tp = W.U.T.pos[s.x], qp = W.U.Q.pos[s.y];
        e = make_uint2(tp & POS_MASK, qp & POS_MASK);
        if (!HEAVY && !(A.dbg & 32u)) {
            const gptr<uint4> tf = W.U.T.fr + s.x, qf = W.U.Q.fr + s.y;
            const uint4 ta = tf[0], tb = tf[W.U.T.fr_stride], tc = tf[2 * (size_t)W.U.T.fr_stride];
            const uint4 qa = qf[0], qb = qf[W.U.Q.fr_stride], qc = qf[2 * (size_t)W.U.Q.fr_stride];
            keep = ((tp | qp) & POS_NFLAG) != 0 || pair_needs_walk_sharp(ta, tb, tc, qa, qb, qc, A.xdrop, A.hspthresh, A.transitions);
            e.x |= WALK_SHARP_DONE;
        }
    }
    const uint64_t km = __ballot(keep);
    if (km) {
        unsigned long long b = 0;
        if (W.lane == 0) b = atomicAdd(&A.q.nwalk_u[(size_t)W.ai * 8 + shard], (unsigned long long)__popcll(km));
        b = __shfl(b, 0) + __popcll(km & W.lt_mask);
        if (keep && b < W.U.walk_cap) A.q.walkq[W.U.walk_base + (size_t)shard * W.U.walk_cap + b] = e;
    }
    __builtin_amdgcn_wave_barrier();
}
// the lanes that `need` a walk stage their pair: its two entries, target te and query q0 + qi (walk_flush looks their positions up)
template <bool HEAVY>
__device__ __forceinline__ void walk_push(const FusedArgs &A, K34Wave &W, uint2 *s_walk, const bool need, const uint32_t te, const uint32_t q0, const uint32_t qi) {
    const uint64_t m = __ballot(need);
    if (m) {
        const uint32_t add = (uint32_t)__popcll(m);
        if (W.n_walk + add > 64u) { walk_flush<HEAVY>(A, W, s_walk, W.n_walk); W.n_walk = 0; }
        if (need) s_walk[W.n_walk + __popcll(m & W.lt_mask)] = make_uint2(te, q0 + qi);
        W.n_walk += add;
    }
}

// ---- a tile --------------------------------------------------------------------------------------------------
// false = one of the two indexes has no entry in this tile (tile_hits is zeroed per batch)
__device__ __forceinline__ bool tile_open(K34Tile &T, const GFusedUnit &U, const uint32_t tile) {
    T.tile = tile;
    T.toff = U.T.off + (size_t)tile * TILE_WORDS; T.qoff = U.Q.off + (size_t)tile * TILE_WORDS;
    T.t0 = T.toff[0]; T.nT = T.toff[TILE_WORDS] - T.t0;
    T.q0 = T.qoff[0]; T.nQ = T.qoff[TILE_WORDS] - T.q0;
    return T.nT && T.nQ;
}
__device__ __forceinline__ void tile_frames(K34Tile &T, const GFusedUnit &U) {
    T.tF0 = U.T.fr + T.t0; T.tF1 = T.tF0 + U.T.fr_stride; T.tF2 = T.tF1 + U.T.fr_stride;
}

// The first pass's count prologue.  A tile with far more hits than the average — a microsatellite's seed words: thousands of
// entries of ONE key on both sides, 10^7-10^8 hits in one tile — or with more query entries than 16-bit offsets can name is not
// worked off by one workgroup while the chip waits: it is listed for the split pass.  The test is an ESTIMATE made up front from
// the exact-key hits alone (one probe per word instead of thirteen; both offset arrays pass through the frame area
// of LDS once): 13 x sum nT(w) nQ(w).  Which pass takes a tile changes nothing in the results; the exact count of a
// tile — the seed_hits statistic — is the sum of the pairs its chunk visits enumerate.
// The answer is the same in every thread of the workgroup (the conditions are uniform).
enum K34TileFate { TILE_NOTHING, TILE_HERE, TILE_LISTED };   // no seed hit in it; work it here; listed for the split pass
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ K34TileFate count_prologue(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, const K34Wave &W, const K34Tile &T) {
    uint32_t *sT = L.count_toff(), *sQ32 = L.count_qoff();
    {
        const gptr<uint4> s0 = T.toff.as<uint4>(), s1 = T.qoff.as<uint4>();
        uint4 *d0 = reinterpret_cast<uint4 *>(sT), *d1 = reinterpret_cast<uint4 *>(sQ32);
        for (uint32_t k = threadIdx.x; k < TILE_WORDS / 4; k += THREADS) { const uint4 a = s0[k], b = s1[k]; d0[k] = a; d1[k] = b; }
        if (threadIdx.x == 0) { sT[TILE_WORDS] = T.t0 + T.nT; sQ32[TILE_WORDS] = T.q0 + T.nQ; *L.s_total = 0ull; }
    }
    __syncthreads();
    unsigned long long cnt = 0;
    for (uint32_t w = threadIdx.x; w < TILE_WORDS; w += THREADS)
        cnt += (unsigned long long)(sT[w + 1] - sT[w]) * (sQ32[w + 1] - sQ32[w]);
    for (int o = 32; o > 0; o >>= 1) cnt += __shfl_xor(cnt, o);
    if (W.lane == 0 && cnt) atomicAdd(L.s_total, cnt);
    __syncthreads();
    if (!*L.s_total && A.transitions) {   // no exact-key hit (sparse tiles of small scaffolds): any hit at all?  Otherwise the tile is done
        __syncthreads();
        unsigned long long c2 = 0;
        for (uint32_t w = threadIdx.x; w < TILE_WORDS; w += THREADS) {
            const uint32_t nt = sT[w + 1] - sT[w];
            if (nt)
                for (int j = 0; j < SEED_WEIGHT; j++) { const uint32_t w2 = w ^ (1u << j); c2 += sQ32[w2 + 1] - sQ32[w2]; }
        }
        if (__syncthreads_or(c2 != 0) == 0) return TILE_NOTHING;
    } else if (!*L.s_total) {
        return TILE_NOTHING;
    }
    const unsigned long long tile_est = *L.s_total * (A.transitions ? (unsigned long long)(SEED_WEIGHT + 1) : 1ull);
    if (tile_est > HEAVY_HITS || T.nQ > 0xFFFFu) {   // (a tile of 65536 query entries and more: 52 segments for one workgroup)
        if (threadIdx.x == 0) {   // at most NTILE entries per unit
            const size_t slot = (size_t)W.ai * NTILE + atomicAdd(&A.q.nheavy_u[W.ai], 1ull);
            A.q.heavy[slot] = T.tile;
            A.q.heavy_est[slot] = tile_est;
        }
        return TILE_LISTED;
    }
    return TILE_HERE;
}

// ---- one query segment in LDS: entries [qs, qe) of the tile ------------------------------------------------------------
template <int THREADS>
constexpr int k34_nro() { return (TILE_WORDS + THREADS) / THREADS; }   // 4097 offsets over the workgroup's threads
// ro: my share of the tile's query offsets (relative to its first entry), kept in registers for all its segments
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void stage_segment(const K34Lds<THREADS, QSEG> &L, const GFusedUnit &U, const K34Tile &T, const uint32_t (&ro)[k34_nro<THREADS>()],
                                              const uint32_t qs, const uint32_t qe) {
    constexpr int NRO = k34_nro<THREADS>();
    const uint32_t qn = qe - qs;
    // the tile's offsets relative to this segment, clamped to it: key w's entries inside the segment are sQ[w] .. sQ[w + 1]
#pragma unroll
    for (int i = 0; i < NRO; i++) {
        const uint32_t k = threadIdx.x + (uint32_t)i * THREADS;
        if (k <= TILE_WORDS) L.sQ[k] = (uint16_t)(min(max(ro[i], qs), qe) - qs);
    }
    {
        const gptr<uint4> s0 = U.Q.fr + T.q0 + qs, s1 = s0 + U.Q.fr_stride, s2 = s1 + U.Q.fr_stride;
        const gptr<uint32_t> sp = U.Q.pos + T.q0 + qs;
        // an entry's four loads are issued together, the LDS writes follow as the data arrives (counted vmcnt waits).  (Two
        // entries per thread and trip, 8 loads in flight, measured no faster on a C4 row and cost 13 VGPRs; three spill.)
        for (uint32_t i = threadIdx.x; i < qn; i += THREADS) {
            const uint4 a = s0[i], b = s1[i], c = s2[i];
            const uint32_t pq = sp[i], pp = pq & POS_MASK;
            L.sQF[i] = a;
            L.sQF[QSEG + i] = b;
            L.sQF[2 * QSEG + i] = c;
            // bit 0: N in the frame; bit 1: too close to an end of the scaffold for the run test's three seed windows
            L.sQN[i] = (uint8_t)((pq >> 31) | ((pp >= 2u && pp + 1u + SEED_LEN <= U.Qv.len) ? 0u : 2u));
        }
    }
}

// ---- the target chunk's registers, fetched one chunk ahead --------------------------------------------------------------
// chunk ch of the tile into C, one entry per lane (the lanes beyond the tile's last entry keep what they hold)
__device__ __forceinline__ void chunk_fetch(K34Chunk &C, const K34Tile &T, const K34Wave &W, const uint32_t ch) {
    const uint32_t e = ch * TCH + W.lane;
    if (e < T.nT) { C.f0 = T.tF0[e]; C.f1 = T.tF1[e]; C.f2 = T.tF2[e]; C.pos = W.U.T.pos[T.t0 + e]; }
}
// my first chunk's frames: in flight while the first query segment is staged
__device__ __forceinline__ K34Chunk chunk_first(const K34Tile &T, const K34Wave &W, const uint32_t ch_first, const uint32_t nchunks) {
    K34Chunk C;
    C.f0 = make_uint4(0, 0, 0, 0); C.f1 = C.f0; C.f2 = C.f0;
    C.pos = 0;
    if (ch_first < nchunks) chunk_fetch(C, T, W, ch_first);
    return C;
}
// next chunk of this wavefront behind ch: the following one of this segment, or its first one for the next segment (more_segments)
__device__ __forceinline__ void chunk_ahead(K34Chunk &C, const K34Tile &T, const K34Wave &W, const uint32_t ch, const uint32_t ch_first, const uint32_t ch_step,
                                            const uint32_t nchunks, const bool more_segments) {
    uint32_t nx = ch + ch_step;
    if (nx >= nchunks) nx = more_segments ? ch_first : 0xFFFFFFFFu;
    if (nx != 0xFFFFFFFFu && nx != ch) chunk_fetch(C, T, W, nx);
}

// ---- a round of 64 pairs --------------------------------------------------------------------------------------------------
struct K34QueryFrame { uint4 a, b, c; uint32_t flag; };   // a query entry's frame and flags out of the segment in LDS
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ K34QueryFrame query_frame(const K34Lds<THREADS, QSEG> &L, const uint32_t qi) {
    K34QueryFrame q;
    q.a = L.sQF[qi]; q.b = L.sQF[QSEG + qi]; q.c = L.sQF[2 * QSEG + qi];
    q.flag = L.sQN[qi];
    return q;
}
// 64 pairs, one per lane: the target entry te (number in the index), its frame and position, the query entry qi of the current
// segment (first entry qs).  live: still to be looked at by the pre-filter
template <bool HEAVY>
__device__ __forceinline__ void pair_round(const FusedArgs &A, K34Wave &W, uint2 *s_walk, const K34Tile &T, const bool valid, const bool live, const uint4 ta,
                                           const uint4 tb, const uint4 tc, const uint32_t tpf, const uint32_t te, const K34QueryFrame &q, const uint32_t qi,
                                           const uint32_t qs) {
    bool need = false;
    uint32_t qp = 0;
    if (__ballot(live)) {
        if (live)
            need = ((tpf >> 31) | (q.flag & 1u)) != 0 || pair_needs_walk(ta, tb, tc, q.a, q.b, q.c, A.xdrop, A.hspthresh, A.transitions);
    }
    if (W.U.same) {  // the main diagonal of a self unit belongs to k4_diag0 (one unit in 2 S: the slow way will do)
        if (valid) {
            qp = W.U.Q.pos[T.q0 + qs + qi] & POS_MASK;
            if ((tpf & POS_MASK) == qp) need = false;
        }
    }
    walk_push<HEAVY>(A, W, s_walk, need, te, T.q0 + qs, qi);
}
// first pass: every valid pair goes to the pre-filter
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void pair_round_first(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const bool valid, const uint4 ta,
                                                 const uint4 tb, const uint4 tc, const uint32_t tpf, const uint32_t te, const uint32_t qi, const uint32_t qs) {
    const K34QueryFrame q = query_frame(L, qi);
    pair_round<false>(A, W, L.s_walk, T, valid, valid, ta, tb, tc, tpf, te, q, qi, qs);
}
// split pass: interior members of runs of consecutive seed hits leave no record: out, before the filter (a microsatellite
// tile is nearly all of them: whole rounds skip the filter)
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void pair_round_split(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const bool valid, const uint4 ta,
                                                 const uint4 tb, const uint4 tc, const uint32_t tpf, const uint32_t te, const uint32_t qi, const uint32_t qs) {
    const K34QueryFrame q = query_frame(L, qi);
    bool live = valid;
    if (!(A.dbg & 16u)) {
        bool inner = false;
        if (valid && ((tpf >> 31) | q.flag) == 0 && !W.U.Tv.svt && run_interior(ta, tb, tc, q.a, q.b, q.c, A.transitions)) {
            const uint32_t tp = tpf & POS_MASK;
            inner = tp >= 2u && tp + 1u + SEED_LEN <= W.U.Tv.len;   // (the query's ends: bit 1 of its flag)
        }
        live = valid && !inner;
    }
    pair_round<true>(A, W, L.s_walk, T, valid, live, ta, tb, tc, tpf, te, q, qi, qs);
}

// ---- the three enumerators of a chunk's pairs in the current segment ---------------------------------------------------
// tvalid: my lane holds a target entry; w: its in-tile key; e0: the chunk's first entry in the tile; hits_acc: the pairs this
// wavefront enumerates in this tile (wave-uniform)

// First pass: descriptors written LEVEL BY LEVEL, probe-major, for the probes jlo .. jhi - 1.  For probe j, level k = the lanes whose range
// holds more than k entries: their slots are ring position + v_mbcnt of the ballot, one LDS write each; a probe's
// range holds 0.6 entries on average on a C4 tile, so a probe is two or three levels (the ballot of the next one is
// empty).  No prefix sum over the lanes, no second visit of the offsets, no per-lane loop that runs as long as the
// busiest lane's: the emission was 20 % of this kernel's time.  The ring holds 128 descriptors: a round of 64 pairs
// runs as soon as 64 are waiting.
constexpr uint32_t RING = 128;
static_assert(RING <= DQ, "the ring lives in the wavefront's descriptor queue");
struct K34Ring { uint32_t head, tail, pend; };   // ring positions (below RING) and descriptors waiting: wave-uniform
// the range of probe jj in this segment (first entry an, cn entries), fetched a probe ahead of its use
__device__ __forceinline__ void probe_range(const uint16_t *sQ, const bool tvalid, const uint32_t w, const int jj, const int jhi, uint32_t &an, uint32_t &cn) {
    an = 0; cn = 0;
    if (tvalid && jj < jhi) {
        const uint32_t w2 = jj ? (w ^ (1u << (jj - 1))) : w;
        an = sQ[w2];
        cn = (uint32_t)sQ[w2 + 1] - an;
    }
}
// the n <= 64 oldest descriptors of the ring
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void ring_round(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const K34Chunk &C, K34Ring &R,
                                           const uint32_t e0, const uint32_t qs, const uint32_t n) {
    __builtin_amdgcn_wave_barrier();
    const bool valid = W.lane < n;
    const uint32_t d = valid ? L.sD[(R.head + W.lane) & (RING - 1u)] : 0u;
    const uint32_t owner = d >> 16, qi = d & 0xFFFFu;
    const uint4 ta = bperm4(owner, C.f0), tb = bperm4(owner, C.f1), tc = bperm4(owner, C.f2);
    const uint32_t tpf = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)C.pos);
    pair_round_first(A, L, W, T, valid, ta, tb, tc, tpf, T.t0 + e0 + owner, qi, qs);
    __builtin_amdgcn_wave_barrier();
    R.head = (R.head + 64u) & (RING - 1u);
    R.pend -= n;
}
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void emit_levels(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const K34Chunk &C, const bool tvalid,
                                            const uint32_t w, const int jlo, const int jhi, const uint32_t e0, const uint32_t qs, unsigned long long &hits_acc) {
    const uint32_t l16 = W.lane << 16;
    K34Ring R{0, 0, 0};
    uint32_t an = 0, cn = 0;
    probe_range(L.sQ, tvalid, w, jlo, jhi, an, cn);
#pragma unroll 1
    for (int j = jlo; j < jhi; j++) {
        const uint32_t ak = l16 | an, cnt = cn;
        probe_range(L.sQ, tvalid, w, j + 1, jhi, an, cn);
        uint32_t k = 0;
#pragma unroll 1
        for (uint64_t m = __ballot(cnt > 0u); m; m = __ballot(cnt > k)) {
            if (cnt > k) {
                const uint32_t slot = __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, R.tail));
                L.sD[slot & (RING - 1u)] = ak + k;
            }
            const uint32_t add = (uint32_t)__popcll(m);
            R.tail = (R.tail + add) & (RING - 1u);
            R.pend += add;
            hits_acc += add;
            k++;
            if (R.pend >= 64u) ring_round(A, L, W, T, C, R, e0, qs, 64u);   // (fewer than 64 waited before this level: the ring never overflows)
        }
    }
    if (R.pend) ring_round(A, L, W, T, C, R, e0, qs, R.pend);   // the rest of this chunk's pairs
}

// Split pass: every probe's range is counted (c: my entry's pairs in short ranges, nmask: its probes with any), and a prefix sum of
// the counts over the lanes places the descriptors lane-major, DQ to a round; a range of DENSE_MIN entries or more is left to
// emit_dense (dmask: those probes)
__device__ __forceinline__ void count_probes(const uint16_t *sQ, const bool tvalid, const uint32_t w, const int nn, uint32_t &c, uint32_t &nmask, uint32_t &dmask) {
    if (!tvalid) return;
    for (int j = 0; j < nn; j++) {
        const uint32_t w2 = j ? (w ^ (1u << (j - 1))) : w;
        const uint32_t a = sQ[w2], b = sQ[w2 + 1];
        if (b - a >= DENSE_MIN) { dmask |= 1u << j; continue; }
        c += b - a;
        nmask |= (b != a ? 1u : 0u) << j;
    }
}
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void emit_lane_major(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const K34Chunk &C, const uint32_t w,
                                                const uint32_t c, const uint32_t nmask, const uint32_t e0, const uint32_t qs, unsigned long long &hits_acc) {
    const uint32_t inc = wave_inclusive_sum(c);
    const uint32_t tot = (uint32_t)__builtin_amdgcn_readlane((int)inc, 63), st = inc - c;
    hits_acc += tot;
    for (uint32_t rb = 0; rb < tot; rb += DQ) {
        if (c && st < rb + DQ && st + c > rb) {
            // a probe's range holds one or two entries nearly always (0.3 on average on a C4 tile, the empty ones
            // are not in nmask): they are written outright, the loop is for the rest; a range that straddles the
            // window of this round is clipped entry by entry
            uint32_t acc = st;
            const uint32_t wend = rb + DQ;
            for (uint32_t m = nmask; m; m &= m - 1u) {
                const uint32_t j = (uint32_t)__builtin_ctz(m);
                const uint32_t w2 = j ? (w ^ (1u << (j - 1u))) : w;
                const uint32_t a = L.sQ[w2], cnt = (uint32_t)L.sQ[w2 + 1] - a, d0 = (W.lane << 16) | a;
                if (acc >= rb && acc + cnt <= wend) {
                    uint32_t *dst = L.sD + (acc - rb);
                    dst[0] = d0;
                    if (cnt > 1) {
                        dst[1] = d0 + 1u;
#pragma unroll 1
                        for (uint32_t k = 2; k < cnt; k++) dst[k] = d0 + k;
                    }
                } else {
                    const uint32_t g0 = max(acc, rb), g1 = min(acc + cnt, wend);
#pragma unroll 1
                    for (uint32_t g = g0; g < g1; g++) L.sD[g - rb] = d0 + (g - acc);
                }
                acc += cnt;
            }
        }
        __builtin_amdgcn_wave_barrier();
        const uint32_t n = min(DQ, tot - rb);
        for (uint32_t i = 0; i < n; i += 64) {
            const bool valid = i + W.lane < n;
            const uint32_t d = valid ? L.sD[i + W.lane] : 0u;
            const uint32_t owner = d >> 16, qi = d & 0xFFFFu;
            // the target frame lives in its owner lane's registers, the query frame in LDS
            const uint4 ta = bperm4(owner, C.f0), tb = bperm4(owner, C.f1), tc = bperm4(owner, C.f2);
            const uint32_t tpf = (uint32_t)__builtin_amdgcn_ds_bpermute((int)(owner << 2), (int)C.pos);
            pair_round_split(A, L, W, T, valid, ta, tb, tc, tpf, T.t0 + e0 + owner, qi, qs);
        }
        __builtin_amdgcn_wave_barrier();
    }
}
// Split pass, long ranges — a microsatellite's key holds hundreds of the segment's entries, and the split pass is made of
// such tiles — are not written out as descriptors: for one target entry at a time (its frame in scalar
// registers) the lanes take 64 consecutive query entries of the range, whose frames are conflict-free LDS
// reads.  No descriptor is written or read and no lane shuffle fetches a frame: the enumeration was 57 % of
// the split pass.
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void emit_dense(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const K34Tile &T, const K34Chunk &C, const uint32_t w,
                                           const uint32_t dmask, const uint32_t e0, const uint32_t qs, unsigned long long &hits_acc) {
    for (uint64_t lm = __ballot(dmask != 0u); lm; lm &= lm - 1ull) {
        const int o = __builtin_ctzll(lm);
        const uint4 ta = readlane4(C.f0, o), tb = readlane4(C.f1, o), tc = readlane4(C.f2, o);
        const uint32_t tpf = (uint32_t)__builtin_amdgcn_readlane((int)C.pos, o), wo = (uint32_t)__builtin_amdgcn_readlane((int)w, o);
        for (uint32_t dm = (uint32_t)__builtin_amdgcn_readlane((int)dmask, o); dm; dm &= dm - 1u) {
            const uint32_t j = (uint32_t)__builtin_ctz(dm), w2 = j ? (wo ^ (1u << (j - 1u))) : wo;
            const uint32_t a = L.sQ[w2], b = L.sQ[w2 + 1];
            hits_acc += b - a;
            for (uint32_t i = a; i < b; i += 64u) {
                const bool valid = i + W.lane < b;
                pair_round_split(A, L, W, T, valid, ta, tb, tc, tpf, T.t0 + e0 + (uint32_t)o, valid ? i + W.lane : a, qs);
            }
        }
    }
}

// ---- the two passes --------------------------------------------------------------------------------------------------
// Everything below returns for the whole workgroup at once (the conditions are uniform).

// First pass: grid (tiles, units).  A workgroup counts its tile, lists it for the split pass or works it off: every target chunk
// (one per wavefront at a time) against every query segment.
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void first_pass_tile(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W) {
    constexpr int WAVES = THREADS / 64, NRO = k34_nro<THREADS>();
    K34Tile T;
    if (!tile_open(T, W.U, blockIdx.x)) return;
    if (count_prologue(A, L, W, T) != TILE_HERE) return;
    // my share of the tile's query offsets: from the copy the count prologue staged in LDS (read before the frames overwrite it:
    // the segment loop opens with a barrier)
    uint32_t ro[NRO];
#pragma unroll
    for (int i = 0; i < NRO; i++) {
        const uint32_t k = threadIdx.x + (uint32_t)i * THREADS;
        ro[i] = 0;
        if (k <= TILE_WORDS) ro[i] = (k < TILE_WORDS ? L.count_qoff()[k] : T.q0 + T.nQ) - T.q0;
    }
    // A tile of two segments (every C4 tile): the cut is put at key TILE_WORDS / 2 when both halves fit a segment.
    // A key and its 13 probes differ in one bit, so in the segment of half h an entry whose key lies in h finds ALL its
    // partners there but the one of bit 11, and an entry of the other half only that one: 13 probes per entry and tile
    // instead of 26 (a chunk of one kind takes 12 probes or 1, wave-uniformly; the one mixed chunk of a tile all 13 —
    // the clamped offsets make every probe right in any segment).  Other tiles are cut by entry count.
    bool aligned = false;
    uint32_t mid = 0;
    if (T.nQ > QSEG) {
        mid = (uint32_t)__builtin_amdgcn_readfirstlane((int)(L.count_qoff()[TILE_WORDS / 2] - T.q0));
        aligned = mid <= QSEG && T.nQ - mid <= QSEG;   // (then 0 < mid < nQ: both segments hold entries)
    }
    tile_frames(T, W.U);
    const uint32_t nchunks = (T.nT + TCH - 1) / TCH;
    const uint32_t ch_first = W.wv, ch_step = WAVES;   // every chunk of the tile is this workgroup's
    K34Chunk next = chunk_first(T, W, ch_first, nchunks);
    unsigned long long hits_acc = 0;   // the tile's exact hit count, this wavefront's share
    for (uint32_t qs = 0, qe; qs < T.nQ; qs = qe) {
        qe = aligned ? (qs ? T.nQ : mid) : min(qs + QSEG, T.nQ);
        const uint32_t half = qs ? 1u : 0u;   // aligned tiles: the half of the key space this segment holds
        __syncthreads();  // every wavefront is through with the previous segment (and with the count prologue's use of the frame area)
        stage_segment(L, W.U, T, ro, qs, qe);
        __syncthreads();
        for (uint32_t ch = ch_first; ch < nchunks; ch += ch_step) {
            const uint32_t e0 = ch * TCH, ne = min(TCH, T.nT - e0);
            const K34Chunk C = next;
            chunk_ahead(next, T, W, ch, ch_first, ch_step, nchunks, qe < T.nQ);
            const bool tvalid = W.lane < ne;
            // my entry's in-tile key from its own frame: hi plane, seed window = frame bits 109 .. 127 (hi3 = f2.y)
            uint32_t w = 0;
            if (tvalid) w = pext12(C.f2.y >> 13);
            const int nn = A.transitions ? SEED_WEIGHT + 1 : 1;
            // the probes this chunk needs in this segment: all of them, or — aligned tiles, a chunk whose keys lie in one half of
            // the key space (all but one chunk of a tile) — the key itself and its partners of bits 0 .. 10 when that is the
            // segment's half, else the partner of bit 11 alone
            int jlo = 0, jhi = nn;
            if (aligned) {
                const uint64_t in_half = __ballot(tvalid && (w >> 11) == half), in_other = __ballot(tvalid && (w >> 11) != half);
                if (!in_other) jhi = min(nn, SEED_WEIGHT);
                else if (!in_half) jlo = SEED_WEIGHT;
            }
            jlo = __builtin_amdgcn_readfirstlane(jlo);   // (wave-uniform by construction: say so)
            jhi = __builtin_amdgcn_readfirstlane(jhi);
            emit_levels(A, L, W, T, C, tvalid, w, jlo, jhi, e0, qs, hits_acc);
        }
    }
    if (W.lane == 0 && hits_acc) atomicAdd(&A.q.tile_hits[(size_t)W.U.unit * NTILE + T.tile], hits_acc);
}

// a workgroup of the first pass: its tile of its unit, then the pairs its wavefronts still hold staged.  (Each pass creates its
// K34Wave itself: handed in by reference from the kernel, the split pass's loop spilled 9 to 11 VGPRs instead of 5.)
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void first_pass(const FusedArgs &A, uint8_t *smem) {
    K34Wave W = wave_open(A, blockIdx.y);
    const K34Lds<THREADS, QSEG> L(smem, W.wv);
    first_pass_tile(A, L, W);
    if (W.n_walk) walk_flush<false>(A, W, L.s_walk, W.n_walk);
}

// Split pass, one part of a listed tile: the target chunk groups p, p + pt, ... against the query entries [qa, qb); 32-bit offsets
struct K34Part { uint32_t p, pt, qa, qb; };
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void split_part(const FusedArgs &A, const K34Lds<THREADS, QSEG> &L, K34Wave &W, const uint32_t tile, const K34Part &P) {
    constexpr int WAVES = THREADS / 64, NRO = k34_nro<THREADS>();
    K34Tile T;
    if (!tile_open(T, W.U, tile)) return;
    // my share of the tile's query offsets: from the offset array
    uint32_t ro[NRO];
#pragma unroll
    for (int i = 0; i < NRO; i++) {
        const uint32_t k = threadIdx.x + (uint32_t)i * THREADS;
        ro[i] = 0;
        if (k <= TILE_WORDS) ro[i] = T.qoff[k] - T.q0;
    }
    tile_frames(T, W.U);
    const uint32_t nchunks = (T.nT + TCH - 1) / TCH;
    const uint32_t ch_first = P.p * WAVES + W.wv, ch_step = P.pt * WAVES;   // the chunks of my share of the tile
    K34Chunk next = chunk_first(T, W, ch_first, nchunks);
    unsigned long long hits_acc = 0;   // the tile's exact hit count, this wavefront's share
    const uint32_t q_end = min(P.qb, T.nQ);
    for (uint32_t qs = P.qa, qe; qs < q_end; qs = qe) {
        qe = min(qs + QSEG, q_end);
        __syncthreads();  // every wavefront is through with the previous segment
        stage_segment(L, W.U, T, ro, qs, qe);
        __syncthreads();
        for (uint32_t ch = ch_first; ch < nchunks; ch += ch_step) {
            const uint32_t e0 = ch * TCH, ne = min(TCH, T.nT - e0);
            const K34Chunk C = next;
            chunk_ahead(next, T, W, ch, ch_first, ch_step, nchunks, qe < q_end);
            const bool tvalid = W.lane < ne;
            // my entry's in-tile key from its own frame: hi plane, seed window = frame bits 109 .. 127 (hi3 = f2.y)
            uint32_t w = 0, c = 0, nmask = 0, dmask = 0;
            if (tvalid) w = pext12(C.f2.y >> 13);
            const int nn = A.transitions ? SEED_WEIGHT + 1 : 1;
            count_probes(L.sQ, tvalid, w, nn, c, nmask, dmask);
            emit_lane_major(A, L, W, T, C, w, c, nmask, e0, qs, hits_acc);
            emit_dense(A, L, W, T, C, w, dmask, e0, qs, hits_acc);
        }
    }
    if (W.lane == 0 && hits_acc) atomicAdd(&A.q.tile_hits[(size_t)W.U.unit * NTILE + T.tile], hits_acc);
}
// Split pass: persistent workgroups; the parts of the listed tiles are handed out by a counter until none is left (every
// workgroup reaches the end: the loop bound is the plan's part count, fixed before this launch)
template <int THREADS, uint32_t QSEG>
__device__ __forceinline__ void split_pass(const FusedArgs &A, uint8_t *smem) {
    K34Wave W = wave_open(A, 0u);   // (the unit comes with the part)
    const K34Lds<THREADS, QSEG> L(smem, W.wv);
    __shared__ uint32_t s_part;
    const uint32_t nparts = A.plan.ctr[2], ntiles = A.plan.ctr[1];
    for (;;) {
        __syncthreads();   // the part before is finished in every wavefront (s_part, the tile's offsets and frames are free)
        if (threadIdx.x == 0) s_part = atomicAdd(&A.plan.ctr[0], 1u);
        __syncthreads();
        const uint32_t g = s_part;
        if (g >= nparts) break;
        // the listed tile that holds part g: base[k] <= g < base[k + 1]
        uint32_t lo = 0, hi = ntiles;
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (A.plan.base[mid] <= g) lo = mid; else hi = mid;
        }
        const uint2 ut = A.plan.tile[lo];
        const uint4 sp = A.plan.split[lo];
        const uint32_t part = g - A.plan.base[lo];
        if (W.n_walk && ut.x != W.ai) { walk_flush<true>(A, W, L.s_walk, W.n_walk); W.n_walk = 0; }   // the staged hits belong to the unit before
        W.ai = ut.x;
        W.U = A.units[W.ai];
        W.part_no = part;
        const uint32_t qa = (part / sp.x) * sp.z;
        split_part(A, L, W, ut.y, K34Part{part % sp.x, sp.x, qa, qa + sp.z});
    }
    if (W.n_walk) walk_flush<true>(A, W, L.s_walk, W.n_walk);
}

// HEAVY = the split pass
template <int THREADS, uint32_t QSEG, bool HEAVY>
__global__ __launch_bounds__(THREADS, 4) void k34_scan_extend(FusedArgs A) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    if constexpr (HEAVY) split_pass<THREADS, QSEG>(A, smem);
    else first_pass<THREADS, QSEG>(A, smem);
}

// one workgroup per unit: unit_hits[u] = sum of its tile counts (once per batch)
__global__ __launch_bounds__(256) void k34_sum_hits(const unsigned long long *__restrict__ tile_hits, unsigned long long *__restrict__ unit_hits) {
    __shared__ unsigned long long red[256];
    unsigned long long s = 0;
    for (uint32_t i = threadIdx.x; i < NTILE; i += 256) s += tile_hits[(size_t)blockIdx.x * NTILE + i];
    red[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) red[threadIdx.x] += red[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) unit_hits[blockIdx.x] = red[0];
}
void launch_sum_hits(const ExtQueues &q, uint32_t nunits, hipStream_t st) {
    hipLaunchKernelGGL(k34_sum_hits, dim3(nunits), dim3(256), 0, st, (const unsigned long long *)q.tile_hits, q.unit_hits);
}

// The plan of the split pass, one workgroup for the whole launch (a few thousand listed tiles; the worst case, every tile of every
// unit listed, is a few milliseconds): the units' lists made dense, every tile cut into parts of about PART_HITS hits — target chunk
// groups (512 entries: one chunk per wavefront of a workgroup) dealt round-robin over Pt shares, query entries in ranges of a
// multiple of 64 — and the parts' prefix sum.
__global__ __launch_bounds__(1024) void k34_plan(const FusedUnit *__restrict__ units, uint32_t nunits, ExtQueues q, HeavyPlan P) {
    __shared__ uint32_t s_scan[1024];
    __shared__ uint32_t s_carry, s_tiles;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) { s_carry = 0; s_tiles = 0; }
    __syncthreads();
    for (uint32_t u = 0; u < nunits; u++) {
        const uint32_t nlist = (uint32_t)min((unsigned long long)NTILE, q.nheavy_u[u]);
        const GFusedUnit U = units[u];
        for (uint32_t i0 = 0; i0 < nlist; i0 += 1024) {
            const uint32_t i = i0 + tid;
            uint32_t parts = 0, pt = 1, pq = 1, qlen = 0, tile = 0;
            if (i < nlist) {
                tile = q.heavy[(size_t)u * NTILE + i];
                const unsigned long long est = P.est[(size_t)u * NTILE + i];
                const gptr<uint32_t> toff = U.T.off + (size_t)tile * TILE_WORDS, qoff = U.Q.off + (size_t)tile * TILE_WORDS;
                const uint32_t nT = toff[TILE_WORDS] - toff[0], nQ = qoff[TILE_WORDS] - qoff[0];
                const uint32_t want = (uint32_t)min((unsigned long long)(1u << 20), (est + PART_HITS - 1) / PART_HITS);
                const uint32_t groups = max(1u, (nT + 511u) / 512u);
                pt = min(groups, max(1u, want));
                const uint32_t need_q = max(1u, (want + pt - 1) / pt);
                qlen = max(64u, (((nQ + need_q - 1) / need_q) + 63u) & ~63u);
                pq = max(1u, (nQ + qlen - 1) / qlen);
                parts = pt * pq;
            }
            // exclusive scan of the parts over the 1024 lanes, carried from iteration to iteration
            s_scan[tid] = parts;
            __syncthreads();
            for (uint32_t o = 1; o < 1024; o <<= 1) {
                const uint32_t v = tid >= o ? s_scan[tid - o] : 0u;
                __syncthreads();
                s_scan[tid] += v;
                __syncthreads();
            }
            if (i < nlist) {
                const uint32_t k = s_tiles + (i - i0);
                P.tile[k] = make_uint2(u, tile);
                P.split[k] = make_uint4(pt, pq, qlen, 0u);
                P.base[k] = s_carry + s_scan[tid] - parts;
            }
            __syncthreads();
            if (tid == 1023) { s_carry += s_scan[1023]; s_tiles += min(1024u, nlist - i0); }
            __syncthreads();
        }
    }
    if (tid == 0) { P.base[s_tiles] = s_carry; P.ctr[0] = 0; P.ctr[1] = s_tiles; P.ctr[2] = s_carry; }
}

constexpr uint32_t QSEG_FIRST = 1280, QSEG_HEAVY = 1024;
constexpr size_t LDS_FIRST = K34Lds<512, QSEG_FIRST>::BYTES, LDS_HEAVY = K34Lds<512, QSEG_HEAVY>::BYTES;

// ---- K34's host side: its buffers and its launches --------------------------------------------------------------------------
// The split pass's tile lists (estimate + number per slot, NTILE slots per unit), its plan for one launch (dense tiles: splits,
// tiles, part bases; three counters) and the per-unit counters (eight walk-queue shards, then the listed tiles).
int K34Buffers::prepare(const std::vector<FusedUnit> &units, ExtQueues &q, hipStream_t st) {
    nactive = (uint32_t)units.size();
    const size_t slots = (size_t)std::min(nactive, K34_LAUNCH_UNITS) * NTILE;
    int rc;
    if ((rc = counters.reserve((size_t)nactive * 9 * 8)) || (rc = lists.reserve((size_t)nactive * NTILE * 12)) || (rc = plan_buf.reserve(slots * 28 + 4096))) return rc;
    q.heavy_est = (unsigned long long *)lists.p;
    q.heavy = (uint32_t *)(q.heavy_est + (size_t)nactive * NTILE);
    plan.est = q.heavy_est;
    plan.split = (uint4 *)plan_buf.p;                       // slots * 16
    plan.tile = (uint2 *)(plan.split + slots);              // slots * 8
    plan.base = (uint32_t *)(plan.tile + slots);            // (slots + 1) * 4
    plan.ctr = (unsigned int *)(plan.base + slots + 4);     // 3 counters
    q.nwalk_u = (unsigned long long *)counters.p;
    q.nheavy_u = q.nwalk_u + (size_t)nactive * 8;
    HIP_TRY(hipMemsetAsync(counters.p, 0, (size_t)nactive * 9 * 8, st));
    return 0;
}
int K34Buffers::split_stats(unsigned int *tiles, unsigned int *slots, unsigned int *parts, unsigned long long *part_hits) const {
    unsigned int pc[3] = {0, 0, 0};
    if (nactive) HIP_TRY(hipMemcpy(pc, plan.ctr, 12, hipMemcpyDeviceToHost));
    *tiles = pc[1]; *slots = nactive * (unsigned)NTILE; *parts = pc[2]; *part_hits = PART_HITS;
    return 0;
}
void K34Buffers::release() {
    for (DeviceBuf *b : {&lists, &plan_buf, &counters}) b->release();
    plan = {}; nactive = 0;
}

// the two instantiations may use their LDS: set exactly once (the library may be driven from any one thread at a time)
static hipError_t allow_lds() {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(k34_scan_extend<512, QSEG_FIRST, false>), hipFuncAttributeMaxDynamicSharedMemorySize,
                                             (int)LDS_FIRST);
    if (e != hipSuccess) return e;
    return hipFuncSetAttribute(reinterpret_cast<const void *>(k34_scan_extend<512, QSEG_HEAVY, true>), hipFuncAttributeMaxDynamicSharedMemorySize,
                               (int)LDS_HEAVY);
}
// the units u0 .. of the batch as one launch sees them: its kernels count units from 0
static FusedArgs launch_view(FusedArgs A, const K34Buffers &K, uint32_t u0) {
    A.units += u0;
    A.q.nwalk_u += (size_t)u0 * 8; A.q.nheavy_u += u0; A.q.heavy += (size_t)u0 * NTILE; A.q.heavy_est += (size_t)u0 * NTILE;
    A.plan = K.plan;
    A.plan.est = A.q.heavy_est;
    return A;
}

// the heavy phase of a batch: the K.nactive units of the table d_units, both passes
int launch_fused_batch(const K34Buffers &K, const FusedUnit *d_units, const ExtQueues &q, const mimeo_params *p, hipStream_t st, uint32_t dbg) {
    if (!K.nactive) return 0;
    FusedArgs A;
    A.units = d_units; A.q = q;
    A.xdrop = p->xdrop; A.hspthresh = p->hspthresh; A.transitions = p->transitions;
    A.dbg = dbg;   // MIMEO_K34_DEBUG, read once per batch by the caller
    static const hipError_t attr_err = allow_lds();
    HIP_TRY(attr_err);
    // measured on a C4 unit (two segments per tile at 1280, three at 1216 and 1024): 1.44 / 1.51 / 1.54 ms for the heavy phase
    for (uint32_t u0 = 0; u0 < K.nactive; u0 += K34_LAUNCH_UNITS) {
        const uint32_t nu = std::min(K34_LAUNCH_UNITS, K.nactive - u0);
        const FusedArgs B = launch_view(A, K, u0);
        hipLaunchKernelGGL((k34_scan_extend<512, QSEG_FIRST, false>), dim3(NTILE, nu), dim3(512), LDS_FIRST, st, B);
        hipLaunchKernelGGL(k34_plan, dim3(1), dim3(1024), 0, st, B.units, nu, B.q, B.plan);
        hipLaunchKernelGGL((k34_scan_extend<512, QSEG_HEAVY, true>), dim3(HEAVY_GRID), dim3(512), LDS_HEAVY, st, B);
    }
    return 0;
}

}  // namespace mimeo
