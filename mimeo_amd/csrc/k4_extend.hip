// K4 — gap-free x-drop extension of seed hits into HSPs with lastz's per-diagonal "already
// extended" suppression, --entropy and --hspthresh (reference call site
// src/mimeo/wrappers.py:1031-1032 `--gfextend --entropy --hspthresh=H`).
//
// lastz resolves the suppression sequentially (one diagonal-extent array updated while the
// query is scanned).  The same result is obtained here without ordering the hit flood
// (DESIGN.md §4, K4):
//   * heavy kernel, one launch per unit — K34 (k34_fused.hip: seed scan, pre-filter and exact walks in one
//     kernel, no hit array) or, for A/B checks, k4_extend_hits below on the hit array of the stand-alone K3 join.
//     A hit is walked left from its seed end; the walk also looks, bit-parallel, for an earlier seed hit on its
//     own diagonal whose seed end lies at a position it reached.  If there is none the hit is a HEAD: no earlier
//     extension can cover it, so it is certainly extended by the sequential process; the lane finishes the
//     extension and emits a candidate HSP if it scores >= hspthresh.  Otherwise the hit is a FOLLOWER and only
//     (unit, diagonal, seed end, nearest earlier seed end) is kept.
//   * ONCE PER BATCH of units (the reference's per-pair loop, wrappers.py:1015-1059, issues these per pair):
//     walks that outlive the frame (k4_extend_generic, then k4_extend_long: one wavefront per hit, wave-level
//     prefix sums); the followers of ALL units are radix-sorted by (unit, diagonal, seed end) in one sort; a run in
//     which each names its predecessor is a segment owned by the head in front of it; k4_resolve_small /
//     k4_resolve_segments replay lastz's rule inside each segment (extend, skip everything whose seed end <=
//     reach, extend the next one, ...); k4_entropy applies the entropy adjustment and the threshold.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>
#include <utility>

#include <rocprim/rocprim.hpp>

#include "k34.h"
#include "k4_queue.h"

namespace mimeo {

// ---- walks that outlive the frame of the heavy kernel: one lane per hit, windows loaded on demand -------------
__global__ __launch_bounds__(EXT_THREADS) void k4_extend_generic(const UnitDesc *__restrict__ units, ExtQueues q, int xdrop,
                                                              int hspthresh, int transitions,
                                                              const uint32_t *__restrict__ group_tab) {
    __shared__ uint32_t tab[GROUP_TAB];
    for (int i = threadIdx.x; i < GROUP_TAB; i += EXT_THREADS) tab[i] = group_tab[i];
    __syncthreads();
    const ShardMap hits(q.ctr->nmed8, q.med_cap);   // the hits come in eight shards (counts produced by the heavy kernels)
    const uint64_t nhits = hits.total();
    // What a hit leaves — a follower record, a place in the long queue or a candidate — waits in LDS until the wavefront has 64
    // of a kind: appended lane by lane where the walks end, these were three same-address atomics per wavefront and step
    // (~13 ns each: the duration of this kernel on a batch with 3 * 10^7 such hits)
    constexpr int GCAP = 64;
    __shared__ FollowerSink<>::Lds<GCAP> s_fol[EXT_THREADS / 64];
    __shared__ LongSink::Lds<GCAP> s_long[EXT_THREADS / 64];
    __shared__ CandSink::Lds<GCAP> s_cd[EXT_THREADS / 64];
    const uint32_t wv = threadIdx.x >> 6, lane = threadIdx.x & 63u;
    WaveQueue<FollowerSink<>, GCAP> fol(FollowerSink<>{q, 0u}, s_fol[wv]);
    WaveQueue<LongSink, GCAP> lng(LongSink{q}, s_long[wv]);
    WaveQueue<CandSink, GCAP> cd(CandSink{q}, s_cd[wv]);
    const uint64_t stride = (uint64_t)gridDim.x * EXT_THREADS;
    for (uint64_t g0 = (uint64_t)blockIdx.x * EXT_THREADS + wv * 64u; g0 < nhits; g0 += stride) {   // wave-uniform bound
        const uint64_t gid = g0 + lane;
        bool o_fol = false, o_long = false, o_cd = false;
        FollowRec r_f{0, 0};
        uint32_t unit = 0;
        uint2 h = make_uint2(0, 0);
        Cand r_cd{0, 0, 0, 0, 0};
        if (gid < nhits) {
            const uint64_t at = hits.slot(gid);
            const uint4 rec = q.medq[at];
            h = make_uint2(rec.x, rec.y);
            unit = q.medu[at];
            const Resume rs = unpack_resume(rec.z, rec.w);
            const GStrandView T = units[unit].T, Q = units[unit].Q;
            const int32_t et = (int32_t)h.x + SEED_LEN, eq = (int32_t)h.y + SEED_LEN;
            const int32_t d = (int32_t)h.x - (int32_t)h.y;
            // The walk kernel has served FRAME_STEPS steps of the walk that is alive (two windows): both walks go on from
            // what it reached, at window RESUME_WIN.  LONG_WINDOWS counts from the seed as before.
            constexpr int RESUME_WIN = (int)(FRAME_STEPS / 32);
            // ---- left walk, with detection of an earlier seed hit at every reached boundary (right alive: it is
            // finished, best and bk are in the record)
            WalkState L{rs.kind ? 0 : rs.run, rs.kind ? rs.lbest : rs.best, rs.kind ? rs.lbk : rs.bk, rs.kind ? 0u : FRAME_STEPS, rs.kind != 0, false, 0};
            const uint32_t maxl = (uint32_t)min(et, eq);
            bool is_long = false;
            for (int win = RESUME_WIN; !L.done; win++) {
                if (win == LONG_WINDOWS) { is_long = true; break; }
                const int32_t P = et - 32 * (win + 1) - SEED_LEN, Pq = P - d;
                const Win64 tw = win64(T, P), qw = win64(Q, Pq);
                const uint64_t dl64 = tw.lo ^ qw.lo, dh64 = tw.hi ^ qw.hi, nm64 = dl64 | dh64;
                const uint32_t nlo = (uint32_t)nm64, nhi = (uint32_t)(nm64 >> 32);
                const uint32_t tlo = (uint32_t)dl64, thi = (uint32_t)(dl64 >> 32);
                // seed hits among the 32 starts P .. P+31: care positions carry at most one non-match,
                // and it must be a transition (dl = 0)
                uint32_t ones = 0, twos = 0, tv = 0;
#pragma unroll
                for (int c = 0; c < SEED_LEN; c++) {
                    if (!((CARE19 >> c) & 1u)) continue;
                    const uint32_t v = c ? __builtin_amdgcn_alignbit(nhi, nlo, c) : nlo;
                    twos |= ones & v;
                    ones |= v;
                    tv |= c ? __builtin_amdgcn_alignbit(thi, tlo, c) : tlo;
                }
                const uint32_t bad = transitions ? (twos | tv) : ones;
                const uint32_t H = ~bad & seedvalid32(T, P, (uint32_t)tw.sv) & (uint32_t)qw.sv;
                // walk bits in step order: step s <-> position P + 19 + 31 - s
                walk_window(tab, L, __brev((uint32_t)(dl64 >> SEED_LEN)), __brev((uint32_t)(dh64 >> SEED_LEN)),
                            __brev((uint32_t)((tw.lo ^ tw.hi) >> SEED_LEN)), __brev((uint32_t)((tw.nm | qw.nm) >> SEED_LEN)),
                            __brev(H), maxl, xdrop);
            }
            if (!is_long && L.found) {
                o_fol = true;
                r_f.key = follow_key(q, unit, d, Q.len, (uint32_t)et);
                r_f.prev = (uint32_t)et - L.found_step;  // position of the base just summed = that seed's end
            } else {
                // ---- right walk: from the seed end, or (right alive) from the record
                WalkState R{rs.kind ? rs.run : 0, rs.kind ? rs.best : 0, rs.kind ? rs.bk : 0u, rs.kind ? FRAME_STEPS : 0u, false, false, 0};
                if (!is_long) {
                    const uint32_t maxr = min(T.len - (uint32_t)et, Q.len - (uint32_t)eq);
                    for (int win = rs.kind ? RESUME_WIN : 0; !R.done; win++) {
                        if (win == LONG_WINDOWS) { is_long = true; break; }
                        const int32_t P = et + 32 * win, Pq = P - d;
                        const Win32 tw = win32(T, P), qw = win32(Q, Pq);
                        walk_window(tab, R, tw.lo ^ qw.lo, tw.hi ^ qw.hi, tw.lo ^ tw.hi, tw.nm | qw.nm, 0u, maxr, xdrop);
                    }
                }
                if (is_long) o_long = true;
                else {
                    const int32_t score = L.best + R.best;
                    if (score >= hspthresh) { o_cd = true; r_cd = Cand{(uint32_t)et - L.bk, (uint32_t)eq - L.bk, L.bk + R.bk, score, unit}; }
                }
            }
        }
        fol.push(o_fol, r_f);
        lng.push(o_long, LongRec{h, unit});
        cd.push(o_cd, r_cd);
    }
    fol.flush();
    lng.flush();
    cd.flush();
}

// ---- heavy kernel of the A/B path: the hit array of the stand-alone K3 join, one lane per hit ----------------
// VARIANT 9 / 5: pre-filter with checkpoints every 16 steps, reading the two-plane copy (9: neither strand holds
// an N) or the full planes (5); 1 = no pre-filter, every hit is walked.  The production heavy kernel is K34
// (k34_fused.hip); this one is kept so that two independent decompositions of the stage can be compared byte for
// byte at full size (MIMEO_HEAVY=v1, tests/test_gpu_hsp.py).
template <int VARIANT>
__device__ __forceinline__ void extend_hits_body(const GStrandView &T, const GStrandView &Q,
                                                 const uint2 *__restrict__ hits, uint64_t nhits,
                                                 int xdrop, int hspthresh, int transitions,
                                                 const uint32_t *__restrict__ group_tab, const ExtQueues &q, uint32_t unit,
                                                 int skip_diag0, const unsigned long long *__restrict__ nhits_dev) {
    constexpr bool FILTER = VARIANT == 5 || VARIANT == 9;
    constexpr int SCAP = 256;   // staged followers per wavefront: one same-address atomic per 256 records
    constexpr int MCAP = 128;   // ... and generic-walk records, 16 bytes each with the walk's state: the 16 KiB that 256 bare hits took
    // nhits_dev: the hits are the walk queue of this unit, filled by K34 just before on the same stream: eight shards of
    // capacity `nhits` each, the counts on the device
    const ShardMap walkq = nhits_dev ? ShardMap(nhits_dev, nhits) : ShardMap();
    if (nhits_dev) nhits = walkq.total();
    __shared__ uint32_t tab[GROUP_TAB];
    __shared__ GenericSink::Lds<MCAP> s_med[FAST_THREADS / 64];
    __shared__ FollowerSink<true>::Lds<SCAP> s_fol[FAST_THREADS / 64];
    __shared__ CandSink::Lds<QCAP> s_cd[FAST_THREADS / 64];
    __shared__ uint2 s_walk[FILTER ? FAST_THREADS / 64 : 1][QCAP];  // hits that passed the pre-filter, per wavefront
    for (int i = threadIdx.x; i < GROUP_TAB; i += FAST_THREADS) tab[i] = group_tab[i];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63u, wv = threadIdx.x >> 6;
    const uint64_t lt_mask = (1ull << lane) - 1ull;
    WaveQueue<GenericSink, MCAP> med(GenericSink{q, unit}, s_med[wv]);
    WaveQueue<FollowerSink<true>, SCAP> fol(FollowerSink<true>{q, unit}, s_fol[wv]);
    WaveQueue<CandSink, QCAP> cd(CandSink{q}, s_cd[wv]);
    uint32_t n_walk = 0, n_walked = 0;  // wave-uniform fill levels

    auto walk_batch = [&](bool active, uint2 h) {
        bool q_med = false, q_fol = false, q_cd = false;
        FollowRec r_f{0, 0};
        Cand r_cd{0, 0, 0, 0, 0};
        uint2 r_st = make_uint2(0, 0);
        if (active) walk_hit(tab, T, Q, h, xdrop, hspthresh, transitions, q_med, r_st, q_fol, q_cd, r_f, r_cd);
        r_cd.unit = unit;
        med.push(q_med, make_uint4(h.x, h.y, r_st.x, r_st.y));
        fol.push(q_fol, r_f);
        cd.push(q_cd, r_cd);
    };

    const uint64_t stride = (uint64_t)gridDim.x * FAST_THREADS;
    for (uint64_t g0 = (uint64_t)blockIdx.x * FAST_THREADS + wv * 64u; g0 < nhits; g0 += stride) {
        const uint64_t gid = g0 + lane;
        uint2 h = make_uint2(0, 0);
        if (gid < nhits) h = hits[nhits_dev ? walkq.slot(gid) : gid];
        // a walk-queue entry that K34's first pass has put through its sharp filter already (WALK_SHARP_DONE) is not filtered
        // again; the mark comes off before anything else uses the position
        const bool marked = nhits_dev && (h.x & WALK_SHARP_DONE) != 0;
        if (nhits_dev) h.x &= POS_MASK;
        const bool valid = gid < nhits && !(skip_diag0 && h.x == h.y);  // the main diagonal of a self unit belongs to k4_diag0
        if (!FILTER) {
            walk_batch(valid, h);
        } else {
            bool need = valid && marked;
            // (no lane with an unmarked entry — every wavefront of a queue the first pass filled alone: the filter and its
            // thirteen loads are skipped wave-uniformly)
            if (__ballot(valid && !marked)) {
                if (valid && !marked)
                    need = VARIANT == 9 ? hit_needs_walk<16, true>(T, Q, h, xdrop, hspthresh, transitions)
                                        : hit_needs_walk<16, false>(T, Q, h, xdrop, hspthresh, transitions);
            }
            const uint64_t m = __ballot(need);
            if (m) {
                const uint32_t add = (uint32_t)__popcll(m);
                if (n_walk + add > (uint32_t)QCAP) {  // walk what is queued (nearly a full wavefront), then queue
                    __builtin_amdgcn_wave_barrier();
                    const uint2 hq = s_walk[wv][lane < n_walk ? lane : 0];
                    walk_batch(lane < n_walk, hq);
                    n_walked += n_walk;
                    n_walk = 0;
                    __builtin_amdgcn_wave_barrier();
                }
                if (need) s_walk[wv][n_walk + __popcll(m & lt_mask)] = h;
                n_walk += add;
            }
        }
    }
    if (FILTER && n_walk) {
        __builtin_amdgcn_wave_barrier();
        const uint2 hq = s_walk[wv][lane < n_walk ? lane : 0];
        walk_batch(lane < n_walk, hq);
        n_walked += n_walk;
    }
    // the statistic: one atomic per WORKGROUP (a same-address atomic serialises at ~13 ns: one per wavefront was 13 us of a
    // 190 us launch)
    __shared__ unsigned int s_nwalked;
    if (FILTER) {
        if (threadIdx.x == 0) s_nwalked = 0;
        __syncthreads();
        if (n_walked && lane == 0) atomicAdd(&s_nwalked, n_walked);
        __syncthreads();
        if (threadIdx.x == 0 && s_nwalked) atomicAdd(&q.ctr->nwalked, (unsigned long long)s_nwalked);
    }
    med.flush();
    fol.flush();
    cd.flush();
    if (!nhits_dev && blockIdx.x == 0 && threadIdx.x == 0) q.unit_hits[unit] = nhits;
}
// the hit array of ONE unit (A/B path: K3's join)
template <int VARIANT>
__global__ __launch_bounds__(FAST_THREADS) void k4_extend_hits(StrandView T, StrandView Q, const uint2 *__restrict__ hits, uint64_t nhits,
                                                              int xdrop, int hspthresh, int transitions,
                                                              const uint32_t *__restrict__ group_tab, ExtQueues q, uint32_t unit, int skip_diag0) {
    extend_hits_body<VARIANT>(T, Q, hits, nhits, xdrop, hspthresh, transitions, group_tab, q, unit, skip_diag0, nullptr);
}
// the walk queues of ALL units of the batch in one launch (grid.y = unit): a unit's region holds eight shards of walk_cap
// entries, filled by K34 just before on the same stream, the counts on the device
template <int VARIANT>
__global__ __launch_bounds__(FAST_THREADS) void k4_walk_batch(const FusedUnit *__restrict__ funits, int xdrop, int hspthresh, int transitions,
                                                             const uint32_t *__restrict__ group_tab, ExtQueues q) {
    const FusedUnit &U = funits[blockIdx.y];
    const GStrandView T = U.Tv, Q = U.Qv;   // out of the table: global address space from here on (device_util.h)
    extend_hits_body<VARIANT>(T, Q, q.walkq + U.walk_base, U.walk_cap, xdrop, hspthresh, transitions, group_tab, q, U.unit, 0,
                              q.nwalk_u + (size_t)blockIdx.y * 8);
}

// the walk queues of the batch: total entries, and the fullest shard in 1/1024 of its capacity (> 1024: an overflow, the
// batch is repeated with larger regions)
__global__ __launch_bounds__(256) void k4_walk_summary(const FusedUnit *__restrict__ funits, uint32_t nactive, const unsigned long long *__restrict__ nwalk_u,
                                                       ExtCounters *ctr) {
    unsigned long long tot = 0, worst = 0;
    for (uint32_t i = blockIdx.x * 256 + threadIdx.x; i < nactive * 8u; i += gridDim.x * 256) {
        const unsigned long long n = nwalk_u[i], cap = funits[i >> 3].walk_cap;
        tot += n;
        worst = max(worst, cap ? (n * 1024ull + cap - 1) / cap : (n ? 1ull << 40 : 0ull));
    }
    for (int o = 32; o > 0; o >>= 1) { tot += __shfl_xor(tot, o); worst = max(worst, (unsigned long long)__shfl_xor(worst, o)); }
    if ((threadIdx.x & 63) == 0) { if (tot) atomicAdd(&ctr->nwalk_total, tot); if (worst) atomicMax(&ctr->nwalk_over, worst); }
}

// ---- long hits, one wavefront each ------------------------------------------------------------------------
// (three wavefronts per SIMD fit its registers; the hits differ in length by orders of magnitude — a microsatellite diagonal
// against a few hundred bases — so a wavefront takes the next 16 hits from a counter instead of a fixed stride; records: RecordStage)
constexpr uint32_t CLAIM = 16;
__global__ __launch_bounds__(EXT_THREADS) void k4_extend_long(const UnitDesc *__restrict__ units, ExtQueues q, int xdrop,
                                                              int hspthresh, int transitions) {
    __shared__ RecordStage::Lds s_stage[EXT_THREADS / 64];
    RecordStage S(q, s_stage[threadIdx.x >> 6]);
    const uint64_t nlong = min((uint64_t)q.ctr->nlong, q.long_cap);
    for (;;) {
        const uint64_t w0 = wave_claim(&q.ctr->long_next, CLAIM);
        if (w0 >= nlong) break;
        for (uint64_t wid = w0; wid < min(nlong, w0 + CLAIM); wid++) {
            const uint32_t unit = q.longu[wid];
            S.push(wave_extend_record(units[unit].T, units[unit].Q, q.longq[wid], xdrop, hspthresh, transitions, true, q, unit, nullptr));
        }
    }
    S.flush();
}

// ---- the follower shards gathered into one array (input of the sort) ---------------------------------------------
__global__ __launch_bounds__(256) void k4_compact_followers(ExtQueues q, uint64_t *__restrict__ key, uint32_t *__restrict__ prev) {
    const ShardMap fol(q.ctr->nfollow8, q.follow_cap);
    const uint64_t n = fol.total();
    if (blockIdx.x == 0 && threadIdx.x == 0) q.ctr->nfollow = n;
    for (uint64_t gid = (uint64_t)blockIdx.x * 256 + threadIdx.x; gid < n; gid += (uint64_t)gridDim.x * 256) {
        const uint64_t at = fol.slot(gid);
        key[gid] = q.fkey[at];
        prev[gid] = q.fprev[at];
    }
}

// ---- follower segments --------------------------------------------------------------------------------------
// flag[i] = 1 iff sorted follower i starts a segment (its predecessor is a head, not follower i-1)
__global__ void k4_segment_flags(const uint64_t *__restrict__ key, const uint32_t *__restrict__ prev, uint64_t n,
                                 ExtQueues q, uint8_t *__restrict__ flag) {
    uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    bool start = true;
    if (i > 0) {
        uint64_t a = key[i - 1], b = key[i];
        // a RUN_END record closes the run its predecessor in the list opened (or continued): never a segment start
        start = prev[i] != RUN_END && (key_unit_diag(q, a) != key_unit_diag(q, b) || key_end(q, a) != prev[i]);
    }
    flag[i] = start ? 1 : 0;
}

// One LANE per segment: almost every segment is a pair of neighbouring random hits (one head, one
// follower, walks of a few dozen bases).  Segments with more than SMALL_SEG members or with a walk
// longer than LONG_WINDOWS windows are queued for k4_resolve_segments (one wavefront each).
constexpr uint32_t SMALL_SEG = 8;
__global__ __launch_bounds__(EXT_THREADS) void k4_resolve_small(const UnitDesc *__restrict__ units, ExtQueues q,
                                                                const uint64_t *__restrict__ key,
                                                                const uint32_t *__restrict__ prev, uint64_t nfollow,
                                                                const uint64_t *__restrict__ seg_start,
                                                                const uint64_t *__restrict__ nseg_dev,
                                                                int xdrop, int hspthresh,
                                                                const uint32_t *__restrict__ group_tab,
                                                                uint64_t *__restrict__ bigseg) {
    __shared__ uint32_t tab[GROUP_TAB];
    const uint64_t nseg = *nseg_dev;
    if ((uint64_t)blockIdx.x * EXT_THREADS >= nseg) return;  // the grid is sized for the followers, segments are fewer
    for (int i = threadIdx.x; i < GROUP_TAB; i += EXT_THREADS) tab[i] = group_tab[i];
    __syncthreads();
    const uint64_t sid = (uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x;
    if (sid >= nseg) return;
    const uint64_t beg = seg_start[sid], end = sid + 1 < nseg ? seg_start[sid + 1] : nfollow;
    bool big = end - beg > SMALL_SEG;
    Cand out[SMALL_SEG];
    uint32_t nout = 0;
    const uint32_t unit = key_unit(q, key[beg]);
    if (!big) {
        const GStrandView T = units[unit].T, Q = units[unit].Q;
        const int32_t d = key_diag(q, key[beg], Q.len);
        const int32_t het = (int32_t)prev[beg];
        WalkState H{0, 0, 0, 0, false, false, 0};
        big = !lane_walk(tab, T, Q, het, d, +1, min(T.len - (uint32_t)het, Q.len - (uint32_t)(het - d)), xdrop, H);
        uint32_t reach = (uint32_t)het + H.bk;
        for (uint64_t i = beg; i < end && !big; i++) {
            // the positions this record stands for: its own seed end, or — a RUN_END record — every one behind the record before it
            const uint32_t hi = key_end(q, key[i]);
            const uint32_t lo = prev[i] == RUN_END ? key_end(q, key[i - 1]) + 1u : hi;
            for (uint32_t et = max(lo, reach + 1u); et <= hi && !big; et = reach + 1u) {   // the next one beyond the region the previous extension reached
                const int32_t eq = (int32_t)et - d;
                WalkState L{0, 0, 0, 0, false, false, 0}, R{0, 0, 0, 0, false, false, 0};
                if (nout == SMALL_SEG ||
                    !lane_walk(tab, T, Q, (int32_t)et, d, -1, (uint32_t)min((int32_t)et, eq), xdrop, L) ||
                    !lane_walk(tab, T, Q, (int32_t)et, d, +1, min(T.len - et, Q.len - (uint32_t)eq), xdrop, R)) {
                    big = true;
                    break;
                }
                if (L.best + R.best >= hspthresh) out[nout++] = Cand{et - L.bk, (uint32_t)eq - L.bk, L.bk + R.bk, L.best + R.best, unit};
                reach = et + R.bk;
            }
        }
    }
    if (big) {  // nothing has been emitted for this segment yet: the wavefront kernel redoes it
        bigseg[wave_slot(&q.ctr->nbig)] = sid;
        return;
    }
    for (uint32_t k = 0; k < nout; k++) append_now(CandSink{q}, out[k]);
}

// one wavefront per segment: replay "skip while seed end <= reach, else extend" (lastz diagEnd rule)
__global__ __launch_bounds__(EXT_THREADS) void k4_resolve_segments(const UnitDesc *__restrict__ units, ExtQueues q,
                                                                   const uint64_t *__restrict__ key,
                                                                   const uint32_t *__restrict__ prev, uint64_t nfollow,
                                                                   const uint64_t *__restrict__ seg_start,
                                                                   const uint64_t *__restrict__ nseg_dev,
                                                                   const uint64_t *__restrict__ list, int xdrop,
                                                                   int hspthresh, int transitions) {
    const uint64_t nseg = *nseg_dev, nlist = q.ctr->nbig;
    __shared__ RecordStage::Lds s_stage[EXT_THREADS / 64];
    RecordStage S(q, s_stage[threadIdx.x >> 6]);
    for (;;) {   // segments differ in size by orders of magnitude: the next 16 from a counter
        const uint64_t w0 = wave_claim(&q.ctr->seg_next, CLAIM);
        if (w0 >= nlist) break;
        // the heads of the 16 segments, one per lane: four dependent loads for all of them instead of four for each
        uint64_t l_beg = 0, l_end = 0, l_k0 = 0;
        uint32_t l_het = 0;
        if ((threadIdx.x & 63u) < CLAIM && w0 + (threadIdx.x & 63u) < nlist) {
            const uint64_t sid = list[w0 + (threadIdx.x & 63u)];
            l_beg = seg_start[sid];
            l_end = sid + 1 < nseg ? seg_start[sid + 1] : nfollow;
            l_k0 = key[l_beg];
            l_het = prev[l_beg];
        }
        for (uint64_t wid = w0; wid < min(nlist, w0 + CLAIM); wid++) {
            const int src = (int)(wid - w0);
            uint64_t beg = __shfl(l_beg, src), end = __shfl(l_end, src);
            uint64_t k0 = __shfl(l_k0, src);
            const uint32_t unit = key_unit(q, k0);
            const GStrandView T = units[unit].T, Q = units[unit].Q;
            const int32_t d = key_diag(q, k0, Q.len);
            // head: seed end = prev[beg]; only its right extent matters (it was emitted by the heavy kernel or the walks)
            int32_t het = (int32_t)__shfl(l_het, src);
            WalkResult R = wave_walk_fast(T, Q, het, d, +1, min(T.len - (uint32_t)het, Q.len - (uint32_t)(het - d)), xdrop);
            uint32_t reach = (uint32_t)het + R.bsteps;
            uint64_t i = beg;
            while (i < end) {
                // first record at or after i that reaches beyond `reach` (records are sorted by seed end; a RUN_END record stands for
                // every position behind the record before it up to its own)
                // (the next 64 records in one load, lane by lane — most segments end there; a binary search, one memory round trip per
                // step, only behind them)
                uint64_t nxt;
                {
                    const uint64_t x = i + (threadIdx.x & 63u);
                    const uint64_t m = __ballot(x < end && key_end(q, key[x]) > reach);
                    if (m) nxt = i + (uint64_t)__builtin_ctzll(m);
                    else {
                        uint64_t lo = min(end, i + 64u), hi = end;
                        while (lo < hi) {
                            uint64_t mid = (lo + hi) >> 1;
                            if (key_end(q, key[mid]) > reach) hi = mid; else lo = mid + 1;
                        }
                        nxt = lo;
                    }
                }
                if (nxt >= end) break;
                uint32_t et = key_end(q, key[nxt]);
                if (prev[nxt] == RUN_END) et = max(key_end(q, key[nxt - 1]) + 1u, reach + 1u);   // the first member of the run beyond the reach
                uint2 h = make_uint2(et - SEED_LEN, (uint32_t)((int32_t)et - d) - SEED_LEN);
                uint32_t rext = 0;
                S.push(wave_extend_record(T, Q, h, xdrop, hspthresh, transitions, false, q, unit, &rext));
                reach = et + rext;
                i = nxt;   // the same record again: a run may hold more members beyond the new reach (a plain record is passed by the search)
            }
        }
    }
    S.flush();
}

// ---- the main diagonal of a strand aligned to itself ---------------------------------------------------------
// When target and query are the same strand every valid seed position is a hit on diagonal 0
// (millions of followers of one head).  The heavy kernel leaves those hits alone and this kernel replays the
// sequential rule directly on the seed-validity planes with one wavefront per self unit: extend the first seed,
// skip every seed whose end lies inside the reach, extend the next one, ...
__global__ __launch_bounds__(64) void k4_diag0(const UnitDesc *__restrict__ units, const uint32_t *__restrict__ selfs, ExtQueues q,
                                               int xdrop, int hspthresh, int transitions) {
    const uint32_t unit = selfs[blockIdx.x];
    const GStrandView T = units[unit].T, Q = units[unit].Q;
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t nwords = (T.len + 31u) >> 5;
    uint32_t p = 0;  // first seed start still to be considered
    for (;;) {
        uint32_t found = 0xFFFFFFFFu;
        for (uint32_t w0 = p >> 5; w0 < nwords; w0 += 64u) {
            const uint32_t w = w0 + lane;
            uint32_t m = 0;
            if (w < nwords) {
                m = (T.svt ? T.svt[w] : T.pw[w].w) & Q.pw[w].w;
                if (w == (p >> 5)) m &= 0xFFFFFFFFu << (p & 31u);
            }
            const uint64_t b = __ballot(m != 0);
            if (b) {
                const int l = __builtin_ctzll(b);
                const uint32_t mm = (uint32_t)__shfl((int)m, l);
                found = ((w0 + (uint32_t)l) << 5) + (uint32_t)__builtin_ctz(mm);
                break;
            }
        }
        if (found == 0xFFFFFFFFu) break;
        uint32_t rext = 0;
        wave_extend_emit(T, Q, make_uint2(found, found), xdrop, hspthresh, transitions, false, q, unit, &rext);
        const uint32_t reach = found + SEED_LEN + rext;  // a later seed is extended iff its end lies beyond
        p = max(found + 1u, reach - (uint32_t)(SEED_LEN - 1));
    }
}

// ---- entropy adjustment + threshold: eight lanes per candidate ------------------------------------------------
// A C4 row has 1.5 M candidates, nearly all of them 30-300 columns long: a group of eight lanes takes one (256
// columns per step, reductions over three xor-shuffles), so a wavefront finishes eight candidates at a time; the
// few long ones (the main diagonal of a self unit: millions of columns) just take more steps of their group.
constexpr uint32_t ENT_LANES = 8;
constexpr uint32_t ENT_LONG = 1u << 16;     // columns: longer candidates (the main diagonal of a self unit: the whole scaffold) ...
constexpr uint32_t ENT_BIGCAP = 4096;       // ... are counted by the whole grid (k4_entropy_big), up to this many per batch
constexpr int ENT_STAGE = 64;        // HSPs a wavefront collects before it appends them (8 per step at most)

// the columns of 32 consecutive positions of a gap-free segment; valid: the positions that belong to it
__device__ __forceinline__ uint32_t valid_columns(uint32_t rem) { return rem < 32 ? (1u << rem) - 1u : 0xFFFFFFFFu; }
// ... the identical ones, per base
template <class C>
__device__ __forceinline__ void column_counts(const Win32 &tw, const Win32 &qw, uint32_t valid, C (&cnt)[4]) {
    const uint32_t m = valid & ~((tw.lo ^ qw.lo) | (tw.hi ^ qw.hi)) & ~(tw.nm | qw.nm);
    cnt[0] += __popc(m & ~tw.lo & ~tw.hi);
    cnt[1] += __popc(m & tw.lo & ~tw.hi);
    cnt[2] += __popc(m & ~tw.lo & tw.hi);
    cnt[3] += __popc(m & tw.lo & tw.hi);
}
// ... and their HOXD70 sum, for a segment whose score does not fit 32 bits (RAW_SATURATED)
__device__ __forceinline__ int64_t column_score64(const Win32 &tw, const Win32 &qw, uint32_t valid) {
    const uint32_t nn = (tw.nm | qw.nm) & valid, ok = valid & ~nn, dl = (tw.lo ^ qw.lo) & ok, dh = (tw.hi ^ qw.hi) & ok;
    const uint32_t cg = tw.lo ^ tw.hi;
    return 91ll * __popc(ok) + 9ll * __popc(ok & ~(dl | dh) & cg) - 122ll * __popc(~dl & dh) - 205ll * __popc(dl) - 9ll * __popc(dl & dh) -
           2ll * __popc(dl & dh & cg) - 100ll * __popc(nn);
}
// lastz's --entropy: the raw score times the Shannon entropy (base 4) of the identical columns' bases, in 1/65536
template <class C>
__device__ __forceinline__ int64_t entropy_adjust(int64_t raw, const C (&cnt)[4], int entropy) {
    if (!entropy) return raw;
    const uint64_t n = (uint64_t)cnt[0] + cnt[1] + cnt[2] + cnt[3];
    double hh = 0.0;
    if (n) {
        for (int b = 0; b < 4; b++)
            if (cnt[b]) { double p = (double)cnt[b] / (double)n; hh -= p * log(p); }
        hh /= log(4.0);
    }
    int64_t q16 = (int64_t)floor(hh * 65536.0 + 0.5);
    q16 = q16 > 65536 ? 65536 : (q16 < 0 ? 0 : q16);
    return (raw * q16) >> 16;
}
__device__ __forceinline__ HspRec make_hsp(const Cand &c, int64_t adj, int64_t raw) {
    mimeo_hsp h;
    h.tstart = c.tstart; h.qstart = c.qstart; h.length = c.len; h.flags = 0; h.score = adj; h.raw_score = raw;
    return HspRec{h, c.unit};
}

__global__ __launch_bounds__(EXT_THREADS) void k4_entropy(const UnitDesc *__restrict__ units, ExtQueues q, int hspthresh,
                                                          int entropy, mimeo_hsp *__restrict__ out,
                                                          uint32_t *__restrict__ out_unit) {
    // The HSPs wait in LDS until the wavefront has 64 of them: one atomic per wavefront and STEP was 2.5 * 10^6 same-address
    // atomics for the 2.7 * 10^7 candidates of 32 C5 units — 13 ns each, the whole duration of this kernel
    __shared__ HspSink::Lds<ENT_STAGE> s_hsp[EXT_THREADS / 64];
    WaveQueue<HspSink, ENT_STAGE> hsps(HspSink{q, out, out_unit}, s_hsp[threadIdx.x >> 6]);
    const uint32_t sub = threadIdx.x & (ENT_LANES - 1u);
    const uint64_t ncand = min((uint64_t)q.ctr->ncand, q.cand_cap);
    const uint64_t ngroups = ((uint64_t)gridDim.x * EXT_THREADS) / ENT_LANES;
    // the loop bound is wave-uniform (rounded up to the wavefront's eight groups): the shuffles below need every lane
    const uint64_t first = (((uint64_t)blockIdx.x * EXT_THREADS + threadIdx.x) / 64) * (64 / ENT_LANES);
    for (uint64_t base = first; base < ncand; base += ngroups) {
        const uint64_t cid = base + (threadIdx.x & 63u) / ENT_LANES;
        const bool live = cid < ncand;
        Cand c = q.cand[live ? cid : ncand - 1];
        if (!live) c.len = 0;
        if (c.len > ENT_LONG) {   // one group of eight lanes would crawl through millions of columns with the wavefront waiting
            unsigned long long slot = ENT_BIGCAP;
            if (sub == 0) slot = wave_slot(&q.ctr->nbigcand);
            slot = __shfl(slot, (int)((threadIdx.x & 63u) & ~(ENT_LANES - 1u)));
            if (slot < ENT_BIGCAP) {
                if (sub == 0) q.bigcand[slot] = cid;
                c.len = 0;   // nothing to do here; k4_entropy_big emits it
            }
        }
        const bool deferred = live && c.len == 0;
        const GStrandView T = units[c.unit].T, Q = units[c.unit].Q;
        int64_t raw = c.raw;
        const int32_t d = (int32_t)c.tstart - (int32_t)c.qstart;
        // the longest candidate of the wavefront sets the number of steps (wave-uniform loops: shuffles inside)
        uint32_t maxlen = c.len;
        for (int o = 32; o >= (int)ENT_LANES; o >>= 1) maxlen = max(maxlen, (uint32_t)__shfl_xor((int)maxlen, o));
        if (__ballot(c.raw == RAW_SATURATED)) {  // recount the column scores of the segment in 64 bits (rare)
            int64_t sum = 0;
            for (uint32_t o0 = 0; o0 < maxlen; o0 += ENT_LANES * 32u) {
                const uint32_t o = o0 + sub * 32u;
                if (o < c.len && c.raw == RAW_SATURATED) {
                    const int32_t pt = (int32_t)(c.tstart + o);
                    sum += column_score64(win32(T, pt), win32(Q, pt - d), valid_columns(c.len - o));
                }
            }
            for (int o = ENT_LANES / 2; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
            if (c.raw == RAW_SATURATED) raw = sum;
        }
        uint32_t cnt[4] = {0, 0, 0, 0};
        if (entropy) {
            for (uint32_t o0 = 0; o0 < maxlen; o0 += ENT_LANES * 32u) {
                const uint32_t o = o0 + sub * 32u;
                if (o < c.len) {
                    const int32_t pt = (int32_t)(c.tstart + o);
                    column_counts(win32(T, pt), win32(Q, pt - d), valid_columns(c.len - o), cnt);
                }
            }
            for (int b = 0; b < 4; b++)
                for (int o = ENT_LANES / 2; o > 0; o >>= 1) cnt[b] += __shfl_xor(cnt[b], o);
        }
        const int64_t adj = entropy_adjust(raw, cnt, entropy);
        hsps.push(live && !deferred && adj >= hspthresh && sub == 0, make_hsp(c, adj, raw));   // at most one HSP per candidate
    }
    hsps.flush();
}

// the long candidates: every workgroup counts a slice (matched columns per base, and the raw score again in 64 bits
// when it had saturated), then one lane per candidate applies the same formula as k4_entropy
__global__ __launch_bounds__(256) void k4_entropy_big(const UnitDesc *__restrict__ units, ExtQueues q) {
    const uint64_t nbig = min((uint64_t)q.ctr->nbigcand, (uint64_t)ENT_BIGCAP);
    __shared__ unsigned long long red[5];
    for (uint64_t bi = blockIdx.y; bi < nbig; bi += gridDim.y) {
        const Cand c = q.cand[q.bigcand[bi]];
        const GStrandView T = units[c.unit].T, Q = units[c.unit].Q;
        const int32_t d = (int32_t)c.tstart - (int32_t)c.qstart;
        unsigned long long cnt[4] = {0, 0, 0, 0};
        long long sum = 0;
        for (uint64_t o = ((uint64_t)blockIdx.x * 256 + threadIdx.x) * 32u; o < c.len; o += (uint64_t)gridDim.x * 256 * 32u) {
            const int32_t pt = (int32_t)(c.tstart + o);
            const Win32 tw = win32(T, pt), qw = win32(Q, pt - d);
            const uint32_t valid = valid_columns((uint32_t)(c.len - o));
            column_counts(tw, qw, valid, cnt);
            sum += column_score64(tw, qw, valid);
        }
        if (threadIdx.x < 5) red[threadIdx.x] = 0;
        __syncthreads();
        for (int k = 0; k < 4; k++) {
            unsigned long long v = cnt[k];
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((threadIdx.x & 63) == 0) atomicAdd(&red[k], v);
        }
        {
            long long v = sum;
            for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
            if ((threadIdx.x & 63) == 0) atomicAdd(&red[4], (unsigned long long)v);
        }
        __syncthreads();
        if (threadIdx.x < 5) atomicAdd(&q.bigacc[bi * 5 + threadIdx.x], red[threadIdx.x]);
        __syncthreads();
    }
}
__global__ void k4_entropy_big_finish(ExtQueues q, int hspthresh, int entropy, mimeo_hsp *__restrict__ out, uint32_t *__restrict__ out_unit) {
    const uint64_t nbig = min((uint64_t)q.ctr->nbigcand, (uint64_t)ENT_BIGCAP);
    for (uint64_t bi = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; bi < nbig; bi += (uint64_t)gridDim.x * blockDim.x) {
        const Cand c = q.cand[q.bigcand[bi]];
        const unsigned long long *a = q.bigacc + bi * 5;
        const unsigned long long cnt[4] = {a[0], a[1], a[2], a[3]};
        const int64_t raw = c.raw == RAW_SATURATED ? (int64_t)a[4] : (int64_t)c.raw, adj = entropy_adjust(raw, cnt, entropy);
        if (adj >= hspthresh) append_now(HspSink{q, out, out_unit}, make_hsp(c, adj, raw));
    }
}

// ---- shared plus strand: the HSPs of unit u once more, transposed, for its mirror unit ------------------------------------
// (A, B, +) and (B, A, +) of a self job: every rule of the gap-free stage is symmetric in target and query (seed words
// and the one-transition rule, N, the x-drop walks, the per-diagonal "already extended" rule — a diagonal keeps its
// order under the swap —, entropy of the identical columns, HOXD70), so the HSP set of (B, A, +) is the set of (A, B, +)
// with tstart and qstart exchanged; the pipeline only pairs units when neither scaffold has soft-masked bases (lastz
// excludes them from TARGET seeding only).  ctr[0] counts the copies.
__global__ __launch_bounds__(256) void k4_mirror_hsps(mimeo_hsp *__restrict__ hsps, uint32_t *__restrict__ hsp_unit, uint64_t nh,
                                                      const uint32_t *__restrict__ mirror_dst, unsigned long long *__restrict__ ctr) {
    for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < nh; i += (uint64_t)gridDim.x * 256) {
        const uint32_t m = mirror_dst[hsp_unit[i]];
        if (m == NO_MIRROR) continue;
        const unsigned long long at = nh + wave_slot(ctr);
        mimeo_hsp h = hsps[i];
        const uint32_t t = h.tstart;
        h.tstart = h.qstart; h.qstart = t;
        hsps[at] = h;
        hsp_unit[at] = m;
    }
}

// ---- host orchestration ---------------------------------------------------------------------
static uint32_t *g_group_tab = nullptr;  // device copy of the 4-base group table (read-only)
static std::once_flag g_group_once;

const uint32_t *group_table_device() {
    std::call_once(g_group_once, [&] {
        std::vector<uint32_t> tab(GROUP_TAB);
        build_group_table(tab.data());
        if (hipMalloc((void **)&g_group_tab, GROUP_TAB * 4) != hipSuccess ||
            hipMemcpy(g_group_tab, tab.data(), GROUP_TAB * 4, hipMemcpyHostToDevice) != hipSuccess)
            g_group_tab = nullptr;
    });
    return g_group_tab;
}

// k4_extend_generic strides over its queue with every wavefront the device can hold at once: workgroups per CU as the
// runtime counts them for this kernel's registers and LDS (five on gfx950: 83 VGPRs, 27 KiB) times the CUs
static uint32_t g_generic_grid = 0;
static std::once_flag g_generic_once;
static uint32_t generic_grid() {
    std::call_once(g_generic_once, [&] {
        int dev = 0, cus = 0, per_cu = 0;
        if (hipGetDevice(&dev) == hipSuccess && hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess &&
            hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k4_extend_generic, EXT_THREADS, 0) == hipSuccess && cus > 0 && per_cu > 0)
            g_generic_grid = (uint32_t)cus * (uint32_t)per_cu;
        else {
            g_generic_grid = 1024;   // what the kernel ran with before it was sized: four wavefronts per SIMD of 256 CUs
            (void)hipGetLastError();
        }
        if (getenv("MIMEO_K4_STATS")) fprintf(stderr, "[k4] k4_extend_generic: %u workgroups (%d CUs x %d)\n", g_generic_grid, cus, per_cu);
    });
    return g_generic_grid;
}

static_assert(sizeof(Cand) == queue_plan::CAND_BYTES && sizeof(mimeo_hsp) == queue_plan::HSP_BYTES, "queue_plan.h prices the candidate and HSP slices with these sizes");

void ExtBatch::release() {
    for (DeviceBuf *b : {&units, &ctr, &nsel, &unit_hits, &tile_hits, &selfs, &hits, &bigcand, &bigacc, &mirror, &funits}) b->release();
    if (k34_) { k34_->release(); delete k34_; k34_ = nullptr; }
    for (DeviceBuf &b : qbuf) b.release();   // slices: nothing is freed here
    for (DeviceBuf &b : sbuf) b.release();
    arena_q.release(); arena_s.release();
    jc.release();
    for (auto &e : ev) { if (e) (void)hipEventDestroy(e); e = nullptr; }
    if (side_done) { (void)hipEventDestroy(side_done); side_done = nullptr; }
    if (side) { (void)hipStreamDestroy(side); side = nullptr; }
    delete q_; q_ = nullptr;
    started_ = false;
}

int ExtBatch::run(const std::vector<UnitWork> &work, const mimeo_params *p, uint64_t *nhsp_out, ExtStats *stats, const std::vector<uint32_t> *mirror_dst) {
    *nhsp_out = 0;
    const int rc = start(work, p, mirror_dst);
    return rc ? rc : finish(nhsp_out, stats);
}

static ExtSwitches read_switches() {
    ExtSwitches s;
    const char *e;
    s.v1 = (e = getenv("MIMEO_HEAVY")) && !strcmp(e, "v1");
    if ((e = getenv("MIMEO_K4_VARIANT"))) s.k4_variant = atoi(e);
    if ((e = getenv("MIMEO_K34_DEBUG"))) s.k34_dbg = (uint32_t)atoi(e);
    s.k4_stats = getenv("MIMEO_K4_STATS") != nullptr;
    if ((e = getenv("MIMEO_QUEUE_SHRINK")) && atof(e) > 0) s.shrink = atof(e);
    if ((e = getenv("MIMEO_QUEUE_BUDGET_MB"))) { s.budget_forced = true; s.budget_mb = atol(e); }
    s.trace = getenv("MIMEO_TRACE") != nullptr;
    return s;
}

// what the queues of the batch may take of the device's memory now
static int queue_budget(const ExtBatch &b, uint64_t *budget) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = queue_plan::queue_budget(free_b, b.arena_q.cap + b.arena_s.cap, b.sw_.budget_forced, b.sw_.budget_mb);
    return 0;
}

// The slices of an arena at these sizes, one behind the other.  An arena that is too small drops its slices and grows
// (queue_plan::arena_want; first_slack_div: the part of its size it takes on top the first time, 0: nothing); when the memory
// is not there a batch that can be cut is cut.
template <int N>
static int lay_out(DeviceBuf &arena, DeviceBuf (&slices)[N], const uint64_t (&bytes)[N], uint64_t headroom, uint64_t first_slack_div, bool splittable) {
    uint64_t off[N];
    const size_t total = queue_plan::place_slices(bytes, off);
    if (total > arena.cap) {
        for (DeviceBuf &s : slices) s.release();
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        const size_t want = queue_plan::arena_want(total, arena.cap, free_b, headroom, first_slack_div ? total / first_slack_div : 0);
        int rc = arena.reserve(want);
        if (rc && want > total) rc = arena.reserve(total);
        if (rc) return rc == MIMEO_ERR_NOMEM && splittable ? MIMEO_ERR_SPLIT : rc;
    }
    for (int i = 0; i < N; i++) slices[i].set_view((char *)arena.p + off[i], bytes[i]);
    return 0;
}

static queue_plan::Counts counts_of(const ExtCounters &c, uint64_t followers, uint64_t generic) {
    return queue_plan::Counts{followers, generic, c.nlong, c.ncand, c.nwalk_total, c.nwalk_over};
}

int ExtBatch::start(const std::vector<UnitWork> &work, const mimeo_params *p, const std::vector<uint32_t> *mirror_dst) {
    hipStream_t st = stream();
    started_ = false;
    const uint32_t nunits = (uint32_t)work.size();
    if (!nunits) return 0;
    w_ = work; p_ = *p;
    sw_ = read_switches();
    // a switch that is silently ignored would falsify someone's profile: the timing experiments of this word are gone
    if (sw_.k34_dbg & ~48u) { set_error("MIMEO_K34_DEBUG: only 16 (run members are kept) and 32 (no flush filter), or their sum, are switches"); return MIMEO_ERR_ARG; }
    uint64_t max_t = 0, max_q = 0;
    uint32_t launching = 0;
    expect_hits_ = 0;
    h_units_.resize(nunits);   // a member: the copy below is asynchronous
    h_selfs_.clear();
    walk_cap_u_.assign(nunits, 0);
    for (uint32_t u = 0; u < nunits; u++) {
        const UnitWork &w = work[u];
        if (w.d.T.len >= 0x7FFFFF00u || w.d.Q.len >= 0x7FFFFF00u) { set_error("scaffold longer than 2^31 bases"); return MIMEO_ERR_LIMIT; }
        h_units_[u] = w.d;
        max_t = std::max<uint64_t>(max_t, w.d.T.len); max_q = std::max<uint64_t>(max_q, w.d.Q.len);
        if (w.d.same) h_selfs_.push_back(u);
        if (!w.ti.n || !w.qi.n) continue;   // a mirror rider: expects no hits, launches nothing
        const double e = host_plan::expected_seed_hits(w.ti.n, w.qi.n);
        expect_hits_ += e;
        walk_cap_u_[u] = queue_plan::walk_cap(e, boost, sw_.shrink);
        launching++;
    }
    splittable_ = launching > 1;   // a batch can be cut in two when at least two of its units launch the heavy kernels (a rider stays with its source)
    mirror_dst_.clear();
    if (mirror_dst && std::any_of(mirror_dst->begin(), mirror_dst->end(), [](uint32_t m) { return m != NO_MIRROR; })) {
        if (mirror_dst->size() != nunits) { set_error("internal: mirror table of the wrong size"); return MIMEO_ERR_ARG; }
        mirror_dst_ = *mirror_dst;
    }
    key_ = queue_plan::follower_key_bits(max_t, max_q, nunits, SEED_LEN);
    if (!key_.fits) { set_error("internal: batch too large for the follower key"); return MIMEO_ERR_ARG; }
    if (!ev[0]) {
        for (auto &e : ev) HIP_TRY(hipEventCreate(&e));
        HIP_TRY(hipEventCreateWithFlags(&side_done, hipEventDisableTiming));
        HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    }
    int rc;
    if ((rc = units.reserve((size_t)nunits * sizeof(UnitDesc))) || (rc = ctr.reserve(sizeof(ExtCounters))) || (rc = unit_hits.reserve((size_t)nunits * 8)) ||
        (rc = nsel.reserve(16)) || (rc = tile_hits.reserve(sw_.v1 ? 8 : (size_t)nunits * NTILE * 8)) || (rc = bigcand.reserve((size_t)ENT_BIGCAP * 8)) ||
        (rc = bigacc.reserve((size_t)ENT_BIGCAP * 5 * 8)) || (rc = selfs.reserve((h_selfs_.size() + 1) * 4)))
        return rc;
    HIP_TRY(hipMemcpyAsync(units.p, h_units_.data(), (size_t)nunits * sizeof(UnitDesc), hipMemcpyHostToDevice, st));
    if (!h_selfs_.empty()) HIP_TRY(hipMemcpyAsync(selfs.p, h_selfs_.data(), h_selfs_.size() * 4, hipMemcpyHostToDevice, st));
    // queue capacities from the hit count expected on random sequence; a batch that does not fit them (repeat-rich units) is
    // repeated in finish() with room for everything the counters saw
    cap_ = queue_plan::initial_caps(expect_hits_, boost, sw_.shrink);
    walk_entries_ = queue_plan::walk_entries(walk_cap_u_);
    // a batch whose queues cannot fit is cut in two by the caller before anything is allocated
    uint64_t budget = 0;
    if ((rc = queue_budget(*this, &budget))) return rc;
    if (sw_.trace)
        fprintf(stderr, "[trace] batch of %u units, %.3g expected hits: queues %.2f GiB of %.2f GiB budget (boosts f %.1f m %.1f l %.1f c %.1f w %.1f; caps f %llu m %llu l %llu c %llu walk entries %llu)\n", nunits, expect_hits_,
                (double)queue_bytes() / (1 << 30), (double)budget / (1 << 30), boost.f, boost.m, boost.l, boost.c, boost.w,
                (unsigned long long)cap_.f, (unsigned long long)cap_.m, (unsigned long long)cap_.l, (unsigned long long)cap_.c, (unsigned long long)walk_entries_);
    if (queue_plan::must_split(splittable_, queue_bytes(), budget)) return MIMEO_ERR_SPLIT;
    if (!mirror_dst_.empty()) {
        if ((rc = mirror.reserve((size_t)nunits * 4 + 16))) return rc;
        HIP_TRY(hipMemcpyAsync(mirror.p, mirror_dst_.data(), (size_t)nunits * 4, hipMemcpyHostToDevice, st));
    }
    if (!q_) q_ = new ExtQueues();
    if ((rc = enqueue_heavy())) return rc;
    started_ = true;
    return 0;
}

// the queues of the batch: slices of the queue arena at the current capacities, and the kernels' view of them
int ExtBatch::carve_queues() {
    using namespace queue_plan;
    ExtQueues &q = *q_;
    memset(&q, 0, sizeof q);
    q.ebits = key_.ebits; q.dbits = key_.dbits;
    const int rc = lay_out(arena_q, qbuf, queue_slices(cap_, walk_entries_, !mirror_dst_.empty(), sw_.v1).bytes, queue_bytes() - arena_bytes() + QUEUE_ARENA_HEADROOM, 0, splittable_);
    if (rc) return rc;
    q.ctr = (ExtCounters *)ctr.p;
    q.cand = (Cand *)qbuf[Q_CAND].p; q.fkey = (uint64_t *)qbuf[Q_FKEY].p; q.fprev = (uint32_t *)qbuf[Q_FPREV].p;
    q.medq = (uint4 *)qbuf[Q_MEDQ].p; q.medu = (uint32_t *)qbuf[Q_MEDU].p; q.longq = (uint2 *)qbuf[Q_LONGQ].p; q.longu = (uint32_t *)qbuf[Q_LONGU].p;
    q.bigcand = (unsigned long long *)bigcand.p; q.bigacc = (unsigned long long *)bigacc.p;
    q.unit_hits = (unsigned long long *)unit_hits.p; q.tile_hits = (unsigned long long *)tile_hits.p;
    q.walkq = (uint2 *)qbuf[Q_WALKQ].p;
    q.cand_cap = cap_.c; q.follow_cap = cap_.f; q.med_cap = cap_.m; q.long_cap = cap_.l;
    return 0;
}

int ExtBatch::enqueue_heavy() {
    hipStream_t st = stream();
    const uint32_t nunits = (uint32_t)w_.size();
    if (!group_table_device()) { set_error("group table upload failed"); return MIMEO_ERR_HIP; }
    int rc;
    if ((rc = carve_queues())) return rc;
    HIP_TRY(hipMemsetAsync(ctr.p, 0, sizeof(ExtCounters), st));
    HIP_TRY(hipMemsetAsync(unit_hits.p, 0, (size_t)nunits * 8, st));
    if (!sw_.v1) HIP_TRY(hipMemsetAsync(tile_hits.p, 0, (size_t)nunits * NTILE * 8, st));   // K34 adds to it: a tile's pairs, wavefront by wavefront
    HIP_TRY(hipMemsetAsync(nsel.p, 0, 16, st));
    HIP_TRY(hipMemsetAsync(bigacc.p, 0, (size_t)ENT_BIGCAP * 5 * 8, st));
    HIP_TRY(hipEventRecord(ev[0], st));
    if (!h_selfs_.empty()) {   // the main diagonals of the self units: one wavefront each, beside the heavy kernels
        HIP_TRY(hipStreamWaitEvent(side, ev[0], 0));
        hipLaunchKernelGGL(k4_diag0, dim3((uint32_t)h_selfs_.size()), dim3(64), 0, side, (const UnitDesc *)units.p, (const uint32_t *)selfs.p, *q_, p_.xdrop, p_.hspthresh, p_.transitions);
        HIP_TRY(hipEventRecord(side_done, side));
    }
    if ((rc = sw_.v1 ? enqueue_v1() : enqueue_k34())) return rc;   // the heavy phase: nothing is read back
    HIP_TRY(hipEventRecord(ev[1], st));
    HIP_TRY(hipGetLastError());
    return 0;
}

// K34 over every unit of the batch in ONE launch (plus its split pass), then the hits it could not dismiss (3-4 % on random
// sequence, most of them false alarms of its cheap filter) through the sharp filter and the exact walk of round 1's fast
// kernel, again one launch for all units (grid.y = unit), then the walk-queue statistics and the hit counts per unit
int ExtBatch::enqueue_k34() {
    hipStream_t st = stream();
    const uint32_t *tab = group_table_device();
    ExtQueues &q = *q_;
    h_funits_.clear();   // a member: the copy below is asynchronous
    bool slim = true;
    uint64_t base = 0;
    for (uint32_t u = 0; u < (uint32_t)w_.size(); u++) {
        const UnitWork &w = w_[u];
        if (!w.ti.n || !w.qi.n) continue;
        FusedUnit f; memset(&f, 0, sizeof f);
        f.T = w.ti; f.Q = w.qi; f.Tv = w.d.T; f.Qv = w.d.Q; f.unit = u; f.same = w.d.same;
        f.walk_base = base; f.walk_cap = walk_cap_u_[u];
        base += queue_plan::SHARDS * f.walk_cap;
        slim = slim && !w.d.T.has_n && !w.d.Q.has_n;
        h_funits_.push_back(f);
    }
    const uint32_t nactive = nactive_ = (uint32_t)h_funits_.size();
    if (nactive) {
        int rc;
        if (!k34_) k34_ = new K34Buffers();
        if ((rc = funits.reserve((size_t)nactive * sizeof(FusedUnit))) || (rc = k34_->prepare(h_funits_, q, st)))
            return rc == MIMEO_ERR_NOMEM && splittable_ ? MIMEO_ERR_SPLIT : rc;
        HIP_TRY(hipMemcpyAsync(funits.p, h_funits_.data(), (size_t)nactive * sizeof(FusedUnit), hipMemcpyHostToDevice, st));
        HIP_TRY(hipEventRecord(ev[4], st));
        if ((rc = launch_fused_batch(*k34_, (const FusedUnit *)funits.p, q, &p_, st, sw_.k34_dbg))) return rc;
        HIP_TRY(hipEventRecord(ev[5], st));
        for (uint32_t u0 = 0; u0 < nactive; u0 += K34_LAUNCH_UNITS) {
            const uint32_t nu = std::min(K34_LAUNCH_UNITS, nactive - u0);
            ExtQueues qq = q;
            qq.nwalk_u = q.nwalk_u + (size_t)u0 * 8;
            const FusedUnit *fu = (const FusedUnit *)funits.p + u0;
            // a unit's queue is worked off by at most 256 workgroups (their end-of-kernel flushes are same-address
            // atomics: more workgroups cost more than they bring), fewer when many small units share the launch
            const uint32_t qblocks = std::max(1u, std::min(256u, (8192u + nu - 1) / nu));
            if (slim) hipLaunchKernelGGL(k4_walk_batch<9>, dim3(qblocks, nu), dim3(FAST_THREADS), 0, st, fu, p_.xdrop, p_.hspthresh, p_.transitions, tab, qq);
            else hipLaunchKernelGGL(k4_walk_batch<5>, dim3(qblocks, nu), dim3(FAST_THREADS), 0, st, fu, p_.xdrop, p_.hspthresh, p_.transitions, tab, qq);
        }
        hipLaunchKernelGGL(k4_walk_summary, dim3(std::min(256u, (nactive * 8u + 255u) / 256u)), dim3(256), 0, st, (const FusedUnit *)funits.p, nactive,
                           (const unsigned long long *)q.nwalk_u, q.ctr);
    }
    launch_sum_hits(q, (uint32_t)w_.size(), st);
    return 0;
}

// MIMEO_HEAVY=v1, the A/B path: per unit, materialise the hits (exact count: one round trip), then the round-1 fast kernel
int ExtBatch::enqueue_v1() {
    for (uint32_t u = 0; u < (uint32_t)w_.size(); u++) {
        const UnitWork &w = w_[u];
        if (!w.ti.n || !w.qi.n) continue;
        uint64_t nh = 0;
        const int rc = join_hits(jc, w.ti, w.qi, p_.transitions, hits, &nh, nullptr);
        if (rc) return rc;
        if (!nh) continue;
        const bool slim = !w.d.T.has_n && !w.d.Q.has_n;
        const auto kernel = sw_.k4_variant == 1 ? k4_extend_hits<1> : sw_.k4_variant == 5 || !slim ? k4_extend_hits<5> : k4_extend_hits<9>;
        hipLaunchKernelGGL(kernel, dim3((uint32_t)std::min<uint64_t>((nh + FAST_THREADS - 1) / FAST_THREADS, 1024)), dim3(FAST_THREADS), 0, stream(),
                           w.d.T, w.d.Q, (const uint2 *)hits.p, nh, p_.xdrop, p_.hspthresh, p_.transitions, group_table_device(), *q_, u, (int)w.d.same);
    }
    return 0;
}

// ---- the tails, once per batch: the steps of finish()
// walks beyond the frame; round trip 1: the follower count (sizes the sort) and the overflow check
int ExtBatch::tails(ExtCounters *c) {
    hipStream_t st = stream();
    const UnitDesc *d_units = (const UnitDesc *)units.p;
    HIP_TRY(hipStreamWaitEvent(st, ev[1], 0));   // the heavy phase may have run on another stream
    HIP_TRY(hipEventRecord(ev[3], st));
    hipLaunchKernelGGL(k4_extend_generic, dim3(generic_grid()), dim3(EXT_THREADS), 0, st, d_units, *q_, p_.xdrop, p_.hspthresh, p_.transitions, group_table_device());
    if (!h_selfs_.empty()) HIP_TRY(hipStreamWaitEvent(st, side_done, 0));
    hipLaunchKernelGGL(k4_extend_long, dim3(768), dim3(EXT_THREADS), 0, st, d_units, *q_, p_.xdrop, p_.hspthresh, p_.transitions);
    HIP_TRY(hipMemcpyAsync(c, ctr.p, sizeof *c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

// the nf followers of all units: gathered, sorted by (unit, diagonal, seed end), cut into segments and resolved
int ExtBatch::resolve_followers(uint64_t nf) {
    using namespace queue_plan;
    hipStream_t st = stream();
    const UnitDesc *d_units = (const UnitDesc *)units.p;
    const ExtQueues &q = *q_;
    // the sort's second buffers, flags, segment lists and rocPRIM's scratch: slices of the sort arena
    size_t t1 = 0, t2 = 0;
    rocprim::counting_iterator<uint64_t> iota(0);
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, t1, (uint64_t *)nullptr, (uint64_t *)nullptr, (uint32_t *)nullptr, (uint32_t *)nullptr, (size_t)nf, 0, key_.key_bits, st));
    HIP_TRY(rocprim::select(nullptr, t2, iota, (uint8_t *)nullptr, (uint64_t *)nullptr, (uint64_t *)nsel.p, (size_t)nf, st));
    const int rc = lay_out(arena_s, sbuf, sort_slices(nf, std::max(t1, t2)).bytes, SORT_ARENA_HEADROOM, 8, splittable_);
    if (rc) return rc;
    uint64_t *fkey = (uint64_t *)qbuf[Q_FKEY].p, *fkey2 = (uint64_t *)sbuf[S_FKEY2].p, *segs = (uint64_t *)sbuf[S_SEGS].p, *bigseg = (uint64_t *)sbuf[S_BIGSEG].p;
    uint32_t *fprev = (uint32_t *)qbuf[Q_FPREV].p, *fprev2 = (uint32_t *)sbuf[S_FPREV2].p;
    uint8_t *flags = (uint8_t *)sbuf[S_FLAGS].p;
    const uint64_t *nseg = (const uint64_t *)nsel.p;
    // the eight shards gathered into fkey2 / fprev2; the sort writes back into the (now free) shard area
    hipLaunchKernelGGL(k4_compact_followers, dim3(1024), dim3(256), 0, st, q, fkey2, fprev2);
    HIP_TRY(rocprim::radix_sort_pairs(sbuf[S_TMP].p, t1, fkey2, fkey, fprev2, fprev, (size_t)nf, 0, key_.key_bits, st));
    hipLaunchKernelGGL(k4_segment_flags, dim3((uint32_t)((nf + 255) / 256)), dim3(256), 0, st, (const uint64_t *)fkey, (const uint32_t *)fprev, nf, q, flags);
    HIP_TRY(rocprim::select(sbuf[S_TMP].p, t2, iota, flags, segs, (uint64_t *)nsel.p, (size_t)nf, st));
    // segments: at most nf of them; the kernels read the real number from nsel
    hipLaunchKernelGGL(k4_resolve_small, dim3((uint32_t)((nf + EXT_THREADS - 1) / EXT_THREADS)), dim3(EXT_THREADS), 0, st, d_units, q, (const uint64_t *)fkey,
                       (const uint32_t *)fprev, nf, (const uint64_t *)segs, nseg, p_.xdrop, p_.hspthresh, group_table_device(), bigseg);
    hipLaunchKernelGGL(k4_resolve_segments, dim3(1024), dim3(EXT_THREADS), 0, st, d_units, q, (const uint64_t *)fkey, (const uint32_t *)fprev, nf,
                       (const uint64_t *)segs, nseg, (const uint64_t *)bigseg, p_.xdrop, p_.hspthresh, p_.transitions);
    return 0;
}

// entropy and threshold; round trip 2: the HSP count (the resolution may have added candidates)
int ExtBatch::entropy(ExtCounters *c) {
    hipStream_t st = stream();
    const UnitDesc *d_units = (const UnitDesc *)units.p;
    hipLaunchKernelGGL(k4_entropy, dim3(1536), dim3(EXT_THREADS), 0, st, d_units, *q_, p_.hspthresh, p_.entropy, (mimeo_hsp *)hsps.p, (uint32_t *)hsp_unit.p);
    hipLaunchKernelGGL(k4_entropy_big, dim3(128, 16), dim3(256), 0, st, d_units, *q_);
    hipLaunchKernelGGL(k4_entropy_big_finish, dim3(16), dim3(256), 0, st, *q_, p_.hspthresh, p_.entropy, (mimeo_hsp *)hsps.p, (uint32_t *)hsp_unit.p);
    HIP_TRY(hipEventRecord(ev[2], st));
    HIP_TRY(hipMemcpyAsync(c, ctr.p, sizeof *c, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return 0;
}

int ExtBatch::print_stats(const ExtCounters &c, uint64_t nf, uint64_t nm, bool over) {
    if (sw_.k4_stats && k34_ && nactive_) {
        unsigned int tiles = 0, slots = 0, parts = 0;
        unsigned long long part_hits = 0;
        const int rc = k34_->split_stats(&tiles, &slots, &parts, &part_hits);
        if (rc) return rc;
        fprintf(stderr, "[k34] split pass: %u tiles listed of %u, %u parts of ~%llu hits\n", tiles, slots, parts, part_hits);
    }
    if (sw_.k4_stats)
        fprintf(stderr, "[k4] units %u walk queue %llu walked %llu generic %llu long %llu followers %llu candidates %llu hsps %llu%s\n", (uint32_t)w_.size(),
                c.nwalk_total, c.nwalked, (unsigned long long)nm, c.nlong, (unsigned long long)nf, c.ncand, c.nhsp, over ? "  (queue overflow: batch repeated)" : "");
    return 0;
}

// An overflow: the queues grow to hold what the counters saw; what the batch showed goes into the sizing of the next ones
// whatever happens to it now; and when the larger queues no longer fit the device the caller cuts the batch in two.
// fullest, batch: the counters (they count beyond the capacities), with the followers and generic walks of the fullest shard / that times eight
int ExtBatch::learn_and_grow(const queue_plan::Counts &fullest, const queue_plan::Counts &batch) {
    queue_plan::grow(cap_, walk_cap_u_, fullest);
    walk_entries_ = queue_plan::walk_entries(walk_cap_u_);
    queue_plan::learn(boost, batch, expect_hits_, sw_.shrink);
    uint64_t budget = 0;
    const int rc = queue_budget(*this, &budget);
    if (rc) return rc;
    if (sw_.trace)
        fprintf(stderr, "[trace] overflow of a batch of %u units: followers %llu (fullest shard), generic %llu, long %llu, cand %llu, walk %.2fx; queues would take %.2f GiB of %.2f GiB\n",
                (uint32_t)w_.size(), (unsigned long long)fullest.followers, (unsigned long long)fullest.generic, (unsigned long long)fullest.nlong, (unsigned long long)fullest.ncand,
                (double)fullest.nwalk_over / 1024.0, (double)queue_bytes() / (1 << 30), (double)budget / (1 << 30));
    return queue_plan::must_split(splittable_, queue_bytes(), budget) ? MIMEO_ERR_SPLIT : 0;
}

int ExtBatch::finish(uint64_t *nhsp_out, ExtStats *stats) {
    *nhsp_out = 0;
    if (!started_) return 0;
    started_ = false;
    hipStream_t st = stream();
    const uint32_t nunits = (uint32_t)w_.size();
    int rc;
    ExtCounters c;
    uint64_t nf = 0, nm = 0;
    // try; if a queue overflowed: learn, grow, maybe split, enqueue again; at most four repeats
    for (int attempt = 0;; attempt++) {
        if ((rc = tails(&c))) return rc;
        uint64_t maxf = 0, maxm = 0;
        nf = nm = 0;
        for (int r = 0; r < queue_plan::SHARDS; r++) {
            nf += std::min<uint64_t>(c.nfollow8[r], cap_.f); nm += std::min<uint64_t>(c.nmed8[r], cap_.m);
            maxf = std::max<uint64_t>(maxf, c.nfollow8[r]); maxm = std::max<uint64_t>(maxm, c.nmed8[r]);
        }
        bool over = queue_plan::over(cap_, counts_of(c, maxf, maxm));
        if (!over) {
            if ((nf && (rc = resolve_followers(nf))) || (rc = entropy(&c))) return rc;
            over = c.ncand > cap_.c;
        }
        HIP_TRY(hipGetLastError());
        if ((rc = print_stats(c, nf, nm, over))) return rc;
        if (!over) break;
        // (a walk queue that overflowed hides followers and candidates of the hits it dropped: the repeat may overflow those in turn)
        if (attempt >= 4) { set_error("extension queues overflowed four times in a row"); return MIMEO_ERR_LIMIT; }
        if (stats) stats->reruns++;
        if ((rc = learn_and_grow(counts_of(c, maxf, maxm), counts_of(c, queue_plan::SHARDS * maxf, queue_plan::SHARDS * maxm)))) return rc;
        if ((rc = enqueue_heavy())) return rc;   // the batch again, on this stream, with room
    }
    float ms_heavy = 0, ms_tails = 0, ms_walk = 0, ms_k34 = 0;
    HIP_TRY(hipEventElapsedTime(&ms_heavy, ev[0], ev[1]));
    HIP_TRY(hipEventElapsedTime(&ms_tails, ev[1], ev[2]));
    HIP_TRY(hipEventElapsedTime(&ms_walk, ev[1], ev[3]));
    if (!sw_.v1 && nactive_) HIP_TRY(hipEventElapsedTime(&ms_k34, ev[4], ev[5]));
    uint64_t nhsp = c.nhsp;
    if (!mirror_dst_.empty() && nhsp) {   // shared plus strand: the mirror units receive their (transposed) HSPs
        unsigned long long *mctr = (unsigned long long *)((char *)mirror.p + (size_t)nunits * 4 + (8 - ((size_t)nunits * 4) % 8) % 8);
        HIP_TRY(hipMemsetAsync(mctr, 0, 8, st));
        hipLaunchKernelGGL(k4_mirror_hsps, dim3((uint32_t)std::min<uint64_t>(1024, (nhsp + 255) / 256)), dim3(256), 0, st, (mimeo_hsp *)hsps.p,
                           (uint32_t *)hsp_unit.p, nhsp, (const uint32_t *)mirror.p, mctr);
        unsigned long long added = 0;
        HIP_TRY(hipMemcpyAsync(&added, mctr, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        nhsp += added;
    }
    h_unit_hits.resize(nunits);
    HIP_TRY(hipMemcpy(h_unit_hits.data(), unit_hits.p, (size_t)nunits * 8, hipMemcpyDeviceToHost));
    *nhsp_out = nhsp;
    queue_plan::learn(boost, counts_of(c, nf, nm), expect_hits_, sw_.shrink);   // a batch that fitted teaches too
    if (stats) {
        for (uint32_t u = 0; u < nunits; u++) {
            const UnitWork &w = w_[u];
            if (!(w.ti.n && w.qi.n)) continue;   // a mirror unit's seed scan is never run: it counts no hits and no bytes
            stats->seed_hits += h_unit_hits[u];
            const uint64_t Lq = w.d.Q.len, H = h_unit_hits[u];
            // B_scan = ceil(Lq/4) + 8*W*(Lq-18) + 4*H + 8*H, W = 13
            stats->scan_bytes_algorithmic += (Lq + 3) / 4 + (Lq > 18 ? 8ull * 13ull * (Lq - 18) : 0) + 12ull * H;
            // compulsory traffic of the fused kernel: both offset arrays, positions and frames of both sides once
            stats->scan_bytes_kernel += 2ull * 4ull * ((uint64_t)NBUCKET + 1) + 52ull * ((uint64_t)w.ti.n + w.qi.n);
            stats->heavy_launches++;   // units: the seed-scan kernel takes a batch of them per launch
        }
        if (!sw_.v1 && nactive_) stats->heavy_kernel_launches++;
        stats->walked += c.nwalked; stats->walk_queue += c.nwalk_total; stats->followers += nf; stats->candidates += c.ncand;
        stats->ms_heavy += ms_heavy; stats->ms_tails += ms_tails; stats->ms_walk += ms_walk; stats->ms_k34 += sw_.v1 ? ms_heavy : ms_k34;
    }
    return 0;
}

}  // namespace mimeo

