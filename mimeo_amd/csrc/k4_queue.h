// k4_queue.h — how the tail kernels of K4 (k4_extend.hip) read and fill the batch-wide queues of ExtQueues: the shard
// map, the wave-uniform claim of work from a counter, and the append — staged per wavefront in LDS (WaveQueue) or at
// once (append_now) — through one sink per queue.  The conventions every append keeps are written here once:
//   * the counter keeps counting past the capacity (the host sees an overflow as "counter > capacity" and repeats the
//     batch with room), the store is guarded by the capacity (sink_store);
//   * a busy queue is filled in eight shards, shard = queue_shard() = workgroup number mod 8, region r = [r * cap, ...)
//     (ShardMap::at); its readers see the shards as one flat range (ShardMap::slot);
//   * staged records are private to their wavefront; a wave barrier stands on both sides of the flush that lets other
//     lanes read them (WaveQueue::flush).
// K34's walk-queue flush (k34_fused.hip: walk_flush) filters inside its flush and is not built on this.
#pragma once
#include "k4_device.h"

namespace mimeo {

// ---- the eight shards of a queue as one flat range ---------------------------------------------------------------------
struct ShardMap {
    uint64_t end[8] = {0, 0, 0, 0, 0, 0, 0, 0};   // end[r] = entries in shards 0 .. r; what a shard counted beyond cap was not stored
    uint64_t cap = 0;
    ShardMap() = default;
    __device__ __forceinline__ ShardMap(const unsigned long long *__restrict__ count8, uint64_t shard_cap) : cap(shard_cap) {
        uint64_t acc = 0;
#pragma unroll
        for (int r = 0; r < 8; r++) { acc += min((uint64_t)count8[r], cap); end[r] = acc; }
    }
    __device__ __forceinline__ uint64_t total() const { return end[7]; }
    // flat index -> where that entry lies
    __device__ __forceinline__ uint64_t slot(uint64_t flat) const {
        uint32_t r = 0;
#pragma unroll
        for (int k = 0; k < 7; k++) r += flat >= end[k] ? 1u : 0u;
        uint64_t before = 0;   // entries in the shards in front of r: end[r - 1], by selects (a variable index would put end[] into scratch)
#pragma unroll
        for (int k = 0; k < 7; k++) before = r == (uint32_t)k + 1u ? end[k] : before;
        return at(r, cap, flat - before);
    }
    // ... and the inverse, for the writers: entry i of a shard
    static __device__ __forceinline__ uint64_t at(uint32_t shard, uint64_t shard_cap, uint64_t i) { return (uint64_t)shard * shard_cap + i; }
};

// the next n work items of a counter for this wavefront (items that differ in cost by orders of magnitude are handed out,
// not strided over): the wave-uniform start
__device__ __forceinline__ uint64_t wave_claim(unsigned long long *counter, uint32_t n) {
    unsigned long long w0 = 0;
    if ((threadIdx.x & 63u) == 0) w0 = atomicAdd(counter, (unsigned long long)n);
    return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(w0 >> 32)) << 32) | (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)w0);
}

// ---- sinks: one per queue ----------------------------------------------------------------------------------------------
// A sink names the queue's counter, its capacity (per shard when SHARDED), the record, how a record is stored at an index,
// and how CAP staged records lie in LDS (Lds<CAP>: structure of arrays where a struct would pad).
__device__ __forceinline__ uint64_t batch_key(const ExtQueues &q, uint32_t unit, uint64_t staged) {
    return ((uint64_t)unit << (q.dbits + q.ebits)) | ((staged >> 32) << q.ebits) | (staged & 0xFFFFFFFFull);
}
// followers.  COMPOSE: the key is staged as (diagonal + Q.len) << 32 | seed end (walk_hit) and gets its batch form — unit, bit
// widths — when it is stored
template <bool COMPOSE = false>
struct FollowerSink {
    using Rec = FollowRec;
    static constexpr bool SHARDED = true;
    template <int CAP> struct Lds {
        uint64_t key[CAP];
        uint32_t prev[CAP];
        __device__ __forceinline__ void put(uint32_t i, const Rec &r) { key[i] = r.key; prev[i] = r.prev; }
        __device__ __forceinline__ Rec get(uint32_t i) const { return Rec{key[i], prev[i]}; }
    };
    const ExtQueues &q;
    uint32_t unit;   // COMPOSE only
    __device__ __forceinline__ unsigned long long *counter() const { return &q.ctr->nfollow8[queue_shard()]; }
    __device__ __forceinline__ uint64_t cap() const { return q.follow_cap; }
    __device__ __forceinline__ void store(uint64_t at, const Rec &r) const { q.fkey[at] = COMPOSE ? batch_key(q, unit, r.key) : r.key; q.fprev[at] = r.prev; }
};
// hits whose walk outlives the frame (hit and walk state: pack_resume), of one unit
struct GenericSink {
    using Rec = uint4;
    static constexpr bool SHARDED = true;
    template <int CAP> struct Lds {
        uint4 rec[CAP];
        __device__ __forceinline__ void put(uint32_t i, const Rec &r) { rec[i] = r; }
        __device__ __forceinline__ Rec get(uint32_t i) const { return rec[i]; }
    };
    const ExtQueues &q;
    uint32_t unit;
    __device__ __forceinline__ unsigned long long *counter() const { return &q.ctr->nmed8[queue_shard()]; }
    __device__ __forceinline__ uint64_t cap() const { return q.med_cap; }
    __device__ __forceinline__ void store(uint64_t at, const Rec &r) const { q.medq[at] = r; q.medu[at] = unit; }
};
// hits whose walk outlives LONG_WINDOWS windows
struct LongRec { uint2 hit; uint32_t unit; };
struct LongSink {
    using Rec = LongRec;
    static constexpr bool SHARDED = false;
    template <int CAP> struct Lds {
        uint2 hit[CAP];
        uint32_t unit[CAP];
        __device__ __forceinline__ void put(uint32_t i, const Rec &r) { hit[i] = r.hit; unit[i] = r.unit; }
        __device__ __forceinline__ Rec get(uint32_t i) const { return Rec{hit[i], unit[i]}; }
    };
    const ExtQueues &q;
    __device__ __forceinline__ unsigned long long *counter() const { return &q.ctr->nlong; }
    __device__ __forceinline__ uint64_t cap() const { return q.long_cap; }
    __device__ __forceinline__ void store(uint64_t at, const Rec &r) const { q.longq[at] = r.hit; q.longu[at] = r.unit; }
};
struct CandSink {
    using Rec = Cand;
    static constexpr bool SHARDED = false;
    template <int CAP> struct Lds {
        Cand c[CAP];
        __device__ __forceinline__ void put(uint32_t i, const Rec &r) { c[i] = r; }
        __device__ __forceinline__ Rec get(uint32_t i) const { return c[i]; }
    };
    const ExtQueues &q;
    __device__ __forceinline__ unsigned long long *counter() const { return &q.ctr->ncand; }
    __device__ __forceinline__ uint64_t cap() const { return q.cand_cap; }
    __device__ __forceinline__ void store(uint64_t at, const Rec &r) const { q.cand[at] = r; }
};
// the HSPs of the batch and their units: at most one per candidate, the buffers hold cand_cap records
struct HspRec { mimeo_hsp h; uint32_t unit; };
struct HspSink {
    using Rec = HspRec;
    static constexpr bool SHARDED = false;
    template <int CAP> struct Lds {
        mimeo_hsp h[CAP];
        uint32_t unit[CAP];
        __device__ __forceinline__ void put(uint32_t i, const Rec &r) { h[i] = r.h; unit[i] = r.unit; }
        __device__ __forceinline__ Rec get(uint32_t i) const { return Rec{h[i], unit[i]}; }
    };
    const ExtQueues &q;
    mimeo_hsp *__restrict__ out;
    uint32_t *__restrict__ out_unit;
    __device__ __forceinline__ unsigned long long *counter() const { return &q.ctr->nhsp; }
    __device__ __forceinline__ uint64_t cap() const { return q.cand_cap; }
    __device__ __forceinline__ void store(uint64_t at, const Rec &r) const { out[at] = r.h; out_unit[at] = r.unit; }
};

// record r as entry i of the sink's queue (of this workgroup's shard): the one capacity guard
template <class Sink>
__device__ __forceinline__ void sink_store(const Sink &k, unsigned long long i, const typename Sink::Rec &r) {
    if (i < k.cap()) k.store(Sink::SHARDED ? ShardMap::at(queue_shard(), k.cap(), i) : i, r);
}
// appended at once, by every lane that calls this together: one atomic for them (wave_slot)
template <class Sink>
__device__ __forceinline__ void append_now(const Sink &k, const typename Sink::Rec &r) {
    sink_store(k, wave_slot(k.counter()), r);
}

// ---- the wave-staged append --------------------------------------------------------------------------------------------
// Records of one kind wait in a CAP-entry LDS array private to the wavefront, and one global atomic serves a whole flush
// (same-address atomics serialise at ~12-15 ns each; appended where they arise, the records of a batch cost millions of
// them).  n, the fill level, is wave-uniform.  A push takes the records of the lanes whose pred holds — at most CAP of
// them: every lane may push when CAP >= 64, below that the caller pushes from one lane — and flushes first when they would
// not fit; the kernel ends with an explicit flush().
template <class Sink, int CAP>
struct WaveQueue {
    using Rec = typename Sink::Rec;
    using Lds = typename Sink::template Lds<CAP>;
    const Sink sink;
    Lds &s;
    uint32_t n = 0;
    __device__ __forceinline__ WaveQueue(const Sink &k, Lds &lds) : sink(k), s(lds) {}
    __device__ __forceinline__ void push(bool pred, const Rec &r) {
        const uint64_t m = __ballot(pred);
        if (!m) return;
        const uint32_t add = (uint32_t)__popcll(m);
        if (n + add > (uint32_t)CAP) flush();
        if (pred) s.put(n + (uint32_t)__popcll(m & ((1ull << (threadIdx.x & 63u)) - 1ull)), r);
        n += add;
    }
    __device__ __forceinline__ void flush() {
        if (!n) return;
        const uint32_t lane = threadIdx.x & 63u;
        __builtin_amdgcn_wave_barrier();   // LDS accesses of one wavefront execute in order: the records are there
        unsigned long long b = 0;
        if (lane == 0) b = atomicAdd(sink.counter(), (unsigned long long)n);
        b = __shfl(b, 0);
        if constexpr (CAP <= 64) {
            if (lane < n) sink_store(sink, b + lane, s.get(lane));
        } else {
            for (uint32_t i = lane; i < n; i += 64) sink_store(sink, b + i, s.get(i));
        }
        n = 0;
        __builtin_amdgcn_wave_barrier();   // ... and read before the next push overwrites them
    }
};

// ---- what wave_extend_record leaves (valid in lane 0) ------------------------------------------------------------------
// ... staged: a wavefront's records wait until STAGE of a kind are there (a C5 batch has 3 * 10^6 long hits and as many large
// segments, and every one of them leaves a record)
constexpr int STAGE = 16;
struct RecordStage {
    struct Lds { FollowerSink<>::Lds<STAGE> fol; CandSink::Lds<STAGE> cd; };   // of one wavefront
    WaveQueue<FollowerSink<>, STAGE> fol;
    WaveQueue<CandSink, STAGE> cd;
    __device__ __forceinline__ RecordStage(const ExtQueues &q, Lds &s) : fol(FollowerSink<>{q, 0u}, s.fol), cd(CandSink{q}, s.cd) {}
    __device__ __forceinline__ void push(const HitRecord &r) {
        const bool lane0 = (threadIdx.x & 63u) == 0;
        fol.push(lane0 && r.kind == 1, r.f);
        cd.push(lane0 && r.kind == 2, r.c);
    }
    __device__ __forceinline__ void flush() { fol.flush(); cd.flush(); }
};
// ... or appended at once
__device__ __forceinline__ void wave_extend_emit(const GStrandView &T, const GStrandView &Q, uint2 h, int xdrop, int hspthresh,
                                                 int transitions, bool detect, const ExtQueues &q, uint32_t unit, uint32_t *rext_out) {
    const HitRecord r = wave_extend_record(T, Q, h, xdrop, hspthresh, transitions, detect, q, unit, rext_out);
    if ((threadIdx.x & 63) != 0) return;
    if (r.kind == 1) append_now(FollowerSink<>{q, 0u}, r.f);
    else if (r.kind == 2) append_now(CandSink{q}, r.c);
}

}  // namespace mimeo
