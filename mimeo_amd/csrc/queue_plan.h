// queue_plan.h — HIP-free sizing policy of the extension batch (ExtBatch, k4_extend.hip): how large the device queues are,
// what an overflow teaches and how the queues grow after one, how the two arenas are cut into slices and how they grow,
// what the queues may take of the device's memory, and how many units the follower key can name.  Every share, byte cost
// and growth rule is written here and nowhere else; tests/sanitize/queue_plan_check.cc holds it to a frozen restatement
// (tests/test_host_queue_plan.py).  The floating-point expressions keep their order of operations: the capacities are
// truncations of doubles, and a reordered product can move one by one.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace mimeo {
namespace queue_plan {

// ---- shares of the expected seed hits (host_plan::expected_seed_hits) that each queue receives on random sequence: 0.65 %
// of the hits are followers, ~1 % outlive the frame, 1e-4 become candidates, K34 passes ~4 % on to the walk queue
constexpr double SHARE_FOLLOW = 0.02, SHARE_GENERIC = 0.03, SHARE_LONG = 0.002, SHARE_CAND = 0.002, SHARE_WALK = 0.08;
constexpr int SHARDS = 8;                 // followers, generic walks and a unit's walk queue are filled in eight shards
constexpr double SHARD_SLACK = 1.5;       // ... sized per shard, with half as much again for their imbalance
constexpr double LEARN_SLACK = 1.5;       // a boost leaves half as much again over what was seen
constexpr double BOOST_MAX = 4096.0;
constexpr double LEARN_MIN_HITS = 1e6;    // smaller batches teach nothing: their shares are noise
constexpr uint64_t QUEUE_FLOOR = 1048576, WALK_FLOOR = 16384, CAP_PAD = 64;   // entries every queue / walk-queue shard has whatever is expected
constexpr uint64_t WALK_FULL = 1024;      // ExtCounters::nwalk_over: the fullest walk-queue shard in 1/1024 of its capacity

// ---- device bytes per entry
constexpr uint64_t CAND_BYTES = 20, HSP_BYTES = 32;   // sizeof(Cand), sizeof(mimeo_hsp): pinned where ExtBatch carves (k4_extend.hip)
constexpr uint64_t FKEY_BYTES = 8, FPREV_BYTES = 4;   // follower: key + predecessor
constexpr uint64_t MEDQ_BYTES = 16, LONGQ_BYTES = 8, UNIT_BYTES = 4;   // generic walk: hit + walk state; long walk: hit; the unit of either and of an HSP
constexpr uint64_t WALK_BYTES = 8, WALK_PAD = 8;      // walk-queue entry; bytes behind the last one (all there is of the slice under MIMEO_HEAVY=v1)
constexpr uint64_t SORT_BYTES_PER_FOLLOWER = 41;      // the sort arena at its worst: second key + predecessor buffers, flags, two segment lists, rocPRIM's scratch
constexpr uint64_t CHAIN_BYTES_PER_CAND = 260;        // chain / gapped scratch and alignment slots: ~200 per HSP, 60 more where k5_chain_wave meets large groups

// ---- boosts: the largest excess over the shares that an earlier batch of the call showed, per queue (a repeat-rich genome
// overflows the first batch once, not every batch)
struct Boosts { double f = 1.0, m = 1.0, l = 1.0, c = 1.0, w = 1.0; };
// what the counters of a batch reported.  followers / generic: batch-wide for learn(), the fullest shard for over() and grow()
struct Counts { uint64_t followers, generic, nlong, ncand, nwalk_total, nwalk_over; };

inline double learn_one(double boost, uint64_t seen, double share, double expect_hits) {
    return std::min(BOOST_MAX, std::max(boost, LEARN_SLACK * (double)seen / (share * expect_hits)));
}
inline void learn(Boosts &b, const Counts &s, double expect_hits, double shrink) {
    if (!(expect_hits > LEARN_MIN_HITS)) return;
    b.f = learn_one(b.f, s.followers, SHARE_FOLLOW, expect_hits);
    b.m = learn_one(b.m, s.generic, SHARE_GENERIC, expect_hits);
    b.l = learn_one(b.l, s.nlong, SHARE_LONG, expect_hits);
    b.c = learn_one(b.c, s.ncand, SHARE_CAND, expect_hits);
    b.w = learn_one(b.w, s.nwalk_total, SHARE_WALK, expect_hits);   // the counters count beyond the capacities
    // ... and the fullest shard of the worst unit, not the batch's average, is what has to fit (microsatellites are not spread
    // evenly over the pairs); shrink (tests) made the capacities smaller, not the need larger
    b.w = std::min(BOOST_MAX, std::max(b.w, LEARN_SLACK * b.w * ((double)s.nwalk_over / (double)WALK_FULL) / shrink));
}

// ---- capacities.  f, m: per shard; l, c: the whole queue
struct Caps { uint64_t f = 0, m = 0, l = 0, c = 0; };
inline uint64_t sharded_cap(double expect_hits, double share, double boost, double shrink, uint64_t floor) {
    return (uint64_t)(expect_hits * share / SHARDS * SHARD_SLACK * boost / shrink) + (uint64_t)((double)floor / shrink) + CAP_PAD;
}
inline uint64_t whole_cap(double expect_hits, double share, double boost, double shrink) {
    return (uint64_t)(expect_hits * share * boost / shrink) + (uint64_t)((double)QUEUE_FLOOR / shrink) + CAP_PAD;
}
inline Caps initial_caps(double expect_hits, const Boosts &b, double shrink) {
    return Caps{sharded_cap(expect_hits, SHARE_FOLLOW, b.f, shrink, QUEUE_FLOOR), sharded_cap(expect_hits, SHARE_GENERIC, b.m, shrink, QUEUE_FLOOR),
                whole_cap(expect_hits, SHARE_LONG, b.l, shrink), whole_cap(expect_hits, SHARE_CAND, b.c, shrink)};
}
// a unit's walk-queue region: eight shards of this many entries, from the unit's own expected hits
inline uint64_t walk_cap(double unit_hits, const Boosts &b, double shrink) { return sharded_cap(unit_hits, SHARE_WALK, b.w, shrink, WALK_FLOOR); }
inline uint64_t walk_entries(const std::vector<uint64_t> &walk_cap_u) { return SHARDS * std::accumulate(walk_cap_u.begin(), walk_cap_u.end(), (uint64_t)0); }

inline bool over(const Caps &c, const Counts &s) {
    return s.followers > c.f || s.generic > c.m || s.nlong > c.l || s.ncand > c.c || s.nwalk_over > WALK_FULL;
}
// after an overflow: room for what the counters saw, and half as much again (the repeated tails may add candidates of their
// own); every unit's walk-queue region grows by what the fullest shard lacked, and a quarter
inline void grow(Caps &c, std::vector<uint64_t> &walk_cap_u, const Counts &s) {
    c.f = std::max<uint64_t>(c.f, s.followers + s.followers / 2 + 1024);
    c.m = std::max<uint64_t>(c.m, s.generic + s.generic / 2 + 1024);
    c.l = std::max<uint64_t>(c.l, s.nlong + s.nlong / 2 + 1024);
    c.c = std::max<uint64_t>(c.c, 2 * s.ncand + 65536);
    if (s.nwalk_over > WALK_FULL) {
        const double by = 1.25 * (double)s.nwalk_over / (double)WALK_FULL;
        for (uint64_t &w : walk_cap_u)
            if (w) w = (uint64_t)((double)w * by) + 1024;
    }
}

// ---- the queue arena: ten slices, each rounded up to 256 bytes, carved in this order
enum QueueSlice { Q_FKEY, Q_FPREV, Q_MEDQ, Q_MEDU, Q_LONGQ, Q_LONGU, Q_CAND, Q_HSPS, Q_HSP_UNIT, Q_WALKQ, Q_SLICES };
struct QueueSizes { uint64_t bytes[Q_SLICES]; };
constexpr uint64_t SLICE_ALIGN = 256;
constexpr uint64_t slice_round(uint64_t bytes) { return (bytes + SLICE_ALIGN - 1) & ~(SLICE_ALIGN - 1); }
// mirror: the batch has mirror riders (every HSP may be emitted twice); v1: MIMEO_HEAVY=v1 has no walk queue
inline QueueSizes queue_slices(const Caps &c, uint64_t walk_entries, bool mirror, bool v1) {
    const uint64_t mf = mirror ? 2 : 1;
    return QueueSizes{{c.f * SHARDS * FKEY_BYTES, c.f * SHARDS * FPREV_BYTES, c.m * SHARDS * MEDQ_BYTES, c.m * SHARDS * UNIT_BYTES, c.l * LONGQ_BYTES, c.l * UNIT_BYTES,
                       c.c * CAND_BYTES, c.c * HSP_BYTES * mf, c.c * UNIT_BYTES * mf, (v1 ? 0 : walk_entries * WALK_BYTES) + WALK_PAD}};   // in the order of QueueSlice
}
template <int N>
inline uint64_t place_slices(const uint64_t (&bytes)[N], uint64_t (&off)[N]) {   // the slices one behind the other: where each starts, what all take
    uint64_t total = 0;
    for (int i = 0; i < N; i++) { off[i] = total; total += slice_round(bytes[i]); }
    return total;
}
// What the batch declares for the queue arena (the budget test rests on it): the entries at their byte costs plus a margin
// that covers the ten roundings and the walk queue's pad, so that carving never passes what was declared
constexpr uint64_t ARENA_MARGIN = 4096;
static_assert(ARENA_MARGIN >= Q_SLICES * (SLICE_ALIGN - 1) + WALK_PAD, "the margin must cover every slice's rounding and the walk queue's pad");
inline uint64_t arena_bytes(const Caps &c, uint64_t walk_entries, bool mirror, bool v1) {
    uint64_t sum = ARENA_MARGIN - (v1 ? 0 : WALK_PAD);
    for (uint64_t b : queue_slices(c, walk_entries, mirror, v1).bytes) sum += b;
    return sum;
}
// ... plus what the rest of the batch may ask for while the queues are alive: the sort arena with every shard full, and the
// chain / gapped stage's scratch
inline uint64_t queue_bytes(const Caps &c, uint64_t walk_entries, bool mirror, bool v1) {
    return arena_bytes(c, walk_entries, mirror, v1) + c.f * SHARDS * SORT_BYTES_PER_FOLLOWER + c.c * (mirror ? 2 : 1) * CHAIN_BYTES_PER_CAND;
}

// ---- the sort arena: six slices sized by the nf followers the batch really has; scratch: what rocPRIM's sort and select ask for
enum SortSlice { S_FKEY2, S_FPREV2, S_FLAGS, S_SEGS, S_BIGSEG, S_TMP, S_SLICES };
struct SortSizes { uint64_t bytes[S_SLICES]; };
inline SortSizes sort_slices(uint64_t nf, uint64_t scratch) {
    return SortSizes{{nf * FKEY_BYTES, nf * FPREV_BYTES, nf, nf * 8, nf * 8, scratch + 16}};   // in the order of SortSlice
}

// ---- the budget: free device memory plus what the batch's arenas would give back, less a reserve for chain / gapped
// scratch.  forced (tests, MIMEO_QUEUE_BUDGET_MB): this many MiB whatever the device has
constexpr uint64_t GiB = 1ull << 30;
inline uint64_t queue_budget(uint64_t free_b, uint64_t held, bool forced, long forced_mb) {
    const uint64_t have = free_b + held, reserve = std::min<uint64_t>(have / 8, 8 * GiB);
    return forced ? (uint64_t)forced_mb << 20 : have - reserve;
}
// a batch whose queues do not fit is cut in two by the caller; one that cannot be cut is tried anyway
inline bool must_split(bool splittable, uint64_t queue_bytes, uint64_t budget) { return splittable && queue_bytes > budget; }

// ---- arena growth.  An arena that holds `cap` bytes must hold `total`: it takes first_slack more on its first allocation and
// half as much again when it grows (hipMalloc costs ~35 ms per GiB: the next overflow or larger batch should not allocate
// again), unless that would leave less than `headroom` of the device's free memory — then exactly `total`.
// The two arenas differ on purpose.  The queue arena is allocated first: its head-room is what comes after it (sort arena at
// its worst + chain scratch = queue_bytes - arena_bytes) plus 8 GiB, and its first allocation is exact: the capacities it
// is sized by carry their slack already.  The sort arena comes after the queue arena, when only the chain / gapped scratch is
// still to come: 4 GiB of head-room, and an eighth of slack at first, since it is sized by the followers a batch really has,
// which differ from batch to batch.
constexpr uint64_t QUEUE_ARENA_HEADROOM = 8 * GiB, SORT_ARENA_HEADROOM = 4 * GiB;
inline uint64_t arena_want(uint64_t total, uint64_t cap, uint64_t free_b, uint64_t headroom, uint64_t first_slack) {
    const uint64_t want = cap ? total + total / 2 : total + first_slack;
    return want + headroom > free_b + cap ? total : want;
}

// ---- the follower key: unit << (dbits + ebits) | (diagonal + Q.len) << ebits | seed end, in 64 bits
inline uint32_t bits_for(uint64_t v) {   // bits needed to hold values 0 .. v
    uint32_t b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}
struct KeyBits { uint32_t ebits, dbits, key_bits; bool fits; };
inline KeyBits follower_key_bits(uint64_t max_tlen, uint64_t max_qlen, uint32_t nunits, uint32_t seed_len) {
    const uint32_t ebits = bits_for(max_tlen + seed_len), dbits = bits_for(max_tlen + max_qlen + seed_len), ubits = nunits > 1 ? bits_for(nunits - 1) : 0;
    return KeyBits{ebits, dbits, std::min(64u, ebits + dbits + ubits), ebits + dbits <= 63 && ebits + dbits + ubits <= 64};
}
// largest batch the key can name for scaffolds of these lengths (at most 2^20 units)
inline uint32_t max_units(uint64_t max_tlen, uint64_t max_qlen, uint32_t seed_len) {
    const KeyBits k = follower_key_bits(max_tlen, max_qlen, 1, seed_len);
    const uint32_t ubits = 64 - std::min(63u, k.ebits + k.dbits);
    return ubits >= 20 ? (1u << 20) : (1u << ubits);
}

}  // namespace queue_plan
}  // namespace mimeo
