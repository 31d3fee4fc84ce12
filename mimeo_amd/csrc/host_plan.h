// host_plan.h — HIP-free planning logic of the pipeline: which scaffolds are concatenated into which super-scaffold
// (pack.hip), whether a pair list is a full cross product, which pairs share a plus strand, and how the units of a call
// are cut into index blocks and batches (pipeline.hip).  Kept apart from the device code so that it runs under the CPU
// sanitizers (tests/sanitize/host_sanitize.cc, tests/test_host_sanitize.py).
#pragma once
#include <algorithm>
#include <cstdint>
#include <map>
#include <utility>
#include <vector>

namespace mimeo {
namespace host_plan {

struct Member { uint32_t id, start, len; };   // scaffold number, first base inside the super-scaffold, bases

// ids: the scaffolds that take part (ascending).  Scaffolds of at most member_max bases are packed, in order, into supers
// of at most about super_len bases: members start on 32-base boundaries, at least `spacer` bases behind the end of the
// member before; every other scaffold (and an empty one) is a super of its own.
inline std::vector<std::vector<Member>> plan_supers(const std::vector<uint64_t> &len_of, const std::vector<uint32_t> &ids, uint32_t spacer,
                                                    uint64_t member_max, uint64_t super_len) {
    std::vector<std::vector<Member>> plan;
    std::vector<Member> cur;
    uint64_t cur_end = 0;
    auto close = [&]() { if (!cur.empty()) { plan.push_back(cur); cur.clear(); } cur_end = 0; };
    for (uint32_t id : ids) {
        const uint64_t len = len_of[id];
        if (len > member_max || len == 0) {
            plan.push_back(std::vector<Member>{Member{id, 0u, (uint32_t)len}});
            continue;
        }
        uint64_t start = cur.empty() ? 0 : ((cur_end + spacer + 31) / 32) * 32;
        if (!cur.empty() && start + len > super_len) { close(); start = 0; }
        cur.push_back(Member{id, (uint32_t)start, (uint32_t)len});
        cur_end = start + len;
    }
    close();
    return plan;
}

// Is (pair_t[k], pair_q[k]), k < n, the full cross product of the targets and the queries it names?  Duplicates count
// once (dups: (duplicate, first occurrence)); pairidx[trank[t] * nq + qrank[q]] = first occurrence of (t, q).
struct CrossProduct {
    bool full = false;
    std::vector<uint32_t> tset, qset, trank, qrank, pairidx;
    std::vector<std::pair<uint64_t, uint64_t>> dups;
    size_t distinct = 0;
};
inline CrossProduct cross_product(const uint32_t *pair_t, const uint32_t *pair_q, uint64_t n, size_t n_targets, size_t n_queries) {
    CrossProduct c;
    c.tset.assign(pair_t, pair_t + n); c.qset.assign(pair_q, pair_q + n);
    std::sort(c.tset.begin(), c.tset.end()); c.tset.erase(std::unique(c.tset.begin(), c.tset.end()), c.tset.end());
    std::sort(c.qset.begin(), c.qset.end()); c.qset.erase(std::unique(c.qset.begin(), c.qset.end()), c.qset.end());
    c.trank.assign(n_targets, 0xFFFFFFFFu); c.qrank.assign(n_queries, 0xFFFFFFFFu);
    for (size_t i = 0; i < c.tset.size(); i++) c.trank[c.tset[i]] = (uint32_t)i;
    for (size_t i = 0; i < c.qset.size(); i++) c.qrank[c.qset[i]] = (uint32_t)i;
    const size_t nq = c.qset.size();
    if (nq && c.tset.size() > (size_t)0xFFFFFFF0u / nq) return c;   // more cells than a pair index can name: not taken
    if (c.tset.size() * nq > n) return c;   // fewer pairs than cells: cannot be the full product (a sparse list would cost |T| x |Q| cells to find out)
    c.pairidx.assign(c.tset.size() * nq, 0xFFFFFFFFu);
    for (uint64_t k = 0; k < n; k++) {
        uint32_t &slot = c.pairidx[(size_t)c.trank[pair_t[k]] * nq + c.qrank[pair_q[k]]];
        if (slot == 0xFFFFFFFFu) { slot = (uint32_t)k; c.distinct++; } else c.dups.emplace_back(k, slot);
    }
    c.full = c.distinct == c.pairidx.size();
    return c;
}

// Seed hits a unit of nt x nq indexed positions yields on random sequence (13 words within one transition of each of 2^24
// keys): what batches are cut by and queues are sized from.
inline double expected_seed_hits(uint64_t nt, uint64_t nq) {
    const double t = (double)nt, q = (double)nq;
    return 13.0 * t * q / 16777216.0;
}

// Index blocks.  units: anything with a target key .t and a query key .q; t_bytes / q_bytes: index bytes a key still costs
// (indexed by key; 0: already there).  When the indexes of all keys named exceed the budget the keys are ranked and the unit
// matrix is cut into blocks of Bt target ranks x Bq query ranks whose indexes fit, half the budget to each side: the units
// are reordered block by block, target-major inside a block and stable otherwise (the two strands of a pair stay adjacent).
// Returns the unit index where each block ends; one block, the order unchanged, when everything fits.
template <typename Unit>
inline std::vector<size_t> index_blocks(std::vector<Unit> &units, const std::vector<uint64_t> &t_bytes, const std::vector<uint64_t> &q_bytes,
                                        uint64_t budget) {
    std::map<uint32_t, uint64_t> tblk, qblk;   // key -> rank, then block
    for (const Unit &u : units) { tblk[u.t]; qblk[u.q]; }
    uint64_t need = 0, tmax = 1, qmax = 1;
    for (auto &kv : tblk) { need += t_bytes[kv.first]; tmax = std::max(tmax, t_bytes[kv.first]); }
    for (auto &kv : qblk) { need += q_bytes[kv.first]; qmax = std::max(qmax, q_bytes[kv.first]); }
    if (need <= budget || units.empty()) return std::vector<size_t>{units.size()};
    const uint64_t Bt = std::max<uint64_t>(1, budget / 2 / tmax), Bq = std::max<uint64_t>(1, budget / 2 / qmax);
    uint64_t rt = 0, rq = 0;
    for (auto &kv : tblk) kv.second = rt++ / Bt;
    for (auto &kv : qblk) kv.second = rq++ / Bq;
    auto block_of = [&](const Unit &u) { return std::make_pair(tblk[u.t], qblk[u.q]); };
    std::stable_sort(units.begin(), units.end(), [&](const Unit &a, const Unit &b) {
        return block_of(a) != block_of(b) ? block_of(a) < block_of(b) : a.t < b.t;
    });
    std::vector<size_t> block_end;
    for (size_t i = 1; i <= units.size(); i++)
        if (i == units.size() || block_of(units[i]) != block_of(units[i - 1])) block_end.push_back(i);
    return block_end;
}

// Shared plus strand of a self job.  When the list names (t, q) and (q, t), t != q, both on the plus strand (strands[k] & 1),
// and neither scaffold has a target-only seed plane (soft-masked bases), the first occurrence of (min, max) also serves
// the first occurrence of (max, min): mirror_of[lo] = hi, served[hi] = 1.  Later occurrences are units of their own.
constexpr uint64_t NO_PAIR = ~0ull;
struct MirrorPairs { std::vector<uint64_t> mirror_of; std::vector<char> served; };
inline MirrorPairs mirror_pairs(const uint32_t *pair_t, const uint32_t *pair_q, const std::vector<uint8_t> &strands,
                                const std::vector<char> &target_plane) {
    const uint64_t n = strands.size();
    MirrorPairs m{std::vector<uint64_t>(n, NO_PAIR), std::vector<char>(n, 0)};
    std::map<std::pair<uint32_t, uint32_t>, std::pair<uint64_t, uint64_t>> first;   // (min, max) -> first (min, max), first (max, min)
    for (uint64_t k = 0; k < n; k++) {
        const uint32_t t = pair_t[k], q = pair_q[k];
        if (t == q || !(strands[k] & 1) || target_plane[t] || target_plane[q]) continue;
        auto &f = first.emplace(std::make_pair(std::min(t, q), std::max(t, q)), std::make_pair(NO_PAIR, NO_PAIR)).first->second;
        uint64_t &slot = t < q ? f.first : f.second;
        if (slot == NO_PAIR) slot = k;
    }
    for (auto &kv : first)
        if (kv.second.first != NO_PAIR && kv.second.second != NO_PAIR) { m.mirror_of[kv.second.first] = kv.second.second; m.served[kv.second.second] = 1; }
    return m;
}

// Rows of one pair as the batches left them -> plus-strand rows first, stable (a pair's strands may come from different
// batches).  cnt / blk (null: no paths): cnt[i] blocks of row i, all rows' blocks one after the other in blk; they move
// with their rows.  Row: anything with .qstrand
template <typename Row, typename Block>
inline void plus_strand_first(std::vector<Row> &rows, std::vector<uint32_t> *cnt, std::vector<Block> *blk) {
    auto by_strand = [](const Row &a, const Row &b) { return a.qstrand < b.qstrand; };
    if (!cnt) { std::stable_sort(rows.begin(), rows.end(), by_strand); return; }
    if (std::is_sorted(rows.begin(), rows.end(), by_strand)) return;
    std::vector<size_t> ord(rows.size()), off(rows.size() + 1, 0);
    for (size_t i = 0; i < rows.size(); i++) { ord[i] = i; off[i + 1] = off[i] + (*cnt)[i]; }
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return rows[a].qstrand < rows[b].qstrand; });
    std::vector<Row> r2;
    std::vector<uint32_t> c2;
    std::vector<Block> b2;
    r2.reserve(rows.size()); c2.reserve(rows.size()); b2.reserve(blk->size());
    for (size_t i : ord) {
        r2.push_back(rows[i]); c2.push_back((*cnt)[i]);
        b2.insert(b2.end(), blk->begin() + off[i], blk->begin() + off[i + 1]);
    }
    rows.swap(r2); cnt->swap(c2); blk->swap(b2);
}

// Batch cut.  A unit takes one work slot, or two with its mirror rider (which never leaves it); the batch that starts at
// unit b0 takes units greedily while the slots, the expected seed hits and the group weights stay within the limits — the
// first unit whatever it costs.
struct BatchUnit { uint32_t slots; double hits; uint64_t weight; };
struct BatchLimits { size_t max_units; double max_hits; uint64_t max_weight; };
struct Batch { size_t end, slots; double hits; };   // [b0, end): work slots and expected seed hits of the batch
inline Batch batch_cut(const std::vector<BatchUnit> &units, size_t b0, size_t block_end, const BatchLimits &lim) {
    Batch b{b0, 0, 0.0};
    uint64_t weight = 0;
    for (; b.end < block_end; b.end++) {
        const BatchUnit &u = units[b.end];
        if (b.slots && (b.slots + u.slots > lim.max_units || b.hits + u.hits > lim.max_hits || weight + u.weight > lim.max_weight)) break;
        b.slots += u.slots; b.hits += u.hits; weight += u.weight;
    }
    return b;
}

// Tandem scorer beyond 64 periods (k8_tandem.hip): one wavefront works through one job = (slice, period block); block k
// holds the periods 64k + 1 .. 64k + 64, lane = period.  A period p walks the diagonals p - b .. p + b (b = 0 for p = 1,
// 1 for p < 5, else 2; delta <= 0: b = 0) of a slice longer than p - b, so a block has work on a slice of L bases only
// when its smallest diagonal lies below L: the others are left out (a 300-base hit at maxperiod 2000 costs 5 waves, not
// 32).  A wave is serial over its slice, so the longest slices come first (stable: equal lengths keep the caller's
// order, blocks ascending inside a slice).  The device sees the list TANDEM_CHUNK_JOBS jobs at a time.
constexpr int TANDEM_MAXPERIOD = 2000;    // TRF's own upper end for this argument
constexpr uint32_t TANDEM_BLOCK = 64;     // periods per job
struct TandemJob { uint32_t slice, block; };
constexpr uint64_t TANDEM_CHUNK_BYTES = 64ull << 20;   // device bytes the job list may take
constexpr uint64_t TANDEM_CHUNK_JOBS = TANDEM_CHUNK_BYTES / sizeof(TandemJob);
constexpr uint32_t tandem_block_first_diagonal(uint32_t block, int delta) {   // constexpr: the kernel calls it too
    return block == 0 ? 1u : block * TANDEM_BLOCK + 1u - (delta > 0 ? 2u : 0u);
}
inline std::vector<TandemJob> tandem_jobs(const std::vector<uint32_t> &lengths, int maxperiod, int delta) {
    const uint32_t nblocks = maxperiod > 0 ? ((uint32_t)maxperiod + TANDEM_BLOCK - 1) / TANDEM_BLOCK : 0;
    std::vector<uint32_t> order(lengths.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = (uint32_t)i;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return lengths[a] > lengths[b]; });
    std::vector<TandemJob> jobs;
    for (uint32_t s : order)
        for (uint32_t k = 0; k < nblocks && tandem_block_first_diagonal(k, delta) < lengths[s]; k++) jobs.push_back(TandemJob{s, k});
    return jobs;
}

}  // namespace host_plan
}  // namespace mimeo
