// pipeline.hip — host orchestration of the per-pair loop of run_jobs.sh
// (src/mimeo/wrappers.py:1015-1059 in the reference): mimeo_align_pairs / mimeo_align_pair / mimeo_align_units.
//
// A call is a list of UNITS, each one seed scan + gap-free stage: (target scaffold, query scaffold, strand) on the per-pair
// path, (target super, query super, strand) on the packed path (fragmented assemblies, pack.hip).  The plus-strand unit of
// an unordered pair of a self job also serves the other order (a "rider": a work slot without indexes that receives the
// transposed HSPs).  Both paths hand their units to ONE driver, run_batches:
//   index blocks  when the seed indexes of the call exceed the budget the unit matrix is cut into blocks whose indexes fit
//                 (host_plan::index_blocks); a block builds its indexes (or adopts them from its genome), runs, gives them
//                 back.  lastz rebuilds its table in every one of the S^2 invocations.
//   batches       a block's units are cut greedily into batches (host_plan::batch_cut: work slots, expected seed hits,
//                 groups; halved when ExtBatch finds that the queues do not fit) — a target row of a C4 job, 200 units, is one — that
//                 run one at a time, each a straight stream of device work: ExtBatch::run (K34 over all units of the batch,
//                 the exact walks of the hits it passes on, then the tails once per batch: walks beyond the frame, one radix
//                 sort of all followers, segment resolution, entropy; two host round trips), the path's groups (one per
//                 scaffold pair and strand), K5 / K6 over all groups (round trips per DP round), the alignments packed
//                 densely and read back
// What differs between the paths is passed in as a BatchPath: how the groups of a batch reach the device (uploaded from
// the host; made on the device from the super units' HSPs) and how the results are routed to the caller's pairs.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <numeric>
#include <set>
#include <tuple>

#include "common.h"

namespace mimeo {

extern mimeo_stats g_stats;

// Seed indexes of one call (or of one index block of it).  key: (scaffold address, strand, target-role sv plane in
// use).  An index a genome kept from an earlier call (mimeo_genome_keep_indexes) is adopted, the others are built
// before the first batch that needs them runs.
struct IndexCache {
    typedef std::tuple<const Scaffold *, int, int> Key;
    std::map<Key, SeedIndex> m;
    std::vector<std::pair<Key, StrandView>> plan;
    std::map<Key, const mimeo_genome *> owner_of;
    std::set<Key> adopted;
    float ms = 0;

    static Key key_of(const Scaffold &s, int minus, bool as_target, StrandView *sv) {
        const bool tsv = as_target && !minus && s.fwd.sv_target != nullptr;
        *sv = (minus ? s.rc : s.fwd).view(tsv);
        return std::make_tuple(&s, minus, tsv ? 1 : 0);
    }
    static std::tuple<uint32_t, int, int> kept_key(const mimeo_genome *g, const Key &k) {
        return std::make_tuple((uint32_t)(std::get<0>(k) - g->scaf.data()), std::get<1>(k), std::get<2>(k));
    }
    void want(const mimeo_genome *owner, const Scaffold &s, int minus, bool as_target, std::set<Key> &seen) {
        StrandView sv;
        Key k = key_of(s, minus, as_target, &sv);
        if (!seen.insert(k).second) return;
        owner_of[k] = owner;
        if (owner) {
            auto it = owner->kept.find(kept_key(owner, k));
            if (it != owner->kept.end()) { m.emplace(k, it->second); adopted.insert(k); return; }
        }
        plan.emplace_back(k, sv);
    }
    int build_all() {
        for (auto &job : plan) {
            SeedIndex idx;
            int rc = build_index(job.second, idx, &ms);
            if (rc) return rc;
            m.emplace(job.first, idx);
        }
        plan.clear();
        return 0;
    }
    int get(const Scaffold &s, int minus, bool as_target, IndexView *out, StrandView *sv) {
        Key k = key_of(s, minus, as_target, sv);
        auto it = m.find(k);
        if (it == m.end()) { set_error("seed index was not planned"); return MIMEO_ERR_ARG; }
        *out = it->second.view();
        return 0;
    }
    // end of a call: indexes go to their genome when it keeps them (also after an error: they are
    // complete), else back to the pool
    ~IndexCache() { clear(); }   // error paths that leave the call early give the indexes back too
    void clear() {
        for (auto &kv : m) {
            if (adopted.count(kv.first)) continue;  // still owned by the genome
            const mimeo_genome *g = owner_of[kv.first];
            if (g && g->keep_indexes) g->kept.emplace(kept_key(g, kv.first), kv.second);
            else kv.second.release();
        }
        m.clear();
    }
};

static ExtBatch g_ext;
static DeviceBuf g_scratch, g_aln, g_dense, g_groups;
static DeviceBuf g_pfirst, g_pblocks;   // paths of the batch's dense alignments (dense_paths_device)
// device tables of the packed path (run_packed)
static struct PackTables {
    DeviceBuf toff, tstart, tlen, trank, qoff, qstart, qlen, qrank, pairidx, pt, pq, tview, qvf, qvr, utab;
    void release() {
        for (DeviceBuf *b : {&toff, &tstart, &tlen, &trank, &qoff, &qstart, &qlen, &qrank, &pairidx, &pt, &pq, &tview, &qvf, &qvr, &utab}) b->release();
    }
} g_pack;
static std::vector<std::pair<uint64_t, int>> g_failed;   // pairs of the last call that hit a limit
const std::vector<std::pair<uint64_t, int>> &failed_pairs() { return g_failed; }

using host_plan::NO_PAIR;
// A work slot of a batch: one (target, query, strand) of scaffolds (per-pair path; pair: its index in pair_t / pair_q) or
// of super-scaffolds (packed path).  A unit is a slot that runs the seed scan; mirrored: the slot behind it is its rider
// (q, t, +), which serves mirror_pair.
struct Slot { uint32_t t, q, minus; uint64_t pair; };
struct Unit : Slot { bool mirrored; uint64_t mirror_pair; };

// switches read once per call (tests change them between calls)
struct Switches {
    bool pack, mirror, no_diag0, timing, k6_stats;
    uint64_t pack_member, pack_super, index_budget_mb;
    size_t pack_min, batch_units;
    double batch_hits;
    static const char *env(const char *k) { return getenv(k); }
    Switches() {
        pack = !(env("MIMEO_PACK") && !atoi(env("MIMEO_PACK")));
        mirror = !(env("MIMEO_MIRROR") && !atoi(env("MIMEO_MIRROR")));
        no_diag0 = env("MIMEO_NO_DIAG0") != nullptr;
        timing = env("MIMEO_TIMING") != nullptr;
        k6_stats = env("MIMEO_K6_STATS") != nullptr;
        pack_member = env("MIMEO_PACK_MEMBER") ? (uint64_t)atol(env("MIMEO_PACK_MEMBER")) : (6ull << 20);
        pack_super = env("MIMEO_PACK_SUPER") ? (uint64_t)atol(env("MIMEO_PACK_SUPER")) : (20ull << 20);
        pack_min = env("MIMEO_PACK_MIN") ? (size_t)atol(env("MIMEO_PACK_MIN")) : 8;
        index_budget_mb = env("MIMEO_INDEX_BUDGET_MB") ? (uint64_t)atol(env("MIMEO_INDEX_BUDGET_MB")) : 0;
        batch_units = env("MIMEO_BATCH_UNITS") ? (size_t)std::max(1l, atol(env("MIMEO_BATCH_UNITS"))) : 0;
        batch_hits = env("MIMEO_BATCH_HITS") ? atof(env("MIMEO_BATCH_HITS")) : 2.5e10;
    }
    // Seed indexes cost 64 MiB + 52 bytes per base and strand (a 1 Gbp genome, both strands: 117 GB; 2000 small scaffolds x 2
    // strands: 256 GB of offset arrays): a call's get 60 % of the free device memory (MIMEO_INDEX_BUDGET_MB for tests)
    int index_budget(uint64_t *budget) const {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        *budget = index_budget_mb ? index_budget_mb << 20 : (uint64_t)(0.6 * (double)free_b);
        return 0;
    }
    // most work slots of a batch: the follower key names at most 2^(64 - end bits - diagonal bits) units, K5 / K6 take at
    // most 8192 groups from the per-pair path
    size_t max_units(uint64_t max_t, uint64_t max_q) const {
        const size_t m = std::min<size_t>(8192, ext_batch_max_units(max_t, max_q));
        return batch_units ? std::min(m, batch_units) : m;
    }
};

// mimeo_shutdown: give the work buffers and streams back
void release_pipeline_buffers() {
    g_ext.release();
    for (DeviceBuf *b : {&g_scratch, &g_aln, &g_dense, &g_groups, &g_pfirst, &g_pblocks}) b->release();
    g_pack.release();
    release_k5_buffers();
    release_pack_buffers();
}

// the extension stage of an arbitrary unit list, HSPs copied to the host per unit (stage entry point
// mimeo_ungapped_hsps: the same code path as mimeo_align_pairs up to K4)
int ungapped_units(const std::vector<UnitWork> &work, const mimeo_params *p, std::vector<std::vector<mimeo_hsp>> *per_unit,
                   ExtStats *st) {
    uint64_t nh = 0;
    g_ext.new_call();
    int rc = g_ext.run(work, p, &nh, st);
    if (rc) return rc;
    per_unit->assign(work.size(), std::vector<mimeo_hsp>());
    if (!nh) return 0;
    std::vector<mimeo_hsp> h(nh);
    std::vector<uint32_t> u(nh);
    HIP_TRY(hipMemcpy(h.data(), g_ext.hsps.p, nh * sizeof(mimeo_hsp), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(u.data(), g_ext.hsp_unit.p, nh * 4, hipMemcpyDeviceToHost));
    for (uint64_t i = 0; i < nh; i++) (*per_unit)[u[i]].push_back(h[i]);
    return 0;
}

template <typename T>
static int upload(DeviceBuf &b, const std::vector<T> &v) {
    int rc = b.reserve((v.size() ? v.size() : 1) * sizeof(T));
    if (rc) return rc;
    if (!v.empty()) HIP_TRY(hipMemcpyAsync(b.p, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream()));
    return 0;
}

static void record_failure(uint64_t pair, uint32_t tid, uint32_t qid, char strand, std::vector<char> &failed) {
    if (failed[pair]) return;
    failed[pair] = 1;
    g_failed.emplace_back(pair, MIMEO_ERR_LIMIT);
    char msg[256];
    snprintf(msg, sizeof msg, "gapped extension of target %u, query %u, strand %c: DP band wider than 65536 columns (or, under the path rule, a "
             "traceback larger than the trace pool): "
             "not supported; the pair is left out (mimeo_get_failed_pairs)", tid, qid, strand);
    set_error(msg);   // readable through mimeo_last_error() although the call succeeds
}

// ---- the batch driver ------------------------------------------------------------------------------------------------------
struct CallTimes { ExtStats est; float ms_chain = 0, ms_gapped = 0, ms_index = 0; };
// mimeo_align_units_paths: the paths travel next to the alignments — per batch in dense order, then per pair
struct PairPaths {
    std::vector<uint64_t> first;               // of the batch at hand: offsets of its dense alignments into dense (one more than alignments)
    std::vector<mimeo_path_block> dense;
    std::vector<std::vector<uint32_t>> cnt;            // per pair: blocks of each of its alignments, in the order of its rows
    std::vector<std::vector<mimeo_path_block>> blk;    // per pair: the blocks, alignment after alignment
    // dense alignments [d0, d1) of the batch go to `pair`
    void take(uint64_t pair, uint64_t d0, uint64_t d1) {
        for (uint64_t d = d0; d < d1; d++) cnt[pair].push_back((uint32_t)(first[d + 1] - first[d]));
        blk[pair].insert(blk[pair].end(), dense.begin() + first[d0], dense.begin() + first[d1]);
    }
};
// what differs between the per-pair path and the packed path
struct BatchPath {
    const mimeo_genome *t_owner, *q_owner;   // the genomes whose kept indexes are adopted and that keep new ones (null: supers)
    const Scaffold *tscaf, *qscaf;           // what Unit::t and Unit::q number
    uint64_t *slots_stat;                    // the field of g_stats that counts the path's work slots
    PairPaths *paths;                        // null: the call asks for no paths
    std::function<uint64_t(const Unit &)> group_bound;   // most groups the unit (with its rider) can yield
    // the groups of the batch (K5 / K6: one per scaffold pair and strand) into g_groups
    std::function<int(const std::vector<Slot> &, const std::vector<UnitWork> &, uint64_t nh, uint32_t *ngroups)> groups_to_device;
    // after K6 and dense_alignments_device: failed pairs, chained_hsps, the alignments (read_alignments) to their pairs
    std::function<int(const std::vector<Slot> &, uint32_t ngroups)> collect;
};

// the alignments of a batch are a few thousand records in an array of one slot per HSP: packed on the device
// (dense_alignments_device), then read; last: the last group of the batch as K6 left it
static int read_alignments(const Group &last, std::vector<mimeo_alignment> &host_aln) {
    host_aln.resize((uint64_t)last.job0 + last.naln);
    if (host_aln.empty()) return 0;
    HIP_TRY(hipMemcpyAsync(host_aln.data(), g_dense.p, host_aln.size() * sizeof(mimeo_alignment), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

// ... and their paths (only when asked for): emitted on the device in dense order, then read
static int read_paths(uint32_t ngroups, PairPaths &pp) {
    Group last;
    HIP_TRY(hipMemcpyAsync(&last, (const Group *)g_groups.p + (ngroups - 1), sizeof(Group), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    const uint64_t ndense = (uint64_t)last.job0 + last.naln;
    uint64_t nblocks = 0;
    int rc = dense_paths_device((const Group *)g_groups.p, ngroups, ndense, g_pfirst, g_pblocks, &nblocks);
    if (rc) return rc;
    pp.first.resize(ndense + 1);
    pp.dense.resize(nblocks);
    HIP_TRY(hipMemcpyAsync(pp.first.data(), g_pfirst.p, pp.first.size() * 8, hipMemcpyDeviceToHost, stream()));
    if (nblocks) HIP_TRY(hipMemcpyAsync(pp.dense.data(), g_pblocks.p, nblocks * sizeof(mimeo_path_block), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

static int print_groups(uint32_t ngroups) {   // MIMEO_K6_STATS
    std::vector<Group> g(std::min(ngroups, 24u));
    HIP_TRY(hipMemcpyAsync(g.data(), g_groups.p, g.size() * sizeof(Group), hipMemcpyDeviceToHost, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    for (const Group &x : g)
        fprintf(stderr, "  [grp] t%u q%u %c hsps %llu nchain %u naln %u\n", x.tid, x.qid, x.minus ? '-' : '+',
                (unsigned long long)(x.hsp_end - x.hsp_begin), x.nchain, x.naln);
    return 0;
}

// Works the units off: index blocks (t_bytes / q_bytes: what the index of a target / query still costs, by Unit::t / Unit::q;
// the units are reordered block by block), batches of at most max_units work slots inside a block, one at a time.  Results
// do not depend on the blocking or the batching: the path assembles them per pair.
static int run_batches(std::vector<Unit> &units, const std::vector<uint64_t> &t_bytes, const std::vector<uint64_t> &q_bytes, uint64_t budget,
                       size_t max_units, const BatchPath &path, const mimeo_params *p, const Switches &sw, CallTimes &tm) {
    const std::vector<size_t> block_end = host_plan::index_blocks(units, t_bytes, q_bytes, budget);
    // the queues of a batch are sized from its expected seed hits (2.5e10: a C4 row is 1.6e10) — less when the free device
    // memory says so (ExtBatch asks for a split: repeat-rich input beside resident indexes, C5: half of all hits are followers
    // inside microsatellites); K5 names a group in 23 bits: at most 2^22 of them
    host_plan::BatchLimits lim{max_units, sw.batch_hits, 1ull << 22};
    std::vector<host_plan::BatchUnit> cost(units.size());
    hipStream_t st = stream();
    size_t blk_begin = 0;
    for (const size_t blk_end : block_end) {
        IndexCache cache;
        std::set<IndexCache::Key> seen;
        for (size_t i = blk_begin; i < blk_end; i++) {
            cache.want(path.t_owner, path.tscaf[units[i].t], 0, true, seen);
            cache.want(path.q_owner, path.qscaf[units[i].q], (int)units[i].minus, false, seen);
        }
        auto head = [&](const Unit &u, UnitWork &w) -> int {   // the unit with the indexes its heavy kernel reads
            memset(&w, 0, sizeof w);
            int rc;
            if ((rc = cache.get(path.tscaf[u.t], 0, true, &w.ti, &w.d.T)) || (rc = cache.get(path.qscaf[u.q], (int)u.minus, false, &w.qi, &w.d.Q))) return rc;
            w.d.same = (w.d.T.pw == w.d.Q.pw && w.d.T.len == w.d.Q.len && !sw.no_diag0) ? 1u : 0u;
            return 0;
        };
        auto batches = [&]() -> int {
            int rc = cache.build_all();
            if (rc) return rc;
            for (size_t i = blk_begin; i < blk_end; i++) {
                UnitWork w;
                if ((rc = head(units[i], w))) return rc;
                cost[i] = host_plan::BatchUnit{units[i].mirrored ? 2u : 1u, host_plan::expected_seed_hits(w.ti.n, w.qi.n), path.group_bound(units[i])};
            }
            for (size_t b0 = blk_begin; b0 < blk_end;) {
                const host_plan::Batch b = host_plan::batch_cut(cost, b0, blk_end, lim);
                std::vector<UnitWork> work;
                std::vector<Slot> slots;
                std::vector<uint32_t> mirror_dst;
                for (size_t i = b0; i < b.end; i++) {
                    const Unit &u = units[i];
                    UnitWork w;
                    if ((rc = head(u, w))) return rc;
                    work.push_back(w); slots.push_back(u); mirror_dst.push_back(NO_MIRROR);
                    if (u.mirrored) {   // (q, t, +): no indexes, no heavy phase; receives the transposed HSPs
                        UnitWork m;
                        memset(&m, 0, sizeof m);
                        IndexCache::key_of(path.qscaf[u.q], 0, true, &m.d.T);   // no soft-masked bases on either: the plain planes in both roles
                        IndexCache::key_of(path.tscaf[u.t], 0, false, &m.d.Q);
                        mirror_dst.back() = (uint32_t)work.size();
                        work.push_back(m); slots.push_back(Slot{u.q, u.t, 0, u.mirror_pair}); mirror_dst.push_back(NO_MIRROR);
                    }
                }
                auto tb0 = std::chrono::steady_clock::now();
                uint64_t nh = 0;
                rc = g_ext.run(work, p, &nh, &tm.est, &mirror_dst);
                if (rc == MIMEO_ERR_SPLIT) {   // the queues of this batch do not fit beside the indexes: smaller batches from here on
                    if (b.end - b0 <= 1) { set_error("internal: a batch of one unit was refused"); return MIMEO_ERR_NOMEM; }
                    lim.max_hits = std::max(1.0, b.hits / 2);
                    lim.max_units = std::max<size_t>(1, std::min(lim.max_units, b.slots / 2));
                    continue;
                }
                if (rc) return rc;
                auto tb1 = std::chrono::steady_clock::now();
                *path.slots_stat += work.size();
                g_stats.hsps += nh;
                for (size_t i = b0; i < b.end; i++) g_stats.query_bases_scanned += path.qscaf[units[i].q].len;
                g_stats.batches++;
                uint32_t ngroups = 0;
                if (nh && (rc = path.groups_to_device(slots, work, nh, &ngroups))) return rc;
                if (ngroups) {
                    if ((rc = g_aln.reserve(nh * sizeof(mimeo_alignment))) || (rc = g_dense.reserve(nh * sizeof(mimeo_alignment)))) return rc;
                    if ((rc = chain_gapped_device((Group *)g_groups.p, ngroups, (const mimeo_hsp *)g_ext.hsps.p, (const uint32_t *)g_ext.hsp_unit.p, nh, p,
                                                  g_scratch, (mimeo_alignment *)g_aln.p, &tm.ms_chain, &tm.ms_gapped, path.paths != nullptr)))
                        return rc;
                    dense_alignments_device((Group *)g_groups.p, ngroups, (const mimeo_alignment *)g_aln.p, (mimeo_alignment *)g_dense.p);
                    if (path.paths && (rc = read_paths(ngroups, *path.paths))) return rc;
                    if (sw.k6_stats && (rc = print_groups(ngroups))) return rc;
                    if ((rc = path.collect(slots, ngroups))) return rc;
                }
                if (sw.timing) {
                    auto tb2 = std::chrono::steady_clock::now();
                    const double ms_ext = std::chrono::duration<double, std::milli>(tb1 - tb0).count(), ms_rest = std::chrono::duration<double, std::milli>(tb2 - tb1).count();
                    fprintf(stderr, "[timing] batch of %zu units: heavy + tails %.2f ms (device heavy %.2f + tails %.2f so far), chain + gapped + read-back %.2f ms (device %.2f + %.2f so far)\n",
                            work.size(), ms_ext, tm.est.ms_heavy, tm.est.ms_tails, ms_rest, tm.ms_chain, tm.ms_gapped);
                }
                b0 = b.end;
            }
            return 0;
        };
        const int rc = batches();
        if (rc) (void)hipStreamSynchronize(st);   // a started batch drains before its indexes go
        cache.clear();
        tm.ms_index += cache.ms;
        g_stats.index_blocks++;
        if (rc) return rc;
        blk_begin = blk_end;
    }
    return 0;
}

// ---- fragmented assemblies: the extension stage on super-scaffolds (pack.hip) ------------------------------------------
// Taken when the pair list is a full cross product T x Q (what every mimeo workflow asks for) with at least
// MIMEO_PACK_MIN (8) scaffolds of at most MIMEO_PACK_MEMBER (6 Mbp) bases on one side and no kept indexes; MIMEO_PACK=0
// switches it off.
// *used = false: the caller runs the unit-per-pair path.
static int run_packed(const mimeo_genome *A, const mimeo_genome *QG, const uint32_t *pair_t, const uint32_t *pair_q, uint64_t npairs,
                      const mimeo_params *p, const Switches &sw, std::vector<std::vector<mimeo_alignment>> &per_pair, std::vector<char> &failed,
                      PairPaths *pp, CallTimes &tm, bool *used) {
    *used = false;
    if (!sw.pack) return 0;
    if (npairs == 0 || npairs >= (1ull << 30)) return 0;
    // K34 works a 10 Mbp x 10 Mbp unit off at 13.5 ps per seed hit, a 5 Mbp x 5 Mbp one at 21.7, a 2 Mbp x 2 Mbp one at 117 (4096
    // tiles to stage whatever the scaffold size): scaffolds of up to 6 Mbp are packed into super-scaffolds of about 20 Mbp
    // when there are at least eight of them (C2, ten scaffolds of 5 Mbp: 144 -> 106 ms per job).
    // indexes kept on a genome handle say that the caller issues the job as many calls (a row per call): they are used
    if (A->keep_indexes || QG->keep_indexes) return 0;
    {   // the cheap rejections first: too few small scaffolds among the ones named (before any |T| x |Q| table is made)
        std::vector<uint8_t> seen_t(A->scaf.size(), 0), seen_q(QG->scaf.size(), 0);
        size_t small_t = 0, small_q = 0;
        for (uint64_t k = 0; k < npairs; k++) {
            if (!seen_t[pair_t[k]]) { seen_t[pair_t[k]] = 1; small_t += A->scaf[pair_t[k]].len <= sw.pack_member; }
            if (!seen_q[pair_q[k]]) { seen_q[pair_q[k]] = 1; small_q += QG->scaf[pair_q[k]].len <= sw.pack_member; }
        }
        if (std::max(small_t, small_q) < sw.pack_min) return 0;
    }
    host_plan::CrossProduct cp = host_plan::cross_product(pair_t, pair_q, npairs, A->scaf.size(), QG->scaf.size());
    const std::vector<uint32_t> &tset = cp.tset, &qset = cp.qset, &trank = cp.trank, &qrank = cp.qrank, &pairidx = cp.pairidx;
    const size_t nq = qset.size();
    if (!cp.full) return 0;   // not the full cross product T x Q
    // one genome, the same scaffolds in both roles: the two roles share the super-scaffolds, and the main diagonals stay
    // with k4_diag0.  A subset of the targets against all scaffolds (a rank's share of a self job, dist.py) packs the two
    // roles separately: a scaffold's main diagonal is then an ordinary diagonal of its unit, whose seed hits are resolved
    // as the followers of its first one — the general rule, which k4_diag0 only short-cuts.
    const bool self = (A == QG) && tset == qset;
    const uint32_t spacer = (uint32_t)std::max(64, p->xdrop / 100 + 32);
    SuperSide side_t, side_q;
    int rc = build_super_side(A, tset, spacer, sw.pack_member, sw.pack_super, side_t);
    if (!rc && !self) rc = build_super_side(QG, qset, spacer, sw.pack_member, sw.pack_super, side_q);
    if (rc) { side_t.release(); side_q.release(); return rc; }
    SuperSide &ST = side_t, &SQ = self ? side_t : side_q;
    struct Cleanup { SuperSide &a, &b; ~Cleanup() { a.release(); b.release(); } } cleanup{side_t, side_q};
    // seed indexes of the supers: when they do not all fit (a 3 Gbp fragmented assembly needs 330 GB of them) the super x super
    // matrix is cut into index blocks, as on the unit-per-pair path
    const int qroles = ((p->strand & MIMEO_STRAND_BOTH) == MIMEO_STRAND_BOTH) ? 2 : 1;
    std::vector<uint64_t> t_bytes, q_bytes;
    uint64_t idx_budget = 0, max_t = 1, max_q = 1;
    for (auto &s : ST.supers) { t_bytes.push_back(seed_index_bytes(s.len)); max_t = std::max<uint64_t>(max_t, s.len); }
    for (auto &s : SQ.supers) { q_bytes.push_back(seed_index_bytes(s.len) * qroles); max_q = std::max<uint64_t>(max_q, s.len); }
    if ((rc = sw.index_budget(&idx_budget))) return rc;
    if (*std::max_element(t_bytes.begin(), t_bytes.end()) + *std::max_element(q_bytes.begin(), q_bytes.end()) > idx_budget)
        return 0;   // not even one pair of supers: the other path cuts finer
    *used = true;
    // ---- device tables
    auto member_tables = [&](const SuperSide &S, const std::vector<uint32_t> &rank, std::vector<uint32_t> &off, std::vector<uint32_t> &start,
                             std::vector<uint32_t> &len, std::vector<uint32_t> &rk) {
        off.assign(1, 0u);
        for (auto &mem : S.members) {
            for (const PackMember &m : mem) { start.push_back(m.start); len.push_back(m.len); rk.push_back(rank[m.id]); }
            off.push_back((uint32_t)start.size());
        }
    };
    std::vector<uint32_t> h_toff, h_tstart, h_tlen, h_trank, h_qoff, h_qstart, h_qlen, h_qrank;
    member_tables(ST, trank, h_toff, h_tstart, h_tlen, h_trank);
    member_tables(SQ, qrank, h_qoff, h_qstart, h_qlen, h_qrank);
    std::vector<StrandView> h_tview(A->scaf.size()), h_qvf(QG->scaf.size()), h_qvr(QG->scaf.size());
    for (uint32_t t : tset) { IndexCache::key_of(A->scaf[t], 0, true, &h_tview[t]); }
    for (uint32_t q : qset) { IndexCache::key_of(QG->scaf[q], 0, false, &h_qvf[q]); IndexCache::key_of(QG->scaf[q], 1, false, &h_qvr[q]); }
    std::vector<uint32_t> h_pt(pair_t, pair_t + npairs), h_pq(pair_q, pair_q + npairs);
    PackTables &d = g_pack;
    if ((rc = upload(d.toff, h_toff)) || (rc = upload(d.tstart, h_tstart)) || (rc = upload(d.tlen, h_tlen)) || (rc = upload(d.trank, h_trank)) ||
        (rc = upload(d.qoff, h_qoff)) || (rc = upload(d.qstart, h_qstart)) || (rc = upload(d.qlen, h_qlen)) || (rc = upload(d.qrank, h_qrank)) ||
        (rc = upload(d.pairidx, pairidx)) || (rc = upload(d.pt, h_pt)) || (rc = upload(d.pq, h_pq)) || (rc = upload(d.tview, h_tview)) ||
        (rc = upload(d.qvf, h_qvf)) || (rc = upload(d.qvr, h_qvr)))
        return rc;
    HIP_TRY(hipStreamSynchronize(stream()));   // the host vectors go out of use only at the end of the call; be plain about it
    RegroupTables R;
    R.t_off = (const uint32_t *)d.toff.p; R.t_start = (const uint32_t *)d.tstart.p; R.t_len = (const uint32_t *)d.tlen.p; R.t_rank = (const uint32_t *)d.trank.p;
    R.q_off = (const uint32_t *)d.qoff.p; R.q_start = (const uint32_t *)d.qstart.p; R.q_len = (const uint32_t *)d.qlen.p; R.q_rank = (const uint32_t *)d.qrank.p;
    R.pairidx = (const uint32_t *)d.pairidx.p; R.nq = (uint32_t)nq; R.pad = 0;
    R.pair_t = (const uint32_t *)d.pt.p; R.pair_q = (const uint32_t *)d.pq.p;
    R.t_view = (const StrandView *)d.tview.p; R.q_view_fwd = (const StrandView *)d.qvf.p; R.q_view_rc = (const StrandView *)d.qvr.p;

    // ---- units: (target super, query super, strand), target-major.  Self job: the plus-strand unit (S1, S2) with S1 < S2 also
    // serves (S2, S1) — its HSPs transposed — when neither super holds soft-masked bases (shared plus strand, k4_mirror_hsps)
    std::vector<Unit> units;
    const bool plus = (p->strand & MIMEO_STRAND_PLUS) != 0;
    auto can_mirror = [&](uint32_t a, uint32_t b) {
        return self && sw.mirror && plus && a != b && !ST.supers[a].fwd.sv_target && !ST.supers[b].fwd.sv_target;
    };
    for (uint32_t ts = 0; ts < ST.supers.size(); ts++)
        for (uint32_t qs = 0; qs < SQ.supers.size(); qs++)
            for (uint32_t minus = 0; minus < 2; minus++) {
                if (!(p->strand & (minus ? MIMEO_STRAND_MINUS : MIMEO_STRAND_PLUS))) continue;
                const bool mirrored = !minus && can_mirror(ts, qs);
                if (mirrored && ts > qs) continue;   // served by (qs, ts, +)
                units.push_back(Unit{{ts, qs, minus, NO_PAIR}, mirrored, NO_PAIR});
            }
    std::vector<uint3> utab;   // of the batch at hand
    BatchPath path{nullptr, nullptr, ST.supers.data(), SQ.supers.data(), &g_stats.super_units, pp, {}, {}, {}};
    // groups of a unit: at most (target members named) x nq x 2 (an upper bound; a mirror unit names the other super's)
    path.group_bound = [&](const Unit &u) { return (uint64_t)(ST.members[u.t].size() + (u.mirrored ? ST.members[u.q].size() : 0)) * nq * 2; };
    // every HSP back to its scaffold pair: the groups are made on the device
    path.groups_to_device = [&](const std::vector<Slot> &slots, const std::vector<UnitWork> &, uint64_t nh, uint32_t *ngroups) -> int {
        utab.clear();
        for (const Slot &s : slots) utab.push_back(make_uint3(s.t, s.q, s.minus));
        int rc = upload(d.utab, utab);
        if (rc) return rc;
        R.unit_tab = (const uint3 *)d.utab.p;
        if ((rc = regroup_hsps_device((mimeo_hsp *)g_ext.hsps.p, (uint32_t *)g_ext.hsp_unit.p, nh, R, (uint32_t)npairs, g_groups, ngroups))) return rc;
        if (*ngroups >= (1u << 23)) { set_error("more than 2^23 scaffold pairs with HSPs in one batch"); return MIMEO_ERR_LIMIT; }
        return 0;
    };
    path.collect = [&](const std::vector<Slot> &, uint32_t ngroups) -> int {
        uint64_t sum[3] = {0, 0, 0};
        int rc = group_summary_device((const Group *)g_groups.p, ngroups, sum);
        if (rc) return rc;
        Group last;
        HIP_TRY(hipMemcpy(&last, (const Group *)g_groups.p + (ngroups - 1), sizeof(Group), hipMemcpyDeviceToHost));
        if (sum[1]) {   // a pair that hit a limit is left out; the others go on (the reference's script has no `set -e`: utils.py:125-128)
            std::vector<uint3> bad;
            if ((rc = overflowed_groups_device((const Group *)g_groups.p, ngroups, sum[1], &bad))) return rc;
            for (const uint3 &tq : bad) record_failure(pairidx[(size_t)trank[tq.x] * nq + qrank[tq.y]], tq.x, tq.y, tq.z ? '-' : '+', failed);
        }
        g_stats.chained_hsps += sum[0];
        std::vector<mimeo_alignment> host_aln;
        if ((rc = read_alignments(last, host_aln))) return rc;
        // dense order = (pair, strand) order: a pair's plus-strand alignments come before its minus-strand ones, as on the other path
        for (size_t d = 0; d < host_aln.size(); d++) {
            const mimeo_alignment &a = host_aln[d];
            const uint32_t pair = pairidx[(size_t)trank[a.tid] * nq + qrank[a.qid]];
            per_pair[pair].push_back(a);
            if (pp) pp->take(pair, d, d + 1);
        }
        return 0;
    };
    rc = run_batches(units, t_bytes, q_bytes, idx_budget, sw.max_units(max_t, max_q), path, p, sw, tm);
    g_stats.pair_strands += cp.distinct * qroles;
    if (!rc)   // duplicates (duplicate, first occurrence) are answered from the first
        for (auto &dp : cp.dups) {
            per_pair[dp.first] = per_pair[dp.second];
            if (pp) { pp->cnt[dp.first] = pp->cnt[dp.second]; pp->blk[dp.first] = pp->blk[dp.second]; }
        }   // a failed pair's duplicates are failed with it by align_units_impl
    return rc;
}

// ---- one unit per scaffold pair and strand ---------------------------------------------------------------------------------
static int run_per_pair(const mimeo_genome *A, const mimeo_genome *QG, const uint32_t *pair_t, const uint32_t *pair_q, const std::vector<uint8_t> &strands,
                        const mimeo_params *p, const Switches &sw, std::vector<std::vector<mimeo_alignment>> &per_pair, std::vector<char> &failed,
                        PairPaths *pp, CallTimes &tm) {
    const uint64_t npairs = strands.size();
    HIP_TRY(hipStreamSynchronize(stream()));   // what run_packed may have started before it declined
    // units in target-major order (stable in the caller's pair order): neighbouring units share the target index
    std::vector<uint64_t> ord(npairs);
    std::iota(ord.begin(), ord.end(), (uint64_t)0);
    std::stable_sort(ord.begin(), ord.end(), [&](uint64_t a, uint64_t b) { return pair_t[a] < pair_t[b]; });
    // Shared plus strand (self jobs): when the list names (t, q) and (q, t), t != q, both on the plus strand, and neither
    // scaffold has soft-masked bases, the unit of the pair with t < q also produces the HSPs of the other one, transposed
    // (k4_mirror_hsps): one seed scan and one gap-free stage instead of two.  Chain and gapped extension run per pair as
    // ever (their tie-breaks are not symmetric).  First occurrences only; MIMEO_MIRROR=0 switches it off (tests).
    host_plan::MirrorPairs mir{std::vector<uint64_t>(npairs, NO_PAIR), std::vector<char>(npairs, 0)};
    if (A == QG && sw.mirror) {
        std::vector<char> target_plane;   // soft-masked bases: target-only seeding rule
        for (const Scaffold &s : A->scaf) target_plane.push_back(s.fwd.sv_target != nullptr);
        mir = host_plan::mirror_pairs(pair_t, pair_q, strands, target_plane);
    }
    std::vector<Unit> units;
    uint64_t max_t = 1, max_q = 1;
    for (uint64_t k = 0; k < npairs; k++) {
        const uint64_t pk = ord[k];
        max_t = std::max(max_t, A->scaf[pair_t[pk]].len);
        max_q = std::max(max_q, QG->scaf[pair_q[pk]].len);
        for (uint32_t minus = 0; minus < 2; minus++) {
            if (!(strands[pk] & (minus ? MIMEO_STRAND_MINUS : MIMEO_STRAND_PLUS))) continue;
            if (!minus && mir.served[pk]) continue;
            const uint64_t mp = minus ? NO_PAIR : mir.mirror_of[pk];
            units.push_back(Unit{{pair_t[pk], pair_q[pk], minus, pk}, mp != NO_PAIR, mp});
        }
    }
    // index bytes still to be built per target / query scaffold: an index kept on the genome costs nothing.  When they exceed
    // the budget the pair matrix is cut into blocks of Bt targets x Bq queries: S + 2 S^2 / Bt builds instead of S + 2 S.
    std::vector<uint64_t> t_bytes(A->scaf.size(), 0), q_bytes(QG->scaf.size(), 0);
    const uint32_t all = (uint32_t)p->strand & MIMEO_STRAND_BOTH;
    for (const Unit &u : units) {
        const Scaffold &ts = A->scaf[u.t], &qs = QG->scaf[u.q];
        StrandView sv;
        if (!A->kept.count(IndexCache::kept_key(A, IndexCache::key_of(ts, 0, true, &sv)))) t_bytes[u.t] = seed_index_bytes(ts.len);
        if (!QG->kept.count(IndexCache::kept_key(QG, IndexCache::key_of(qs, (int)u.minus, false, &sv))))
            q_bytes[u.q] = seed_index_bytes(qs.len) * (all == MIMEO_STRAND_BOTH ? 2 : 1);
    }
    uint64_t budget = 0;
    int rc = sw.index_budget(&budget);
    if (rc) return rc;
    std::vector<Group> groups;   // of the batch at hand, as uploaded and as K6 left them
    BatchPath path{A, QG, A->scaf.data(), QG->scaf.data(), &g_stats.pair_strands, pp, {}, {}, {}};
    path.group_bound = [](const Unit &u) { return (uint64_t)(u.mirrored ? 2 : 1); };   // a group per work slot
    path.groups_to_device = [&](const std::vector<Slot> &slots, const std::vector<UnitWork> &work, uint64_t, uint32_t *ngroups) -> int {
        groups.resize(slots.size());
        memset(groups.data(), 0, groups.size() * sizeof(Group));
        for (size_t i = 0; i < slots.size(); i++) {
            Group &g = groups[i];
            g.T = work[i].d.T; g.Q = work[i].d.Q; g.tid = slots[i].t; g.qid = slots[i].q; g.minus = slots[i].minus;
        }
        int rc = g_groups.reserve(groups.size() * sizeof(Group));
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(g_groups.p, groups.data(), groups.size() * sizeof(Group), hipMemcpyHostToDevice, stream()));
        *ngroups = (uint32_t)groups.size();
        return 0;
    };
    path.collect = [&](const std::vector<Slot> &slots, uint32_t) -> int {
        HIP_TRY(hipMemcpyAsync(groups.data(), g_groups.p, groups.size() * sizeof(Group), hipMemcpyDeviceToHost, stream()));
        HIP_TRY(hipStreamSynchronize(stream()));
        std::vector<mimeo_alignment> host_aln;
        int rc = read_alignments(groups.back(), host_aln);
        if (rc) return rc;
        for (size_t gi = 0; gi < groups.size(); gi++) {
            const Group &g = groups[gi];
            if (g.overflow) {   // this pair hit a limit: it is left out, the others go on (utils.py:125-128: no `set -e`)
                record_failure(slots[gi].pair, g.tid, g.qid, g.minus ? '-' : '+', failed);
                continue;
            }
            g_stats.chained_hsps += g.nchain;
            auto &dst = per_pair[slots[gi].pair];
            dst.insert(dst.end(), host_aln.begin() + g.job0, host_aln.begin() + g.job0 + g.naln);
            if (pp) pp->take(slots[gi].pair, g.job0, (uint64_t)g.job0 + g.naln);
        }
        return 0;
    };
    return run_batches(units, t_bytes, q_bytes, budget, sw.max_units(max_t, max_q), path, p, sw, tm);
}

int align_units_impl(const mimeo_genome *A, const mimeo_genome *B, const uint32_t *pair_t, const uint32_t *pair_q, const uint8_t *pair_strand,
                     uint64_t npairs, const mimeo_params *p, mimeo_alignment **out, uint64_t *nout, uint64_t **path_first,
                     mimeo_path_block **path_blocks, uint64_t *npath_blocks) {
    auto t0 = std::chrono::steady_clock::now();
    memset(&g_stats, 0, sizeof g_stats);
    g_failed.clear();
    g_ext.new_call();
    const Switches sw;
    const mimeo_genome *QG = B ? B : A;
    bool uniform = true;   // every pair on the same strands: what run_jobs.sh asks for (wrappers.py:1031 --strand=both)
    const uint32_t all = (uint32_t)p->strand & MIMEO_STRAND_BOTH;
    std::vector<uint8_t> strands(npairs);
    for (uint64_t k = 0; k < npairs; k++) {
        if (pair_t[k] >= A->scaf.size() || pair_q[k] >= QG->scaf.size()) { set_error("pair index out of range"); return MIMEO_ERR_ARG; }
        strands[k] = (uint8_t)(pair_strand ? ((uint32_t)pair_strand[k] & all) : all);
        if (strands[k] != strands[0]) uniform = false;
    }
    std::vector<std::vector<mimeo_alignment>> per_pair(npairs);
    std::vector<char> failed(npairs, 0);
    CallTimes tm;
    int rc = 0;
    bool packed = false;
    PairPaths paths, *pp = path_first ? &paths : nullptr;
    if (pp) { pp->cnt.resize(npairs); pp->blk.resize(npairs); }
    HIP_TRY(hipStreamSynchronize(stream()));
    if (uniform && npairs) {
        mimeo_params ps = *p;
        ps.strand = (int32_t)strands[0];
        if (ps.strand && (rc = run_packed(A, QG, pair_t, pair_q, npairs, &ps, sw, per_pair, failed, pp, tm, &packed))) return rc;
    }
    if (!packed && (rc = run_per_pair(A, QG, pair_t, pair_q, strands, p, sw, per_pair, failed, pp, tm))) return rc;
    // What is left out is a SCAFFOLD pair: every entry of the list that names the (t, q) of a failed entry fails with it — a
    // duplicate, or the entry that carries the pair's other strand (dist.units_of_row) — and is reported once.
    if (!g_failed.empty()) {
        std::set<std::pair<uint32_t, uint32_t>> bad;
        for (uint64_t k = 0; k < npairs; k++)
            if (failed[k]) bad.emplace(pair_t[k], pair_q[k]);
        for (uint64_t k = 0; k < npairs; k++)
            if (!failed[k] && bad.count(std::make_pair(pair_t[k], pair_q[k]))) {
                failed[k] = 1;
                g_failed.emplace_back(k, MIMEO_ERR_LIMIT);
            }
    }
    for (uint64_t k = 0; k < npairs; k++)
        if (failed[k]) {   // a pair that hit a limit on one strand yields no rows at all (its lastz run failed)
            per_pair[k].clear();
            if (pp) { pp->cnt[k].clear(); pp->blk[k].clear(); }
        }
    // a pair's plus-strand alignments come before its minus-strand ones whichever batch made them
    for (uint64_t k = 0; k < npairs; k++)
        host_plan::plus_strand_first(per_pair[k], pp ? &pp->cnt[k] : nullptr, pp ? &pp->blk[k] : (std::vector<mimeo_path_block> *)nullptr);
    uint64_t total = 0, total_blocks = 0;
    for (auto &v : per_pair) total += v.size();
    if (pp) for (auto &v : pp->blk) total_blocks += v.size();
    mimeo_alignment *res = (mimeo_alignment *)malloc((total ? total : 1) * sizeof(mimeo_alignment));
    uint64_t *pfirst = pp ? (uint64_t *)malloc((total + 1) * sizeof(uint64_t)) : nullptr;
    mimeo_path_block *pblk = pp ? (mimeo_path_block *)malloc((total_blocks ? total_blocks : 1) * sizeof(mimeo_path_block)) : nullptr;
    if (!res || (pp && (!pfirst || !pblk))) { free(res); free(pfirst); free(pblk); set_error("host allocation failed"); return MIMEO_ERR_NOMEM; }
    uint64_t w = 0;
    for (auto &v : per_pair) { if (!v.empty()) memcpy(res + w, v.data(), v.size() * sizeof(mimeo_alignment)); w += v.size(); }
    if (pp) {   // in the order of the records
        uint64_t r = 0, b = 0;
        for (uint64_t k = 0; k < npairs; k++) {
            for (uint32_t c : pp->cnt[k]) { pfirst[r++] = b; b += c; }
            if (!pp->blk[k].empty()) memcpy(pblk + (b - pp->blk[k].size()), pp->blk[k].data(), pp->blk[k].size() * sizeof(mimeo_path_block));
        }
        pfirst[r] = b;
        *path_first = pfirst;
        *path_blocks = pblk;
        *npath_blocks = total_blocks;
    }
    *out = res;
    *nout = total;
    const ExtStats &est = tm.est;
    g_stats.alignments = total;
    g_stats.seed_hits = est.seed_hits;
    g_stats.scan_bytes_algorithmic = est.scan_bytes_algorithmic;
    g_stats.scan_bytes_kernel = est.scan_bytes_kernel;
    g_stats.scan_launches = est.heavy_launches;
    g_stats.scan_kernel_launches = est.heavy_kernel_launches;
    g_stats.walked_hits = est.walked;
    g_stats.followers = est.followers;
    g_stats.queue_reruns = est.reruns;
    g_stats.ms_index = tm.ms_index;
    g_stats.ms_scan = est.ms_heavy;
    g_stats.ms_scan_fill = est.ms_k34;
    g_stats.ms_extend = est.ms_tails;
    g_stats.ms_chain = tm.ms_chain;
    g_stats.ms_gapped = tm.ms_gapped;
    g_stats.ms_total = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (getenv("MIMEO_TRACE")) {
        extern double g_alloc_ms;
        fprintf(stderr, "[trace] call: %.1f ms in all, %.1f ms of it in hipMalloc / hipFree of work buffers (since the library was loaded: cumulative)\n", g_stats.ms_total, g_alloc_ms);
    }
    return 0;
}

int build_kept_indexes(mimeo_genome *g, const uint32_t *scaf, uint64_t n) {
    const uint64_t cnt = n ? n : g->scaf.size();
    for (uint64_t i = 0; i < cnt; i++) {
        const uint32_t id = n ? scaf[i] : (uint32_t)i;
        const Scaffold &s = g->scaf[id];
        for (int role = 0; role < 3; role++) {  // query +, query -, target + (only when it differs)
            StrandView sv;
            IndexCache::Key k = IndexCache::key_of(s, role == 1, role == 2, &sv);
            auto kk = std::make_tuple(id, std::get<1>(k), std::get<2>(k));
            if (g->kept.count(kk)) continue;
            SeedIndex idx;
            int rc = build_index(sv, idx, nullptr);
            if (rc) return rc;
            g->kept.emplace(kk, idx);
        }
    }
    HIP_TRY(hipStreamSynchronize(stream()));
    return 0;
}

int chain_gapped_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_hsps, const uint32_t *d_hsp_unit, uint64_t nhsps,
                        const mimeo_params *p, DeviceBuf &scratch, mimeo_alignment *d_aln, float *ms_chain,
                        float *ms_gapped, bool want_paths) {
    if (!ngroups || !nhsps) return 0;
    hipStream_t st = stream();
    // scratch: sorted HSPs | best | cand | pred | order
    size_t off_hs = 0, off_best = off_hs + nhsps * sizeof(mimeo_hsp), off_cand = off_best + nhsps * 8,
           off_pred = off_cand + nhsps * 8, off_order = off_pred + nhsps * 4, total = off_order + nhsps * 4;
    int rc = scratch.reserve(total);
    if (rc) return rc;
    char *b = (char *)scratch.p;
    static hipEvent_t e0 = nullptr, e1 = nullptr, e2 = nullptr;  // calls are blocking and single-threaded: one set will do
    if (!e0) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); HIP_TRY(hipEventCreate(&e2)); }
    HIP_TRY(hipEventRecord(e0, st));
    if ((rc = chain_device(d_groups, ngroups, d_hsps, d_hsp_unit, nhsps, p->chain, (mimeo_hsp *)(b + off_hs), (long long *)(b + off_best),
                           (long long *)(b + off_cand), (int *)(b + off_pred), (uint32_t *)(b + off_order))))
        return rc;
    HIP_TRY(hipEventRecord(e1, st));
    if ((rc = gapped_device(d_groups, ngroups, (const mimeo_hsp *)(b + off_hs), (const uint32_t *)(b + off_order), nhsps, p,
                            d_aln, want_paths)))
        return rc;
    HIP_TRY(hipEventRecord(e2, st));
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    float a = 0, c = 0;
    HIP_TRY(hipEventElapsedTime(&a, e0, e1));
    HIP_TRY(hipEventElapsedTime(&c, e1, e2));
    if (ms_chain) *ms_chain += a;
    if (ms_gapped) *ms_gapped += c;
    return 0;
}

}  // namespace mimeo
