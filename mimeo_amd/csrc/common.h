// common.h — shared declarations of the mimeo HIP engine (gfx950 only).
//
// Data layout in HBM:
//   a scaffold strand is stored as four 1-bit planes, interleaved word by word: pw[w] is a uint4
//   holding 32 bases (base i at bit (i & 31) of word (i >> 5)) of
//     .x lo — bit 0 of the 2-bit code (A0 C1 G2 T3)
//     .y hi — bit 1 of the 2-bit code; a transition (A<->G, C<->T) flips exactly this bit
//     .z nm — 1 where the base is not ACGT (scored as N)
//     .w sv — 1 where a valid 12of19 seed word starts in the QUERY role (no N inside the 19-base
//             window, and the window fits)
//   so one 64-byte cache line carries all planes of 128 consecutive bases: an extension touches
//   one or two lines per sequence instead of one per plane.  A scaffold with lower-case bases has
//   an extra plane svt = seed validity in the TARGET role (lastz excludes soft-masked target
//   bases from seeding).  PLANE_PAD zero words lie in front of word 0 and behind the last word
//   so that window loads never need a bounds check.
//   A second copy holds the lo / hi planes alone (uint2 per 32 bases, same padding): the K4 pre-filter gathers
//   ~200 bases around every seed hit and is bound by the bytes it pulls through L2, so it reads this
//   copy (6.4 + 4 = 10.4 bits per base and strand in all).
//   The seed index of a strand is CSR: off[2^24 + 1] (u32) and pos[nvalid] (u32, ascending
//   inside a bucket).  Key = (pext12(lo window) << 12) | pext12(hi window): the low 12 bits are
//   the transition bits, so the 13 words within one transition of a key differ only in the low
//   12 bits and a block of 4096 consecutive keys ("tile") is closed under them.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <functional>
#include <map>
#include <tuple>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/mimeo_hip.h"
#include "host_plan.h"
#include "queue_plan.h"

namespace mimeo {

constexpr int SEED_LEN = 19;
constexpr int SEED_WEIGHT = 12;
constexpr uint32_t NBUCKET = 1u << 24;
constexpr uint32_t TILE_WORDS = 4096;  // keys per join tile
constexpr uint32_t NTILE = NBUCKET / TILE_WORDS;
constexpr int PLANE_PAD = 8;  // u32 words (256 bases) of zero padding on both sides

void set_error(const std::string &msg);
int hip_fail(hipError_t e, const char *what, const char *file, int line);

#define HIP_TRY(call)                                                         \
    do {                                                                      \
        hipError_t e__ = (call);                                              \
        if (e__ != hipSuccess) return mimeo::hip_fail(e__, #call, __FILE__, __LINE__); \
    } while (0)

// device views ---------------------------------------------------------------------------
struct StrandView {
    const uint4 *pw;       // interleaved planes {lo, hi, nm, sv}, pointer to word 0
    const uint32_t *svt;   // target-role seed validity plane (word 0), or null: use pw[].w
    const uint2 *p2;       // the same lo / hi planes alone, 8 bytes per 32 bases (K4 pre-filter: half the bytes to gather)
    uint32_t len;          // bases
    uint32_t has_n;        // the strand holds at least one non-ACGT base
};

// Seed frames (K2, read by the fused seed-scan / extension kernel K34): every index entry carries the 192 bases
// [p - FRAME_LEFT, p - FRAME_LEFT + 192) around its seed start p as two bit planes brought into ONE alignment (bit 0 =
// base p - FRAME_LEFT), 12 words = three uint4 {lo0..lo3} {lo4,lo5,hi0,hi1} {hi2..hi5}.  Target and query frames of
// a seed hit then XOR word by word with no shifting, and every shift in the pre-filter is a compile-time constant.
// The seed end p + 19 sits at frame bit 128: the left walk (through the seed) owns bits 127 .. 32 (96 steps, six
// half-word blocks), the right walk bits 128 .. 191 (64 steps), and bits 13 .. 31 only serve the seed windows that
// END where the last left steps arrive.  Bit 31 of pos[] is set for an entry whose frame holds a non-ACGT base (the
// frame shows it as A): such a hit always goes to the exact walk.
constexpr int FRAME_LEFT = 109;            // frame bit 0 = base p - 109
constexpr int FRAME_WORDS = 6;             // per plane
constexpr uint32_t POS_MASK = 0x7FFFFFFFu;
constexpr uint32_t POS_NFLAG = 0x80000000u;

struct IndexView {
    const uint32_t *off;  // NBUCKET + 1
    const uint32_t *pos;  // bit 31: the entry's frame holds an N (POS_NFLAG)
    const uint4 *fr;      // 3 parts per entry, part k of entry i at fr[k * fr_stride + i]
    uint32_t fr_stride;
    uint32_t n;  // number of indexed positions
};

// host-side owner of one strand's planes
struct Strand {
    uint4 *base = nullptr;          // nwords + 2*PLANE_PAD interleaved words
    uint2 *slim = nullptr;          // nwords + 2*PLANE_PAD words of {lo, hi} only
    bool has_n = false;
    uint32_t *sv_target = nullptr;  // separate sv plane for the target role (soft-mask aware); null = same as sv
    uint32_t nwords = 0;
    uint32_t len = 0;
    StrandView view(bool as_target) const;
};

struct SeedIndex {
    uint32_t *off = nullptr;
    uint32_t *pos = nullptr;
    uint4 *fr = nullptr;
    uint32_t n = 0, fr_stride = 0;
    size_t pos_bytes = 0, fr_bytes = 0;  // allocation sizes (free-list keys)
    IndexView view() const { return IndexView{off, pos, fr, fr_stride, n}; }
    void release();
};
// device bytes of the seed index of one strand of `len` bases: offsets, positions, frames
inline uint64_t seed_index_bytes(uint64_t len) { return ((uint64_t)NBUCKET + 2) * 4 + len * (4 + 48); }

struct Scaffold {
    uint64_t len = 0;
    bool has_lower = false;
    Strand fwd, rc;
};

}  // namespace mimeo

struct mimeo_genome {
    std::vector<mimeo::Scaffold> scaf;
    std::vector<std::string> names;  // record ids when loaded from FASTA (ingest.hip); else empty
    // seed indexes kept across mimeo_align_pairs calls (mimeo_genome_keep_indexes); key =
    // (scaffold number, strand, target-role sv plane in use).  Only touched between calls and by the
    // calling thread at the start / end of a call.
    bool keep_indexes = false;
    mutable std::map<std::tuple<uint32_t, int, int>, mimeo::SeedIndex> kept;
    bool owns(const mimeo::Scaffold *s) const { return !scaf.empty() && s >= scaf.data() && s < scaf.data() + scaf.size(); }
};

namespace mimeo {

// stream used by every kernel launch of the library (created by mimeo_init)
hipStream_t stream();
void set_thread_stream(hipStream_t s);  // per-thread override (worker threads)
int device_id();
std::string last_error_copy();
bool initialised();

// K1: ASCII -> planes for both strands (k1_pack.hip)
int pack_scaffold(const uint8_t *d_ascii, uint64_t len, Scaffold &out);
void free_scaffold(Scaffold &s);

// streaming FASTA ingest (ingest.hip)
int load_fasta_impl(const char *const *paths, uint32_t npaths, const char *split_dir, mimeo_genome **out);

// K2: seed index of one strand (k2_index.hip)
// [p0, p1): index only the seed words that start in that range (chunks of a very large query; default = all)
int build_index(const StrandView &s, SeedIndex &out, float *ms, uint32_t p0 = 0, uint32_t p1 = 0xFFFFFFFFu);

// K3: index join (k3_join.hip).  Produces all seed hits of (T, Q) into a device buffer the
// caller owns (grown on demand).
struct DeviceBuf {
    void *p = nullptr;
    size_t cap = 0;
    bool view = false;     // a slice of an arena (another DeviceBuf owns the memory): never freed or grown through this handle
    int reserve(size_t bytes);
    void release();
    void set_view(void *ptr, size_t bytes) { p = ptr; cap = bytes; view = true; }
};
struct JoinTiming { float ms_count = 0, ms_fill = 0; };
// per-lane work state of K3 (a lane = one host thread + one stream working through units)
struct JoinCtx {
    unsigned long long *tile_count = nullptr, *tile_base = nullptr;
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    void release();
};
// exact mode: one host round trip for the hit count, then the fill (stage entry point, A/B heavy path)
int join_hits(JoinCtx &ctx, const IndexView &T, const IndexView &Q, int transitions, DeviceBuf &hits, uint64_t *nhits,
              JoinTiming *tm);

// K4: seed hits -> HSPs for a BATCH of units (k4_extend.hip, k34_fused.hip).  One unit = one (target scaffold,
// query scaffold, strand); the device table of UnitDesc is what every K4 kernel looks its two strands up in.
struct UnitDesc {
    StrandView T, Q;
    uint32_t same;  // target and query are the same strand of the same scaffold: diagonal 0 belongs to k4_diag0
    uint32_t pad[3];
};
struct UnitWork {  // host side: a unit with the seed indexes its heavy kernel reads
    UnitDesc d;
    IndexView ti, qi;
};
// a unit of the batch as the heavy kernels see it (K34 over all units in one launch; the walk-queue kernel likewise)
struct FusedUnit {
    IndexView T, Q;
    StrandView Tv, Qv;
    uint32_t unit;        // number in the batch (index into the UnitDesc table, tag of every record)
    uint32_t same;        // target and query are the same strand: the main diagonal belongs to k4_diag0
    uint64_t walk_base;   // this unit's region of the walk queue: eight shards of walk_cap entries from here
    uint64_t walk_cap;
};

struct ExtStats {
    uint64_t seed_hits = 0, walked = 0, walk_queue = 0, followers = 0, candidates = 0, reruns = 0;
    uint64_t scan_bytes_algorithmic = 0, scan_bytes_kernel = 0, heavy_launches = 0, heavy_kernel_launches = 0;
    float ms_heavy = 0, ms_k34 = 0, ms_walk = 0, ms_tails = 0;  // ms_k34: the K34 launches alone (event pair per launch)  // ms_walk: the exact walks of the walk queue (part of ms_tails)
};
// The extension stage of one batch: the heavy phase (K34 fused seed scan + pre-filter over all units of the batch in one
// launch, the exact walks of the hits it passes on; or, MIMEO_HEAVY=v1 for A/B checks, the stand-alone K3 join + K4 fast
// kernel of round 1 per unit) appending to batch-wide queues, then the tails ONCE per batch: walks beyond the frame,
// k4_diag0 of the self units, ONE radix sort of the followers of all units, segment resolution, entropy.  Two host
// synchronisations per batch.  Leaves nhsp HSPs in hsps / hsp_unit (device).
// How large the queues are, what an overflow teaches, when a batch is refused with MIMEO_ERR_SPLIT and how the arenas are
// cut and grow is policy, written once in queue_plan.h: shares, boosts and learn(), initial_caps() / walk_cap() / grow(),
// queue_slices() / arena_bytes() / queue_bytes(), sort_slices(), queue_budget() / must_split(), arena_want() and
// follower_key_bits().  ExtBatch feeds it counters and free memory and makes the HIP calls.
struct ExtQueues;     // k4_device.h
struct ExtCounters;
struct K34Buffers;    // k34.h
// development / test switches of a batch, read from the environment once per batch (k4_extend.hip: read_switches): MIMEO_HEAVY=v1,
// MIMEO_K4_STATS, MIMEO_TRACE, MIMEO_K4_VARIANT, MIMEO_K34_DEBUG, MIMEO_QUEUE_SHRINK (smaller queues; tests: force the rerun),
// MIMEO_QUEUE_BUDGET_MB (tests: force the split)
struct ExtSwitches {
    bool v1 = false, k4_stats = false, trace = false, budget_forced = false;
    int k4_variant = 0;
    uint32_t k34_dbg = 0;
    double shrink = 1.0;
    long budget_mb = 0;
};
struct ExtBatch {
    // mirror: mirror_dst_ on the device + one counter; funits: per-unit table of the heavy kernels (FusedUnit)
    DeviceBuf units, ctr, nsel, unit_hits, tile_hits, selfs, hits, bigcand, bigacc, mirror, funits;
    K34Buffers *k34_ = nullptr;   // K34's own buffers (k34.h: tile lists, split-pass plan, per-unit counters), owned
    // hipMalloc / hipFree of tens of GB cost seconds (C5 at full size spent 80 % of its wall time there): the queues of a batch are
    // slices of ONE allocation that only ever grows (arena_q, carved per batch: qbuf), the follower sort's buffers of another
    // (arena_s: sbuf).  The 8 GiB and 4 GiB of head-room they leave when they grow differ on purpose: the queue arena is allocated
    // first and leaves room for the sort arena too (queue_plan::arena_want).
    DeviceBuf arena_q, arena_s;
    DeviceBuf qbuf[queue_plan::Q_SLICES], sbuf[queue_plan::S_SLICES];
    DeviceBuf &hsps = qbuf[queue_plan::Q_HSPS], &hsp_unit = qbuf[queue_plan::Q_HSP_UNIT];   // what the batch leaves to the pipeline
    JoinCtx jc;
    hipEvent_t ev[6] = {};           // 0, 1: around the heavy phase; 3, 2: around the tails; 4, 5: around the seed-scan kernel (both passes)
    hipStream_t side = nullptr;      // k4_diag0 of the self units runs beside the heavy kernels
    hipEvent_t side_done = nullptr;
    std::vector<unsigned long long> h_unit_hits;
    // Boosts hold within one API call: every call starts from the random-sequence shares.  Boosts learned on one input would
    // size the queues of every later call on any other (a tandem-array job of 1e6 expected hits left boosts of ~100-300; the C4
    // row after it was cut into 125 batches instead of one, and a C2 call after that asked for 190 GiB of queues);
    // microsatellites flood the follower queue alone (C5: half of all hits), hence one boost per queue
    queue_plan::Boosts boost;
    void new_call() { boost = queue_plan::Boosts(); }
    // run = start (sizes the queues, enqueues the heavy phase on the calling thread's stream, waits for nothing) + finish (the
    // tails on the same stream: two host round trips; a batch whose queues overflowed is repeated there with room).  The
    // pipeline only calls run, one batch at a time: a batch is finished before the next one starts.
    // mirror_dst (optional, one entry per unit): unit u's HSPs are also emitted transposed (target <-> query) for unit
    // mirror_dst[u] (NO_MIRROR: none).  The plus-strand units (A, B) and (B, A) of a self job have transposed HSP sets —
    // seeds, x-drop walks, the per-diagonal rule, entropy and HOXD70 are all symmetric — so one heavy phase serves both
    // (DESIGN.md "Shared plus strand"); the mirror unit itself comes with empty indexes and launches nothing.
    // MIMEO_ERR_SPLIT (internal): the queues of this batch do not fit the free device memory — the caller cuts it in two.
    int run(const std::vector<UnitWork> &work, const mimeo_params *p, uint64_t *nhsp, ExtStats *st, const std::vector<uint32_t> *mirror_dst = nullptr);
    int start(const std::vector<UnitWork> &work, const mimeo_params *p, const std::vector<uint32_t> *mirror_dst = nullptr);
    int finish(uint64_t *nhsp, ExtStats *st);
    void release();
    // state of the batch between start and finish
    std::vector<UnitWork> w_;
    mimeo_params p_;
    std::vector<uint32_t> h_selfs_, mirror_dst_;
    std::vector<UnitDesc> h_units_;
    std::vector<FusedUnit> h_funits_;
    ExtSwitches sw_;
    queue_plan::Caps cap_;
    std::vector<uint64_t> walk_cap_u_;   // walk-queue capacity per unit and shard
    uint64_t walk_entries_ = 0;          // ... all regions together
    uint32_t nactive_ = 0;               // units of the batch that launch the heavy kernels
    double expect_hits_ = 0;
    queue_plan::KeyBits key_ = {0, 0, 0, false};
    bool started_ = false, splittable_ = false;
    ExtQueues *q_ = nullptr;   // the queues as the kernels see them, owned
    uint64_t arena_bytes() const { return queue_plan::arena_bytes(cap_, walk_entries_, !mirror_dst_.empty(), sw_.v1); }   // the queue arena at the current capacities
    uint64_t queue_bytes() const { return queue_plan::queue_bytes(cap_, walk_entries_, !mirror_dst_.empty(), sw_.v1); }   // ... plus what the rest of the batch may ask for meanwhile
    // the steps of start: the heavy phase of the batch on the calling thread's stream, with the current capacities = the queue
    // arena's slices, then K34 and the walk-queue kernel over all units or, MIMEO_HEAVY=v1, join + fast kernel per unit
    int enqueue_heavy(), carve_queues(), enqueue_k34(), enqueue_v1();
    // ... and of finish
    int tails(ExtCounters *c), resolve_followers(uint64_t nf), entropy(ExtCounters *c);
    int print_stats(const ExtCounters &c, uint64_t nf, uint64_t nm, bool over);
    int learn_and_grow(const queue_plan::Counts &fullest, const queue_plan::Counts &batch);
};
constexpr uint32_t NO_MIRROR = 0xFFFFFFFFu;
constexpr int MIMEO_ERR_SPLIT = -100;   // internal: never crosses the C-ABI
// largest batch the follower key can name for scaffolds of these lengths (unit bits = 64 - end bits - diagonal bits)
inline uint32_t ext_batch_max_units(uint64_t max_tlen, uint64_t max_qlen) { return queue_plan::max_units(max_tlen, max_qlen, SEED_LEN); }

// K5/K6: one group = one (target scaffold, query scaffold, strand) with its HSP range
// K6 takes up to MAX_BATCH anchors per group and round, K6_ROUND_ANCHORS over all groups (k6_gapped.hip: gapped_setup, k6_pick)
constexpr int MAX_BATCH = 128;
constexpr uint32_t K6_ROUND_ANCHORS = 32768;
struct Group {
    StrandView T, Q;
    uint32_t tid, qid, minus, nchain;
    uint64_t hsp_begin, hsp_end;
    uint32_t naln, overflow;
    // K6 round state: anchors are taken in order, nbatch of them in the round under way
    uint32_t next, nacc, nbatch, job0;
};
// K5 (k5_chain.hip): sort + chain + anchor order for every group
int chain_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_hsps, const uint32_t *d_hsp_unit, uint64_t nhsps,
                 int do_chain, mimeo_hsp *d_sorted, long long *d_best, long long *d_cand, int *d_pred, uint32_t *d_order);
// K6 (k6_gapped.hip): anchors -> gapped alignments; alignments of group g land at
// d_aln[hsp_begin .. hsp_begin + naln).  want_paths: the blocks of every returned alignment are kept for dense_paths_device
// (box rule: one trace pass after the last round); without it the launches are those of a call that knows no paths
int gapped_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_sorted, const uint32_t *d_order,
                  uint64_t nhsps, const mimeo_params *p, mimeo_alignment *d_aln, bool want_paths = false);
// alignments of all groups packed densely (group g: d_dense[job0 .. job0 + naln)); same stream as gapped_device
void dense_alignments_device(Group *d_groups, uint32_t ngroups, const mimeo_alignment *d_aln, mimeo_alignment *d_dense);
// ... and, after gapped_device(want_paths), their paths in the same order: first = ndense + 1 offsets (uint64) into blocks
// (mimeo_path_block), merged at the anchor
int dense_paths_device(const Group *d_groups, uint32_t ngroups, uint64_t ndense, DeviceBuf &first, DeviceBuf &blocks, uint64_t *nblocks);
// ---- super-scaffolds (pack.hip): small scaffolds concatenated behind spacers of N for K2 / K34 / K4 -------------------
typedef host_plan::Member PackMember;   // scaffold number, first base inside the super-scaffold, bases (host_plan.h)
struct SuperSide {
    std::vector<Scaffold> supers;                   // a super of ONE member at offset 0 is the scaffold itself (not owned)
    std::vector<bool> owned;
    std::vector<std::vector<PackMember>> members;
    std::vector<uint32_t> super_of, start_of;       // per scaffold number of the genome (0xFFFFFFFF: takes no part)
    void release();
};
int build_super_side(const mimeo_genome *g, const std::vector<uint32_t> &ids, uint32_t spacer, uint64_t member_max,
                     uint64_t super_len, SuperSide &out);
struct RegroupTables {   // device pointers
    const uint3 *unit_tab;                                // per unit of the batch: target super, query super, minus
    const uint32_t *t_off, *t_start, *t_len, *t_rank;     // members of target super s: slots t_off[s] .. t_off[s + 1]; rank in the target set
    const uint32_t *q_off, *q_start, *q_len, *q_rank;
    const uint32_t *pairidx;                              // [t_rank * nq + q_rank] -> index of the pair in pair_t / pair_q
    uint32_t nq, pad;
    const uint32_t *pair_t, *pair_q;                      // scaffold numbers of the pairs
    const StrandView *t_view, *q_view_fwd, *q_view_rc;    // per scaffold number
};
int regroup_hsps_device(mimeo_hsp *d_hsps, uint32_t *d_hunit, uint64_t nh, const RegroupTables &R, uint32_t npairs, DeviceBuf &groups,
                        uint32_t *ngroups);
int group_summary_device(const Group *d_groups, uint32_t ngroups, uint64_t out[3]);
int overflowed_groups_device(const Group *d_groups, uint32_t ngroups, uint64_t expect, std::vector<uint3> *out);
void release_pack_buffers();
void release_k5_buffers();   // k5_chain.hip
// chain + gapped extension of every group (pipeline.hip)
int chain_gapped_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_hsps, const uint32_t *d_hsp_unit, uint64_t nhsps,
                        const mimeo_params *p, DeviceBuf &scratch, mimeo_alignment *d_aln, float *ms_chain,
                        float *ms_gapped, bool want_paths = false);

// K7: depth runs (bedtools genomecov -bg); host in, host out (in chrom, start order)
int coverage_bedgraph_device(const mimeo_interval *h_iv, uint64_t n, const uint32_t *h_chrom_len, uint32_t nchrom,
                             std::vector<mimeo_depth_run> &out);
// K7: coverage collapse (k7_collapse.hip); host in, host out (sorted by chrom, start)
int coverage_collapse_device(const mimeo_interval *h_iv, uint64_t n, const uint32_t *h_chrom_len, uint32_t nchrom,
                             uint32_t min_cov, uint32_t min_len, std::vector<mimeo_interval> &out, float *ms);

// whole-job loop (pipeline.hip): pair k on the strands pair_strand[k] (null: p->strand for every pair)
int align_units_impl(const mimeo_genome *A, const mimeo_genome *B, const uint32_t *pair_t, const uint32_t *pair_q,
                     const uint8_t *pair_strand, uint64_t npairs, const mimeo_params *p, mimeo_alignment **out, uint64_t *nout,
                     uint64_t **path_first = nullptr, mimeo_path_block **path_blocks = nullptr, uint64_t *npath_blocks = nullptr);
// pairs of the last align call that hit a documented limit (their rows are left out, the call goes on): (pair index, code)
const std::vector<std::pair<uint64_t, int>> &failed_pairs();

void release_pipeline_buffers();  // pipeline.hip
int ungapped_units(const std::vector<UnitWork> &work, const mimeo_params *p, std::vector<std::vector<mimeo_hsp>> *per_unit,
                   ExtStats *st);  // pipeline.hip: the extension stage of a batch, HSPs per unit on the host
int build_kept_indexes(mimeo_genome *g, const uint32_t *scaf, uint64_t n);  // pipeline.hip

// K8: tandem scorer (k8_tandem.hip); host in, host out.  h_words (optional): the slices' mask words, the very words
// k8_tandem_count sums into h_masked; slice k owns (clipped length + 31) / 32 of them, in slice order.
int tandem_masked_device(const mimeo_genome *A, const mimeo_interval *h_iv, uint64_t n, int match, int mismatch, int delta,
                         int minscore, int maxperiod, uint32_t *h_masked, std::vector<uint32_t> *h_words = nullptr);

// K9: column statistics of alignment paths (k9_path_stats.hip); host in, host out.  Q is never null here.
int path_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                      const mimeo_path_block *blocks, uint64_t nblocks, mimeo_column_stats *out);
// K10: the same statistics clipped to target windows and summed into groups (k10_window_stats.hip); host in, host out.  Q is
// never null here, and nitems > 0.
int window_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                        const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_window_item *items, uint64_t nitems, uint64_t ngroups,
                        mimeo_window_stats *out);
// K11: the two rows of every alignment as letters (k11_path_text.hip); host in, three malloc'ed arrays out.  Q is never null here.
int path_text_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, uint64_t **row_first, uint8_t **trow, uint8_t **qrow);
// K12: regions linked into families through alignment paths (k12_link_regions.hip); host in, host out.  A self job, and
// nitems > 0.
int link_regions_device(const mimeo_genome *T, const mimeo_alignment *aln, uint64_t n, const uint64_t *first, const mimeo_path_block *blocks,
                        uint64_t nblocks, const mimeo_interval *regions, uint64_t nreg, const uint32_t *chrom_of_scaf, const mimeo_window_item *items,
                        uint64_t nitems, uint32_t min_cover_pct, uint32_t *family, uint64_t *links);
// K13: the pile of the alignments per target column and a base called from each (k13_pileup.hip); host in, host out.  Q is never
// null here, and nwin > 0; cols and call may each be null.
int path_pileup_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                       const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                       uint64_t nitems, mimeo_pileup_column *cols, uint8_t *call);
// K14: the pile of the inserted bases at the sites of a pileup and a base called from each insertion column (k14_insertions.hip);
// host in, host out.  Q is never null here, and nsites > 0; res, icols and icall may each be null.
int path_insertions_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                           const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                           uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, mimeo_insert_result *res, mimeo_insert_column *icols,
                           uint8_t *icall);
// K15: one row of text per item of a pileup, in its window's columns with the sites' insertion columns opened up (k15_stack.hip);
// host in, two malloc'ed arrays out (and res, the caller's, which may be null).  Q is never null here.
int path_stack_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                      const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                      uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, mimeo_stack_row *res, uint64_t **row_first, uint8_t **rows);
// K16: the six column counts and the query stretch of every item of a pileup against a supplied call (k16_call_stats.hip);
// host in, host out.  Q is never null here.
int path_call_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                           const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                           uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, const uint8_t *call, const uint8_t *icall, mimeo_call_stats *out);

// K17: terminal repeats of features, both orientations of every item (k17_terminal.hip); host in, records into the caller's
// `out`, two malloc'ed arrays out.
int terminal_repeats_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, const mimeo_terminal_params *p, mimeo_alignment *out,
                            uint64_t **path_first, mimeo_path_block **blocks, uint64_t *nblocks);
// K18: the target-site duplication at the two ends of every item (k18_flank.hip); host in, records into the caller's `out`.
int flank_repeats_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, const mimeo_flank_params *p, mimeo_flank_repeat *out);
// K19: the longest open run of the six reading frames of every item (k19_frames.hip); host in, 6 n records into the caller's `out`.
int open_frames_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, uint32_t flags, mimeo_open_frame *out);
}  // namespace mimeo
