/*
 * mimeo_hip.h — C-ABI of libmimeo_hip.so, the MI355X (gfx950) engine behind the
 * `mimeo self | x | map` hot path.
 *
 * What this boundary replaces in the reference (Adamtaranto/mimeo):
 *   the reference has no library API for its hot path; it builds a shell script
 *   (src/mimeo/wrappers.py:899-1271 self_LZ_cmds, :683-896 xspecies_LZ_cmds,
 *   :525-680 map_LZ_cmds) and runs it with src/mimeo/utils.py:213-254 run_cmd.
 *   Every entry point below cites the command line(s) of that script whose work
 *   it performs.  The Python host (mimeo_amd/) binds these with ctypes; see
 *   INTEGRATION.md for the stub a reference maintainer would add.
 *
 * Conventions
 *   - plain pointers and sizes only; no C++/torch types cross the boundary;
 *   - every function returns 0 on success, <0 on error; the message is read with
 *     mimeo_last_error() (reference convention: non-zero exit of run_jobs.sh ->
 *     RuntimeError, utils.py:194-210);
 *   - buffers returned through `**out` are allocated by the library and released
 *     with mimeo_free(); inputs are borrowed for the duration of the call;
 *   - calls are blocking; a handle must not be used from two threads at once;
 *   - coordinates are 0-based half-open inside the ABI.  The origin-one `start1`
 *     / `start2+` columns of LASTZ's `general` format (wrappers.py:1031) are
 *     produced by the host writer, not here.
 *   - there is NO CPU fallback: every entry point that computes fails with
 *     MIMEO_ERR_NO_DEVICE when no gfx950 device is usable.
 */
#ifndef MIMEO_HIP_H
#define MIMEO_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MIMEO_ABI_VERSION 3

enum {
    MIMEO_OK = 0,
    MIMEO_ERR_ARG = -1,        /* bad argument (null pointer, id out of range, ...) */
    MIMEO_ERR_NO_DEVICE = -2,  /* no usable HIP device / library not initialised   */
    MIMEO_ERR_HIP = -3,        /* a HIP runtime call failed                         */
    MIMEO_ERR_NOMEM = -4,      /* host or device allocation failed                  */
    MIMEO_ERR_LIMIT = -5       /* input exceeds a documented limit                  */
};

/* Strand selector == lastz --strand=plus|minus|both (wrappers.py:1031 passes both). */
enum { MIMEO_STRAND_PLUS = 1, MIMEO_STRAND_MINUS = 2, MIMEO_STRAND_BOTH = 3 };

/* Anchor rule of the gapped stage (mimeo_params.anchor_rule): which anchors are skipped.
 *   MIMEO_ANCHOR_BOX  an anchor inside the (t, q) box of an earlier alignment of its (pair, strand)
 *                     (alignment specification v1, rule 6; the default)
 *   MIMEO_ANCHOR_PATH an anchor on a match/mismatch column of the path of an earlier alignment of its
 *                     (pair, strand): lastz's documented --gapped rule.  lastz also bounds a new extension
 *                     by earlier alignments: mimeo_params.bound_extensions adds that (opt-in, path rule only;
 *                     the project's own statement of it, parity unpinned; DESIGN.md §2 rule 7). */
enum { MIMEO_ANCHOR_BOX = 0, MIMEO_ANCHOR_PATH = 1 };

/*
 * Alignment parameters == the lastz flags the reference passes
 * (wrappers.py:1025-1037 / 786-798 / 607-653) plus the LASTZ defaults they imply.
 * mimeo_params_default() fills the values in brackets.  anchor_rule selects the skip rule of
 * the gapped stage (MIMEO_ANCHOR_*); any other value is MIMEO_ERR_ARG.  bound_extensions = 1 (only with
 * MIMEO_ANCHOR_PATH; anything else is MIMEO_ERR_ARG) bounds every gapped extension by the earlier alignments of its
 * (pair, strand): a DP cell on or beyond the nearest earlier path on either side of the anchor's diagonal is dead, so
 * the alignments of a (pair, strand) neither cross nor run onto each other.  It took the first reserved slot: size and
 * the other offsets are unchanged.
 */
typedef struct mimeo_params {
    int32_t hspthresh;    /* --hspthresh [3000]; also the gapped threshold (lastz default)  */
    int32_t xdrop;        /* ungapped x-drop [910 = 10*sub[A][A]]; >= 500 (MIMEO_ERR_ARG below)  */
    int32_t ydrop;        /* gapped y-drop [9400 = open + 300*extend]                      */
    int32_t gap_open;     /* [400]                                                        */
    int32_t gap_extend;   /* [30]                                                         */
    int32_t transitions;  /* seed tolerates one transition [1] (lastz default)            */
    int32_t entropy;      /* --entropy [1]                                                */
    int32_t chain;        /* --chain [1]                                                  */
    int32_t gapped;       /* --gapped [1]                                                 */
    int32_t strand;       /* --strand [MIMEO_STRAND_BOTH]                                 */
    int32_t anchor_rule;  /* gapped-stage skip rule [MIMEO_ANCHOR_BOX]                    */
    int32_t bound_extensions; /* bound extensions by earlier alignments [0]; 1 needs MIMEO_ANCHOR_PATH */
    int32_t reserved[4];
} mimeo_params;

/* One raw seed hit: 0-based starts of the 19-base seed window (12of19, lastz default seed). */
typedef struct mimeo_seed_hit {
    uint32_t tpos;
    uint32_t qpos; /* on the strand being scanned (reverse-complement coordinates for '-') */
} mimeo_seed_hit;

/* One gap-free HSP (lastz --gfextend output, after --entropy and --hspthresh). */
typedef struct mimeo_hsp {
    uint32_t tstart;
    uint32_t qstart; /* strand coordinates, as above */
    uint32_t length;
    uint32_t flags;  /* bit0: survives --chain (set by mimeo_chain_hsps / align) */
    int64_t score;   /* entropy-adjusted score (== raw when entropy is off) */
    int64_t raw_score;
} mimeo_hsp;

/*
 * One gapped alignment == one row of lastz --format=general:name1,strand1,start1,
 * end1,length1,name2,strand2,start2+,end2+,length2,score,identity (wrappers.py:1031).
 * qstart/qend are on the query PLUS strand (like start2+/end2+), 0-based half-open.
 */
typedef struct mimeo_alignment {
    uint32_t tid;    /* index of the target scaffold in genome A */
    uint32_t qid;    /* index of the query scaffold in genome B (or A for self) */
    uint32_t tstart, tend;
    uint32_t qstart, qend;
    int64_t score;
    uint32_t id_n;   /* identity numerator: matched columns                         */
    uint32_t id_d;   /* identity denominator: matched + mismatched columns (no gaps) */
    uint32_t qstrand; /* 0 '+', 1 '-' */
    uint32_t reserved;
} mimeo_alignment;

/* Half-open interval on a chromosome, BED-interpreted (wrappers.py:1120). */
typedef struct mimeo_interval {
    uint32_t chrom;
    uint32_t start;
    uint32_t end;
} mimeo_interval;

/* Per-call statistics of the last mimeo_align_pairs / stage call (metrics). */
typedef struct mimeo_stats {
    uint64_t pair_strands;        /* (target, query, strand) units processed              */
    uint64_t seed_hits;           /* raw seed hits produced by the seed-scan kernel        */
    uint64_t hsps;                /* HSPs >= hspthresh                                    */
    uint64_t chained_hsps;
    uint64_t alignments;
    uint64_t query_bases_scanned; /* sum over pair-strands of Lq                           */
    uint64_t scan_bytes_algorithmic; /* SURVEY §8(d) B_scan summed over pair-strands       */
    uint64_t scan_bytes_kernel;   /* compulsory bytes of the seed-scan kernel   */
    double ms_index;              /* HIP-event time in the index-build kernels              */
    double ms_scan;               /* HIP-event time of the heavy phase: the fused seed-scan / pre-filter / walk kernels (K34) */
    double ms_extend;             /* the tails of the gap-free stage, once per batch: long walks, follower sort + resolution, entropy */
    double ms_chain;
    double ms_gapped;
    double ms_collapse;
    double ms_total;              /* host wall time of the call                            */
    uint64_t scan_launches;       /* units (target, query, strand) the seed-scan kernel worked off in ms_scan_fill (one launch per unit until ABI 2) */
    double ms_scan_fill;          /* HIP-event time of the seed-scan kernels (K34, the roofline kernel), back to back per batch */
    uint64_t index_blocks;        /* blocks the pair matrix was cut into so that the seed indexes fit in memory (1 = none) */
    uint64_t batches;             /* batches of units the call was worked off in (tails, chain and gapped stage run once per batch) */
    uint64_t queue_reruns;        /* batches repeated because a queue sized for random sequence overflowed (repeat-rich units) */
    uint64_t walked_hits;         /* seed hits the pre-filter could not dismiss: walked exactly */
    uint64_t followers;           /* hits with an earlier seed hit of their diagonal in reach: resolved after one sort per batch */
    uint64_t super_units;         /* units of super-scaffolds (small scaffolds packed behind spacers: fragmented assemblies); 0 = the call ran one unit per scaffold pair and strand */
    uint64_t scan_kernel_launches; /* launches of the seed-scan kernel K34 (first pass) in ms_scan_fill: one per BATCH of units (ABI 3) */
} mimeo_stats;

typedef struct mimeo_genome mimeo_genome; /* opaque: device-resident packed scaffolds */

/* ---- lifecycle ------------------------------------------------------------------ */

/* ABI version of the loaded library (compare with MIMEO_ABI_VERSION). Never fails. */
int mimeo_abi_version(void);

/* Select HIP device `device` for this process and create the library's streams.
 * One process drives one GPU (multi-GPU = one process per GPU). */
int mimeo_init(int device);
void mimeo_shutdown(void);

/* Message of the last failing call on this thread ("" if none). */
const char *mimeo_last_error(void);

/* Fill *p with the LASTZ defaults listed at mimeo_params. */
int mimeo_params_default(mimeo_params *p);

int mimeo_get_stats(mimeo_stats *out);

void mimeo_free(void *p);

/* ---- genome ingest (replaces utils.py:274-309 splitFasta + lastz's own file read) --- */

/*
 * Upload `nscaf` scaffolds given as concatenated ASCII bases (`bases`, any case,
 * anything outside ACGTacgt is treated as N) with `offsets[nscaf+1]` delimiting
 * them, and pack them on the device into 2-bit bit-planes + N / soft-mask planes
 * for both strands (kernel K1).  Lower-case target bases are excluded from seeding
 * and N from seeding on both sides, as lastz does by default.
 */
int mimeo_genome_create(uint32_t nscaf, const uint8_t *bases, const uint64_t *offsets,
                        mimeo_genome **out);
void mimeo_genome_destroy(mimeo_genome *g);
int mimeo_genome_nscaf(const mimeo_genome *g, uint32_t *nscaf);
int mimeo_genome_length(const mimeo_genome *g, uint32_t scaf, uint64_t *length);

/*
 * Streaming FASTA ingest: replaces splitFasta + chromlens + the Biopython parse
 * (src/mimeo/utils.py:274-309, 502-557; call sites run_self.py:199-224).  Every
 * record of every file in `paths` (in order) becomes one scaffold; the record id is
 * the first word of the header line, as Biopython's rec.id.  A host thread parses
 * record i+1 into pinned memory while record i is copied and packed (K1).  A
 * duplicate id is MIMEO_ERR_ARG with the reference's message (utils.py:300-306).
 * If `split_dir` is non-NULL one `<id>.fa` per record is also written there — the
 * side effect of the reference's --adir/--bdir.  `mimeo_genome_name` returns a
 * pointer owned by the genome ("" for genomes made by mimeo_genome_create).
 */
int mimeo_genome_load_fasta(const char *const *paths, uint32_t npaths, const char *split_dir,
                            mimeo_genome **out);
int mimeo_genome_name(const mimeo_genome *g, uint32_t scaf, const char **name);

/*
 * Seed-index residency.  lastz rebuilds the target's seed table in every one of the S^2 runs
 * of run_jobs.sh (call site wrappers.py:1028-1031); mimeo_align_pairs builds the index of a
 * scaffold strand once per call and, by default, gives it back when the call returns.  With
 * keep != 0 the indexes that later calls build for scaffolds of `g` stay attached to the handle
 * (64 MiB + 52 bytes per base and strand — offsets, positions and the seed frames the fused seed-scan
 * kernel streams: a 1 Gbp genome, both strands, is 117 GB of the 288 GB)
 * and are reused by every later call, so a job may be issued as several calls (one per target
 * scaffold, say) without paying for the tables again.  mimeo_genome_drop_indexes releases the
 * indexes (both strands) of the listed scaffolds, or all of them when n == 0;
 * mimeo_genome_destroy releases them too.  Results never depend on this setting.
 */
int mimeo_genome_keep_indexes(mimeo_genome *g, int keep);
/* Build (and keep: implies keep != 0) the indexes of the listed scaffolds now — both strands, and the
 * soft-mask-aware target variant where the scaffold has lower-case bases; n == 0: every scaffold. */
int mimeo_genome_build_indexes(mimeo_genome *g, const uint32_t *scaf, uint64_t n);
int mimeo_genome_drop_indexes(mimeo_genome *g, const uint32_t *scaf, uint64_t n);

/* ---- stage entry points (parity tests, profiling) ----------------------------- */

/*
 * lastz seed stage (SURVEY §8a A6+A7): build the 12of19 seed index of target
 * scaffold `tid` of T and of query scaffold `qid` of Q on strand `qstrand`
 * (0 '+', 1 '-'), and return every seed hit.  Order of the returned hits is
 * unspecified; the multiset is exact.
 */
int mimeo_seed_hits(const mimeo_genome *T, uint32_t tid, const mimeo_genome *Q, uint32_t qid,
                    uint32_t qstrand, const mimeo_params *p, mimeo_seed_hit **out, uint64_t *nout);

/*
 * lastz --gfextend --entropy --hspthresh (A8): seed hits -> gap-free HSPs with the
 * per-diagonal "already extended" suppression.  Returned sorted by
 * (tstart-qstart, tstart, length).
 */
int mimeo_ungapped_hsps(const mimeo_genome *T, uint32_t tid, const mimeo_genome *Q, uint32_t qid,
                        uint32_t qstrand, const mimeo_params *p, mimeo_hsp **out, uint64_t *nout);

/*
 * lastz --chain alone (A9; wrappers.py:1031), a stage inside lastz exposed for parity tests like the two above:
 * the n HSPs of ONE (target, query, strand) are copied to out[0 .. n) in (tstart, qstart, length) order with bit 0
 * of `flags` set on the members of the best chain (ties: earliest predecessor, earliest end) and cleared on the
 * others.  Runs K5 as mimeo_align_pairs does (the kernel is chosen by the number of HSPs).  out: n records, the caller's.
 */
int mimeo_chain_hsps(const mimeo_hsp *in, uint64_t n, mimeo_hsp *out);

/*
 * One full `lastz t.fa q.fa ...` invocation (A6-A10; wrappers.py:1025-1037): all
 * requested strands of one (target, query) pair -> gapped alignments.
 */
int mimeo_align_pair(const mimeo_genome *T, uint32_t tid, const mimeo_genome *Q, uint32_t qid,
                     const mimeo_params *p, mimeo_alignment **out, uint64_t *nout);

/* ---- whole-job entry points ---------------------------------------------------- */

/*
 * The per-pair loop of run_jobs.sh (wrappers.py:1015-1059): for k in [0,npairs)
 * align target scaffold pair_t[k] of A against query scaffold pair_q[k] of B
 * (B == NULL: of A, i.e. `mimeo self`).  Results are concatenated in pair order;
 * the host applies the awk/sort filter (A11) when it writes the TAB.
 *
 * How the pairs are worked off is the library's business and changes no record: units
 * (target, query, strand) in batches; when the list is a full cross product with at least eight
 * scaffolds of at most 6 Mbp on one side (and no kept indexes), they are concatenated behind spacers
 * of N into super-scaffolds for the seed index and the gap-free stage, and every HSP is handed
 * back to its scaffold pair before chaining and gapped extension (mimeo_stats.super_units > 0;
 * DESIGN.md "Fragmented assemblies"); in a self job (B == NULL) the plus-strand units of (t, q) and
 * (q, t) share one seed scan and gap-free stage when neither scaffold has soft-masked bases (DESIGN.md
 * "Shared plus strand").  Limits: scaffolds below 2^31 - 256 bases.  A pair whose gapped extension
 * needs a DP band beyond 65 536 columns is LEFT OUT — no row of it is returned,
 * the other pairs are, the call returns 0 and mimeo_get_failed_pairs names the pair: the reference's
 * run_jobs.sh has no `set -e`, a failing lastz run costs its own pair's rows only (utils.py:125-128,
 * :194-210 look at the last command's status).
 */
int mimeo_align_pairs(const mimeo_genome *A, const mimeo_genome *B, const uint32_t *pair_t,
                      const uint32_t *pair_q, uint64_t npairs, const mimeo_params *p,
                      mimeo_alignment **out, uint64_t *nout);

/*
 * The same loop with the strands chosen per pair: pair k is aligned on the strands pair_strand[k]
 * (MIMEO_STRAND_PLUS | MIMEO_STRAND_MINUS, masked with p->strand; pair_strand == NULL: p->strand for every
 * pair, i.e. mimeo_align_pairs).  This is what a rank's share of a sharded self job looks like
 * (mimeo_amd/dist.py deal_units): all minus-strand units of its target rows, and the plus-strand units
 * of the unordered scaffold pairs dealt to it in BOTH orders, so that the shared plus strand applies.
 * Results are concatenated in pair order, a pair's plus-strand rows first.
 *
 * What is left out at a limit (mimeo_align_pairs) is a SCAFFOLD pair, not an entry of the list: when a group of (t, q)
 * hits a limit on either strand, every entry k of the call with (pair_t[k], pair_q[k]) == (t, q) yields no row and no
 * path block, whatever strands it names, and mimeo_get_failed_pairs reports each such entry once — a duplicate of the
 * pair, and the entry that carries the pair's other strand, included.  The set of failed scaffold pairs depends neither
 * on how the call is worked off nor on the entry point.  (Across calls nothing is known: a caller that spreads a pair's
 * strands over calls or ranks drops the pair itself — workflow.drop_failed_pairs.)
 */
int mimeo_align_units(const mimeo_genome *A, const mimeo_genome *B, const uint32_t *pair_t,
                      const uint32_t *pair_q, const uint8_t *pair_strand, uint64_t npairs,
                      const mimeo_params *p, mimeo_alignment **out, uint64_t *nout);

/*
 * mimeo_align_units with the alignments themselves: where the gaps are, and which base is paired with which.  `out` / `nout`
 * are byte for byte what mimeo_align_units returns for the same arguments.  The path of alignment i is the gap-free blocks
 * blocks[path_first[i] .. path_first[i + 1]): path_first has *nout + 1 entries, *nblocks = path_first[*nout].  All three
 * arrays are released with mimeo_free.  Under the box rule the paths cost one more traceback of the returned alignments;
 * a call of mimeo_align_units pays nothing for them.
 *
 * Coordinates of a block: `t` on the target plus strand; `q` on the strand that was aligned — for qstrand == 1 these are
 * reverse-complement coordinates, as mimeo_seed_hit.qpos (the record's qstart / qend stay on the plus strand: with Lq the
 * query's length, qstart = Lq - (q_last + len_last) and qend = Lq - q_first); `len` columns of the diagonal from (t, q),
 * each a match or a mismatch.
 *
 * What a caller may rely on:
 *   - the blocks of one alignment are strictly increasing in t and in q and never touch on a diagonal (two that would are
 *     one block);
 *   - between two consecutive blocks exactly one of t and q jumps (a gap), or both do (an insertion next to a deletion);
 *   - the first block starts at (tstart, q_first) and the last one ends at tend;
 *   - the sum of len over an alignment's blocks is its id_d.
 * --gapped off: one block per alignment.  A pair with a half extension whose traceback alone exceeds the trace pool (a share
 * of the free device memory) is left out with MIMEO_ERR_LIMIT like a pair whose band exceeds the DP limit
 * (mimeo_get_failed_pairs) — only here, where paths are asked for.
 *
 * A new symbol beside the old ones: no struct changed size or meaning and no existing entry point changed, so
 * MIMEO_ABI_VERSION stays 3; a host that needs paths checks for the symbol.
 */
typedef struct mimeo_path_block {
    uint32_t t, q, len;
} mimeo_path_block;
int mimeo_align_units_paths(const mimeo_genome *A, const mimeo_genome *B, const uint32_t *pair_t,
                            const uint32_t *pair_q, const uint8_t *pair_strand, uint64_t npairs,
                            const mimeo_params *p, mimeo_alignment **out, uint64_t *nout,
                            uint64_t **path_first, mimeo_path_block **blocks, uint64_t *nblocks);

/*
 * Column statistics of alignment paths (kernel K9): what the aligned columns of each alignment ARE, where the path only says
 * where they lie.  Replaces nothing in the reference, which keeps lastz's identity column and no alignment; it is what a
 * substitution divergence (Kimura's two-parameter distance needs transitions and transversions apart) and the NM / de tags
 * of a PAF row are computed from.  The sequences are read from the device-resident genomes: no base text crosses the ABI.
 *
 * aln[0 .. n) are records as the align entry points return them, of target scaffolds of T and query scaffolds of Q (NULL: of
 * T, a self job); the path of record i is blocks[path_first[i] .. path_first[i + 1]) in the coordinates of mimeo_path_block
 * above (t on the target plus strand, q on the strand that was aligned); path_first has n + 1 entries.  Of a record only tid,
 * qid and qstrand are read.  out[i] receives, for the columns of record i's blocks with target base x and query base y,
 *   ambiguous      x or y is not one of ACGT
 *   matches        x == y
 *   transitions    A<->G or C<->T
 *   transversions  every other pair of different bases
 * and from the jumps between consecutive blocks the gaps, with the meaning of I and D in a CIGAR whose reference is the
 * target: ins_runs / ins_bases are the runs and the bases of query sequence absent from the target, del_runs / del_bases
 * those of target sequence absent from the query (both jump: one run of each).
 *
 * What a caller may rely on, for paths that mimeo_align_units_paths returned with these records:
 *   - matches == id_n, and matches + transitions + transversions + ambiguous == id_d;
 *   - del_bases == tend - tstart - id_d and ins_bases == qend - qstart - id_d;
 *   - the counts are exact integers: they depend on nothing but the sequences and the blocks.
 * Any path is accepted that keeps the contract of mimeo_path_block; everything is checked before the device sees it, and a
 * violation is MIMEO_ERR_ARG with a message naming the record and the block: path_first[0] == 0, path_first non-decreasing,
 * path_first[n] == nblocks; tid / qid inside their genomes, qstrand 0 or 1; len >= 1, t + len and q + len inside their
 * scaffolds; the blocks of an alignment increasing and non-overlapping.  An alignment without blocks counts nothing.
 * n == 0 returns MIMEO_OK at once.  Records and blocks go to the device in slices of bounded size, so a job of any size runs
 * in the memory that is free next to the genomes.
 *
 * A new symbol beside the old ones, like mimeo_align_units_paths: MIMEO_ABI_VERSION stays 3; a host that needs it checks for
 * the symbol.
 */
typedef struct mimeo_column_stats {
    uint32_t matches, transitions, transversions, ambiguous;   /* their sum is id_d */
    uint32_t ins_runs, ins_bases, del_runs, del_bases;         /* I / D of the CIGAR: runs and bases */
} mimeo_column_stats;                                          /* 32 bytes */
int mimeo_path_stats(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                     const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                     mimeo_column_stats *out /* caller's, n entries */);

/*
 * Column statistics of alignment paths clipped to target windows and accumulated into groups (kernel K10): what ties a
 * divergence to a REGION of the target — a repeat of `mimeo self`, a candidate of `mimeo x` — where mimeo_path_stats counts
 * whole alignments.  An alignment routinely runs past a region's ends or across several regions, and the host holds no
 * sequence text to clip with: the clipping is done on the device, from the device-resident genomes.
 *
 * T, Q, aln, n, path_first, blocks and nblocks are those of mimeo_path_stats.  An item asks for the path of record `aln`
 * clipped to the window [w0, w1) on the plus strand of that record's target scaffold, added to group `group`.  With the
 * path's blocks b_0 .. b_{m-1}, p_k = b_{k-1}.t + b_{k-1}.len the end of the block before b_k, dt_k = b_k.t - p_k and
 * dq_k = b_k.q - (b_{k-1}.q + b_{k-1}.len):
 *   columns     a column of b_k is counted iff its target base lies in [w0, w1); it is ambiguous, a match, a transition or a
 *               transversion as for mimeo_path_stats: the N planes mask first;
 *   del_bases   the overlap of [p_k, b_k.t) with [w0, w1);
 *   del_runs    the run is counted iff dt_k > 0 and w0 <= p_k < w1: a run belongs to the window that holds its first base;
 *   ins_runs, ins_bases   for dq_k > 0 the run and all dq_k bases are counted iff w0 <= p_k < w1: the insertion sits in front
 *               of target base p_k (where both sequences jump, this is the I-then-D order of a CIGAR); an insertion is
 *               never split.
 * What follows, and what a caller may rely on:
 *   - all eight fields are additive over any partition of a window;
 *   - over a partition of [tstart, tend) they sum to what mimeo_path_stats returns for the alignment;
 *   - a window that misses the alignment counts nothing, and so does an empty window (w0 == w1), which is legal;
 *   - matches + transitions + transversions + ambiguous + del_bases is the length of the overlap of the window with
 *     [tstart, tend).
 * out[g], g < ngroups, is the sum over the items with group == g; a group without items is zero.  Items come in any order,
 * and an alignment may appear in any number of them.  The counters are 64 bits: a region of megabases under hundreds of rows
 * exceeds 2^32.  They are exact integers and depend on nothing but the sequences, the blocks and the items.
 *
 * Everything is checked before the device sees it; a violation is MIMEO_ERR_ARG with a message naming the item (or, for the
 * paths, the record and the block): everything mimeo_path_stats checks; aln < n, group < ngroups, w0 <= w1, and w1 <= the
 * length of the record's target scaffold.  nitems == 0 zeroes out[0 .. ngroups) and returns MIMEO_OK.  Records and blocks go
 * to the device in the same bounded slices as for mimeo_path_stats, and only the slices that an item asks for.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
typedef struct mimeo_window_item {
    uint32_t aln, group, w0, w1;
} mimeo_window_item;                                           /* 16 bytes */
typedef struct mimeo_window_stats {
    uint64_t matches, transitions, transversions, ambiguous;   /* columns whose target base lies in the window */
    uint64_t ins_runs, ins_bases, del_runs, del_bases;         /* I / D of the CIGAR: runs and bases */
} mimeo_window_stats;                                          /* 64 bytes */
int mimeo_path_window_stats(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                            const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                            const mimeo_window_item *items, uint64_t nitems, uint64_t ngroups,
                            mimeo_window_stats *out /* caller's, ngroups entries */);

/*
 * The text of alignment paths (kernel K11): the two rows of every pairwise alignment, target over query, as letters — what a
 * MAF block or a cs:Z: tag is written from, and the way to read a single aligned base.  The host holds no sequence text
 * (the FASTA is streamed to the device); the rows are made on the device from the resident genomes.
 *
 * T, Q, aln, n, path_first, blocks and nblocks are those of mimeo_path_stats, and so is every check: a violation is
 * MIMEO_ERR_ARG before anything is uploaded, with a message that starts with "mimeo_path_text:" and names the record and the
 * block.  Of a record only tid, qid and qstrand are read.  With X the target's forward strand and Y the query's forward
 * strand for qstrand == 0, its stored reverse complement for qstrand == 1 (the coordinates of mimeo_path_block; nothing is
 * flipped), row i is trow[row_first[i] .. row_first[i + 1]) over the same range of qrow: two rows of equal length, no
 * padding, no terminator.  For the blocks b_0 .. b_{m-1} of the path, in order:
 *   between blocks  for k > 0, with dq = b_k.q - (b_{k-1}.q + b_{k-1}.len) and dt likewise: first dq insertion columns, '-'
 *                   in trow over the query bases Y[b_{k-1}.q + b_{k-1}.len + j] in qrow; then dt deletion columns, the
 *                   target bases in trow over '-' in qrow.  Insertions before deletions: the order of a CIGAR's I and D
 *                   and of mimeo_path_window_stats;
 *   every block     b_k.len columns of X[b_k.t + j] over Y[b_k.q + j];
 *   letters         A C G T in upper case where the base is one of ACGT, N for every other base (the N plane decides first,
 *                   as for mimeo_path_stats).  The device keeps neither case nor IUPAC codes: a soft-masked 'a' comes out
 *                   'A', and 'R' or 'n' comes out 'N'.
 * An alignment without blocks has zero columns.
 *
 * What a caller may rely on:
 *   - row_first[i + 1] - row_first[i] = (t_end - t_first) + (q_end - q_first) - the sum of len, in 64 bits;
 *   - the bytes of trow that are not '-' are the target slice, those of qrow the slice of the aligned strand;
 *   - the columns where both bytes are equal and neither 'N' nor '-' number exactly `matches` of mimeo_path_stats;
 *   - the bytes depend on nothing but the sequences and the blocks.
 * row_first (n + 1 entries), trow and qrow (row_first[n] bytes each) are allocated by the library and released with
 * mimeo_free.  n == 0 returns MIMEO_OK with row_first holding one zero; where there is no column at all, trow and qrow are
 * NULL.  The rows pass through device buffers in slices of bounded size, so a job of any size runs in the memory that is free
 * next to the genomes; the host arrays hold the whole call, and a caller bounds those by what it asks for in one call.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
int mimeo_path_text(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                    const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                    uint64_t **row_first /* n + 1 */, uint8_t **trow, uint8_t **qrow /* row_first[n] bytes each */);

/*
 * Repeat families: the regions of a self job linked through the alignment paths (kernel K12) — which repeats are copies of
 * each other.  Replaces nothing in the reference, which keeps lastz's coordinates and no alignment.  An alignment row that
 * covers a region of its target scaffold is projected, through its path, onto its query scaffold; a region that the projection
 * covers belongs to the same family.  The join of rows and regions has one item per pair: a family of c copies makes on the
 * order of c * c of them, so the rule runs on the device, with a lock-free union-find over the regions.
 *
 * "Family linking v1".  Inputs:
 *   T, aln, n, path_first, blocks, nblocks   as for mimeo_path_stats; a self job: the query scaffolds are T's
 *   regions[0 .. nreg)       sorted by (chrom, start) and disjoint, none empty — as mimeo_coverage_collapse returns them
 *   chrom_of_scaf[nscaf]     the region chromosome number of scaffold i; NULL: i itself.  It numbers every chromosome once
 *   items[0 .. nitems)       `aln` a record, `group` the number r of a region of that record's TARGET scaffold, [w0, w1) the
 *                            part of the region that the record is asked about (the overlap of the two, as a rule)
 *   min_cover_pct            1 .. 100
 * Per item, with r = [rs, re):
 *   A  the alignment covers the region: 100 * (w1 - w0) >= min_cover_pct * (re - rs).  Otherwise the item links nothing.
 *   B  projection.  Of the columns of the record's blocks, take those whose target base lies in [w0, w1).  None (the window
 *      lies wholly in a deletion, or off the alignment, or the record has no block): the item links nothing.  Otherwise q_lo
 *      is the aligned-strand query coordinate (mimeo_path_block.q) of the first such column and q_hi that of the last one
 *      plus one; on the query's plus strand the projection is P = [q_lo, q_hi) for qstrand 0 and [Lq - q_hi, Lq - q_lo) for
 *      qstrand 1, Lq the query scaffold's length.
 *   C  linking.  For every region s = [ss, se) of scaffold qid with ov = |P n s| > 0: if 100 * ov >= min_cover_pct * (se - ss)
 *      and s != r, then r and s are in one family and links[r] grows by one.  s == r (a tandem array inside one region) is
 *      skipped and not counted.
 * All arithmetic is in 64 bits; there are no floats.
 *
 * Output (caller's arrays of nreg entries): family[i] is the smallest region number in region i's component of the graph of
 * these links (family[i] <= i; a region nobody links is its own family), links[i] the number of (item, s) that linked from
 * region i.  Both depend on nothing but the inputs: not on the order of the items, the grid, or the cut into slices.
 * nitems == 0: family[i] = i, links[i] = 0, MIMEO_OK, nothing else is looked at.
 *
 * Everything is checked before the device sees it; a violation is MIMEO_ERR_ARG with a message that starts with
 * "mimeo_link_regions:" and names the item, the region, or the record and the block: min_cover_pct in 1 .. 100; everything
 * mimeo_path_stats checks; chrom_of_scaf[i] < nscaf and no chromosome twice; the regions sorted, disjoint, start < end, and
 * end inside the scaffold of their chromosome; per item aln < n, group < nreg, the region's chrom == chrom_of_scaf[tid], and
 * rs <= w0 <= w1 <= re.  Records and blocks go to the device in the same bounded slices as for mimeo_path_stats, and only
 * the slices that an item asks for; the union-find stays on the device across them.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
int mimeo_link_regions(const mimeo_genome *T, const mimeo_alignment *aln, uint64_t n, const uint64_t *path_first,
                       const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_interval *regions, uint64_t nreg,
                       const uint32_t *chrom_of_scaf /* NULL: identity */, const mimeo_window_item *items, uint64_t nitems,
                       uint32_t min_cover_pct, uint32_t *family /* caller's, nreg entries */, uint64_t *links /* caller's, nreg entries */);

/*
 * Column pileup of alignment paths and a base called from every column (kernel K13): the producer of a repeat library.  Where
 * mimeo_path_window_stats collapses the columns of every alignment that piles up on a region to eight sums, this keeps the same
 * pile PER COLUMN of the target, and calls a base from each: the consensus of the copies that align to a region, in the
 * region's own coordinates.  Replaces nothing in the reference, which keeps no alignment; the sequences are read from the
 * device-resident genomes, and no base text crosses the ABI on the way in.
 *
 * "Pileup v1".  T, Q, aln, n, path_first, blocks and nblocks are those of mimeo_path_stats.  Window g is [start, end) on the plus
 * strand of target scaffold `tid`; column x of window g is entry col_first[g] + (x - start) of `cols` and of `call`, with
 * col_first the prefix sum of end - start over the windows and ncols its total, in 64 bits.  Windows may overlap or repeat: each
 * has columns of its own.  An item (aln, group, w0, w1) adds record `aln`, clipped to [w0, w1), to window `group`.
 *
 * Counts, per item and target base x in [w0, w1), with b_k, p_k, dt_k and dq_k as for mimeo_path_window_stats:
 *   a c g t n   x lies under block b_k: with y the base of the aligned query strand at b_k.q + (x - b_k.t), the counter of y
 *               grows by one where y is one of ACGT, and n where it is not (the N plane decides first).  The target's own base
 *               plays no part in the counts;
 *   del         x lies in a gap [p_k, b_k.t): del grows by one;
 *   nothing     x lies outside [tstart, tend), or the record has no block;
 *   ins_runs, ins_bases   for dq_k > 0 and w0 <= p_k < w1, column p_k gets ins_runs += 1 and ins_bases += dq_k: the insertion
 *               sits in front of target base p_k and is never split — the rule of mimeo_path_window_stats.
 * What follows, and what a caller may rely on:
 *   - the counts are additive over any partition of an item's window;
 *   - summed over a window's columns, a + c + g + t + n is matches + transitions + transversions + ambiguous of
 *     mimeo_path_window_stats for the same items, del its del_bases, ins_runs and ins_bases its own;
 *   - the counts are exact integers of 32 bits (a call in which more than 2^32 - 1 items name one window is refused) and depend
 *     on nothing but the sequences, the blocks and the items.
 *
 * Call, per column, with x0 the target's own base (its letter A, C, G or T, or N for anything else):
 *   votes      v[b] = count[b] + (x0 == b ? 1 : 0) for b in A, C, G, T, and vd = del: the region's own copy votes once;
 *   winner     the largest vote.  Among equal votes x0 wins if it is one of them, otherwise the order is A, C, G, T; a deletion
 *              wins only when it is strictly larger than every base;
 *   byte       all five votes zero: 'N'; a winning deletion: '-'; otherwise the upper-case letter of the winner.
 * So `call` always has ncols bytes, and a column that nobody covers calls the target's own letter.  A limit of v1: nothing is
 * inserted into the call; insertions are reported through ins_runs / ins_bases, and a consumer decides.
 *
 * Everything is checked before the device sees it; a violation is MIMEO_ERR_ARG with a message that starts with
 * "mimeo_path_pileup:" and names the item, the window, or the record and the block: everything mimeo_path_stats checks; per
 * window tid inside T, start <= end and end <= the scaffold's length; per item aln < n, group < nwin, the record's tid equal to
 * the window's, and start <= w0 <= w1 <= end.  nwin == 0 returns MIMEO_OK at once; nitems == 0 leaves zero counts and the target's
 * own letters.  cols and call may each be NULL.  Records and blocks go to the device in the same bounded slices as for
 * mimeo_path_stats, and only the slices that an item asks for; the columns are worked off in batches of a bounded number, so a
 * call of any ncols runs in the memory that is free next to the genomes.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
typedef struct mimeo_pileup_window {
    uint32_t tid, start, end;
} mimeo_pileup_window;                                         /* 12 bytes */
typedef struct mimeo_pileup_column {
    uint32_t a, c, g, t, n, del, ins_runs, ins_bases;
} mimeo_pileup_column;                                         /* 32 bytes */
int mimeo_path_pileup(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                      const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                      const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items, uint64_t nitems,
                      mimeo_pileup_column *cols /* caller's, ncols entries, or NULL */, uint8_t *call /* caller's, ncols bytes, or NULL */);

/*
 * Insertion columns of a pileup (kernel K14): the bases that mimeo_path_pileup counts in ins_runs / ins_bases and leaves out of
 * its call, piled up column by column and called.  A region's representative copy routinely lacks something that most of its
 * family carries — a private deletion, a truncated segment; the rows of the pile then all insert at one target base, and this
 * call says what they insert.  A consumer splices the called bytes into the call of mimeo_path_pileup.
 *
 * "Pileup v2, insertion columns".  T, Q, aln, n, path_first, blocks, nblocks, windows, nwin, items and nitems are exactly those
 * of mimeo_path_pileup.  Site s is the position IN FRONT OF target base x of window `window`; it has ncols insertion columns, and
 * column j of site s is entry icol_first[s] + j of `icols` and of `icall`, with icol_first the prefix sum of ncols over the sites
 * and nicols its total, in 64 bits.  `voters` is the number of sequences that vote at the site, the region's own copy among them
 * (depth + 1 of the pileup's column x, as a rule); only the call reads it.
 *
 * Counts.  Per item (aln, group, w0, w1) and site s with sites[s].window == group and w0 <= x < w1, where the record has a block
 * b_k, k > 0, with p_k == x and dq_k > 0 (p_k and dq_k as for mimeo_path_window_stats: the end of the block before, and the query
 * bases skipped) — the "never split, belongs to the column that holds p_k" rule of ins_runs:
 *   res[s]      runs += 1, bases += dq_k, max_len = max(max_len, dq_k), and longer += 1 where dq_k > ncols;
 *   icols       for j in [0, min(dq_k, ncols)), with y the base of the aligned query strand at b_{k-1}.q + b_{k-1}.len + j — the
 *               bases, in the order, that mimeo_path_text puts over '-' — column icol_first[s] + j counts y under a / c / g / t,
 *               or under n where y is not one of ACGT (the N plane decides first).  Runs are left-aligned: every run's first
 *               inserted base votes in column 0.
 * A site inside a deletion (p_k < x < b_k.t) gets nothing from that item, and so does a site at the record's first block start, at
 * a block boundary with dq_k == 0, or off the alignment.  Where both sequences jump (dq_k > 0 and dt_k > 0) the run counts at p_k:
 * insertions come before deletions, as everywhere else.
 * What follows, and what a caller may rely on:
 *   - res[s].runs and res[s].bases equal ins_runs and ins_bases of mimeo_path_pileup at column x of that window, for the same items;
 *   - a + c + g + t + n of column j is the number of runs with dq > j: it does not increase with j;
 *   - where longer == 0, the sum of a + c + g + t + n over the site's columns is `bases`;
 *   - the counts are exact integers of 32 bits and depend on nothing but the sequences, the blocks, the items and the sites: not on
 *     the grid, the slices, the cut into jobs or the order of the items.
 *
 * Call, per insertion column:
 *   top     the largest of a, c, g, t; among equal counts the order is A, C, G, T;
 *   total   a + c + g + t + n;
 *   vg      voters > total ? voters - total : 0 — the gap vote: everyone at the site who has no j-th inserted base, the region's
 *           own copy among them;
 *   byte    the winner's upper-case letter where top > vg; otherwise 'N' where top == 0 and n > vg; otherwise '-'.
 * A tie goes to the gap: the representative inserts nothing.  With voters = depth + 1, "2 * ins_runs > depth + 1" — the rule by
 * which a consumer picks its sites — is exactly total > vg in column 0.
 *
 * ncols is 1 .. 1024 (INSERT_MAX_COLS).  That is ample: with the default gap penalties and y-drop a single gap run cannot exceed
 * about (ydrop - gap_open) / gap_extend = 300 bases.  With other parameters a longer run is truncated to the site's columns and
 * counted in `longer` (max_len says how long it was).
 *
 * Everything is checked on the host before anything is uploaded; a violation is MIMEO_ERR_ARG with a message that starts with
 * "mimeo_path_insertions:" and names the site, the item, the window, or the record and the block: everything mimeo_path_pileup
 * checks, in the same order; then per site window < nwin, start <= x < end, 1 <= ncols <= 1024, and the sites strictly increasing
 * by (window, x).  nsites == 0 returns MIMEO_OK at once; nitems == 0 leaves zero counts and '-' bytes.  res, icols and icall may
 * each be NULL.  Records and blocks go to the device in the same bounded slices as for mimeo_path_stats, and only the slices that
 * an item asks for; the insertion columns are worked off in batches of a bounded number.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
typedef struct mimeo_insert_site {
    uint32_t window, x, ncols, voters;
} mimeo_insert_site;                                           /* 16 bytes */
typedef struct mimeo_insert_result {
    uint32_t runs, bases, longer, max_len;
} mimeo_insert_result;                                         /* 16 bytes */
typedef struct mimeo_insert_column {
    uint32_t a, c, g, t, n;
} mimeo_insert_column;                                         /* 20 bytes */
int mimeo_path_insertions(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                          const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                          const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items, uint64_t nitems,
                          const mimeo_insert_site *sites, uint64_t nsites,
                          mimeo_insert_result *res /* caller's, nsites entries, or NULL */,
                          mimeo_insert_column *icols /* caller's, nicols entries, or NULL */, uint8_t *icall /* caller's, nicols bytes, or NULL */);

/*
 * The stacked rows of a pile (kernel K15): the evidence behind a consensus — for every item of a pileup one row of text in the
 * coordinates of its window, with the insertion columns of the window's sites opened up, so that the rows of a window stand
 * under each other as one multiple alignment (a Stockholm seed alignment per family is written from it).  mimeo_path_pileup
 * reduces every column to eight counters and mimeo_path_text renders one pairwise row in that row's own columns; the host
 * holds no sequence text, so the stack is made on the device from the resident genomes.
 *
 * "Pileup v3, the stack".  Everything up to nsites is word for word the argument list of mimeo_path_insertions, and the checks
 * are the same, in the same order; only `voters` of a site is not read.
 *
 * Columns of a window.  Window g is [start, end); its sites are s_0 < ... < s_{m-1} at target bases x_i with n_i = ncols:
 *   W_g           (end - start) + the sum of n_i, in 64 bits;
 *   tcol of x     the column of target base x: (x - start) + the sum of n_i over the sites with x_i <= x;
 *   insertion column j of site i   tcol of x_i - n_i + j: a site's columns sit directly in front of the column of its base.
 *
 * Rows.  Row k belongs to item k, in item order: rows[row_first[k] .. row_first[k + 1]), with row_first the 64-bit prefix sum
 * of W of the item's window.  Each item has a row of its own, also where two items name the same record and window.
 *
 * Bytes of item k = (aln, group, w0, w1), with b_k, p_k, dt_k and dq_k as for mimeo_path_window_stats, lo = max of w0 and the
 * first block's t, hi = min of w1 and the last block's end:
 *   target column x    '.' where x lies outside [lo, hi), the record has no block, or lo >= hi;
 *                      under block b_k: the letter of the aligned query strand at b_k.q + (x - b_k.t), in upper case, 'N' where
 *                      the base is not one of ACGT (the N plane decides first);
 *                      in a gap [p_k, b_k.t): '-';
 *   insertion column j of site i   where w0 <= x_i < w1 and the record has a block b_k, k > 0, with p_k == x_i and j < dq_k: the
 *                      letter of the aligned query strand at b_{k-1}.q + b_{k-1}.len + j in lower case, a c g t, or n — the
 *                      bases, in the order, that mimeo_path_insertions counts; every other insertion column: '.'.
 * An insertion column never holds '-' or an upper-case letter, a target column never a lower-case letter.
 *
 * res[k].  The item's query bases are the bases under its target columns in [w0, w1) and its insertion runs with
 * w0 <= p_k < w1 (the "never split" rule): one contiguous stretch [q_lo, q_hi) of the aligned strand, in the coordinates of
 * mimeo_path_block.q.  `bases` is the number of letters in the row, `hidden` the number of inserted bases of those runs that
 * have no column: there is no site at p_k, or the run is longer than ncols.  bases + hidden == q_hi - q_lo always; all four
 * fields are zero for an item without a query base.
 *
 * What a caller may rely on:
 *   - per target column of a window, the numbers of A C G T N - over the rows of the window's items equal a c g t n del of
 *     mimeo_path_pileup for the same items;
 *   - per insertion column, the numbers of a c g t n equal icols of mimeo_path_insertions;
 *   - the rows whose column 0 of a site holds a letter number res.runs of that site;
 *   - where hidden == 0, the row's letters in order, upper-cased, are the slice [q_lo, q_hi) of the aligned strand as
 *     mimeo_path_text writes it;
 *   - the bytes depend on nothing but the sequences, blocks, windows, items and sites: not on slices, batches, jobs or the grid.
 *
 * Everything is checked on the host before anything is uploaded; a violation is MIMEO_ERR_ARG with a message that starts with
 * "mimeo_path_stack:" and names the site, the item, the window, or the record and the block.  nitems == 0 returns MIMEO_OK with
 * row_first holding one zero and rows NULL (also where no row has a column); nsites == 0 is legal and gives a stack without
 * insertion columns.  res may be NULL.  row_first and rows are allocated by the library and released with mimeo_free.  Records
 * and blocks go to the device in the same bounded slices as for mimeo_path_stats, and only the slices that an item asks for;
 * the rows pass through a device buffer of bounded size (a single row goes in whole), so a call of any size runs in the memory
 * that is free next to the genomes; the host arrays hold the whole call, and a caller bounds those by what it asks for at once.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
typedef struct mimeo_stack_row {
    uint32_t q_lo, q_hi, bases, hidden;
} mimeo_stack_row;                                             /* 16 bytes */
int mimeo_path_stack(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                     const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                     const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items, uint64_t nitems,
                     const mimeo_insert_site *sites, uint64_t nsites,
                     mimeo_stack_row *res /* caller's, nitems entries, or NULL */,
                     uint64_t **row_first /* nitems + 1 */, uint8_t **rows /* row_first[nitems] bytes */);

/*
 * The rows of a pile against the call (kernel K16): how far every copy of a family is from the family's consensus — the number
 * that dates a copy, and, binned and weighted by bases, the repeat landscape of a library.  mimeo_path_window_stats measures a
 * row against the region's own copy, which between two copies is twice the distance to their ancestor and is wrong wherever
 * the representative carries a private indel; mimeo_path_stack could hand the rows over as text, nitems * W bytes for six
 * integers per item.  Here the aligned query strand is compared on the device with a supplied call instead of with the
 * target's own base, inserted columns included.
 *
 * "Pileup v4, rows against the call".  Everything up to nsites is word for word the argument list of mimeo_path_stack, and the
 * checks are the same, in the same order; `voters` of a site is not read.  `call` is indexed as mimeo_path_pileup returns it:
 * column x of window g is call[col_first[g] + (x - start)]; `icall` as mimeo_path_insertions returns it: column j of site s is
 * icall[icol_first[s] + j].  Every byte of both is one of A C G T N -.
 *
 * Item k = (aln, g, w0, w1), with b_k, p_k and dq_k as for mimeo_path_window_stats; as for mimeo_path_stack, lo = max of w0 and
 * the first block's t, hi = min of w1 and the last block's end.  A record without a block, or lo >= hi, gives eight zeros.
 *
 * A pair (c, y) — c from the call, y from the aligned query strand, the N plane deciding first — is classified:
 *   ambiguous       c or y is N;
 *   matches         c == y;
 *   transitions     A <-> G, C <-> T;
 *   transversions   every other pair.
 * Target columns, x in [lo, hi), c = call[col_first[g] + (x - start)]:
 *   under block b_k, c a letter   classify (c, y), y the base at b_k.q + (x - b_k.t);
 *   under a block, c == '-'       ins_bases += 1: the copy holds a base where the consensus has none;
 *   in a gap [p_k, b_k.t), c a letter   del_bases += 1;
 *   in a gap, c == '-'            nothing.
 * Inserted runs, every k > 0 with dq_k > 0 and w0 <= p_k < w1 (the never-split rule), base j < dq_k, y the base at
 * b_{k-1}.q + b_{k-1}.len + j:
 *   a site s = (g, p_k) exists, j < ncols, and icall[icol_first[s] + j] is a letter   classify;
 *   every other case              ins_bases += 1: no site, a run beyond ncols, or '-' in the consensus.
 * Spanned sites, every site s of window g with w0 <= x_s < w1 and first block's t < x_s < last block's end:
 *   every column j whose icall byte is a letter and for which the item has no j-th inserted base there   del_bases += 1.  It
 *   has none where no block has p_k == x_s, where dq_k == 0, or where j >= dq_k; a site inside a deletion is included.
 * q_lo and q_hi are the stretch of mimeo_stack_row: the item's bases under its target columns and in its runs.
 *
 * What a caller may rely on:
 *   - matches + transitions + transversions + ambiguous + ins_bases == q_hi - q_lo;
 *   - q_lo and q_hi are those of mimeo_path_stack for the same inputs;
 *   - with `call` the target's own letters (mimeo_path_pileup without items) and nsites == 0, the first six fields of item k
 *     equal matches, transitions, transversions, ambiguous, ins_bases, del_bases of mimeo_path_window_stats for that item alone
 *     in a group, wherever the target's letter is not N; where it is N both count the column ambiguous;
 *   - over a window's items, for every letter column of the call the classified letters number a + c + g + t + n of
 *     mimeo_path_pileup at that column, and likewise those of mimeo_path_insertions at a site's letter columns;
 *   - the counts are exact integers and depend on nothing but the sequences, blocks, windows, items, sites and the two calls:
 *     not on slices, jobs, launches or the grid.
 *
 * Everything is checked on the host before anything is uploaded; a violation is MIMEO_ERR_ARG with a message that starts with
 * "mimeo_path_call_stats:" and names the site, the item, the window, the record and the block, or — checked last — the column
 * of `call` or the insertion column of `icall` whose byte is not one of the six.  call is NULL only where the windows have no
 * column, icall iff nicols == 0.  nitems == 0 returns MIMEO_OK at once behind the checks; nsites == 0 is legal.  Records and
 * blocks go to the device in the same bounded slices as for mimeo_path_stats, and only the slices that an item asks for; the
 * two calls are packed into bit planes on the device once per call, 1.5 bytes of device memory per column while it runs.
 *
 * A new symbol beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs it checks for the symbol.
 */
typedef struct mimeo_call_stats {
    uint32_t matches, transitions, transversions, ambiguous;
    uint32_t ins_bases, del_bases, q_lo, q_hi;
} mimeo_call_stats;                                            /* 32 bytes */
int mimeo_path_call_stats(const mimeo_genome *T, const mimeo_genome *Q /* NULL: T */, const mimeo_alignment *aln, uint64_t n,
                          const uint64_t *path_first, const mimeo_path_block *blocks, uint64_t nblocks,
                          const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items, uint64_t nitems,
                          const mimeo_insert_site *sites, uint64_t nsites,
                          const uint8_t *call /* ncols bytes */, const uint8_t *icall /* nicols bytes, NULL iff nicols == 0 */,
                          mimeo_call_stats *out /* caller's, nitems entries */);

/*
 * Terminal repeats of features (kernel K17): what kind of element a region is, read off its own two ends.  Two direct repeats
 * at the ends are the LTRs of a retrotransposon, and their divergence dates that one insertion; two inverted repeats are the
 * TIRs of a DNA transposon.  The seeded pipeline cannot see either (a TIR is 10 - 50 bases; a 12of19 seed and hspthresh 3000
 * need about 33 clean ones), so this is a dense, exhaustive DP: for every item the first w bases against the last w bases,
 * and against the reverse complement of the last w bases.  The result is the library's own currency — records and gap-free
 * blocks as mimeo_align_units_paths returns them — so mimeo_path_stats, mimeo_path_text and the writers of CIGARs serve it.
 *
 * Item k = [start, end) on scaffold `chrom` of G, of length len; fwd and rc are the scaffold's forward strand and its stored
 * reverse complement.
 *   window     w = min(window, (end - start) / 2), integer division: the two windows never overlap
 *   head       a[i] = fwd[start + i], 0 <= i < w
 *   direct     out[2k], qstrand 0:      b[j] = fwd[end - w + j]
 *   inverted   out[2k + 1], qstrand 1:  b[j] = rc[len - end + j] — the stored reverse complement; nothing is flipped, as in
 *              the coordinates of mimeo_path_block
 *   column     s(x, y) = +match where both bases are ACGT and equal, else -mismatch (the N plane decides first)
 * A Gotoh local alignment over the cells (i, j), 0 <= i, j < w, with H = 0 (and no E, no F) outside:
 *   E[i][j] = max(H[i][j-1] - gap_open - gap_extend, E[i][j-1] - gap_extend)    consumes b[j]: q jumps, an insertion
 *   F[i][j] = max(H[i-1][j] - gap_open - gap_extend, F[i-1][j] - gap_extend)    consumes a[i]: t jumps, a deletion
 *   H[i][j] = max(0, H[i-1][j-1] + s(a[i], b[j]), E[i][j], F[i][j])
 * The best cell is the largest H; of equal cells the smallest i, then the smallest j.  Below min_score nothing is found.
 * The traceback from the best cell decides every tie:
 *   in H with value v > 0   the diagonal if v == H[i-1][j-1] + s; else to E if v == E[i][j]; else to F;
 *   in E                    the gap was opened here — back to H at (i, j-1) — if E[i][j] == H[i][j-1] - gap_open - gap_extend,
 *                           else it extends: E at (i, j-1);
 *   in F                    the same with i - 1;
 *   it stops where the H value reached is 0.
 * The diagonal steps merge into blocks with t = start + i on the plus strand and q on the strand that was aligned: end - w + j
 * (direct) or len - end + j (inverted); the path keeps the contract of mimeo_path_block.  The record: tid = qid = chrom;
 * tstart / tend from the first and the last block; qstart / qend on the plus strand (qstrand 1: by the formula above); score
 * the best H; id_d the sum of the blocks' len; id_n the matching columns — so what mimeo_path_stats promises for paths of
 * mimeo_align_units_paths holds here too.  Nothing found (also w == 0): the record is zero except tid, qid and qstrand, and
 * its path is empty; mimeo_path_stats accepts it and counts nothing.
 *
 * `out` is the caller's, 2 n records; *path_first (2 n + 1 entries), *blocks and *nblocks are the library's, released with
 * mimeo_free (*blocks is NULL where there is no block).  Everything is checked before the device sees it: a window outside
 * 1 .. 4096 is MIMEO_ERR_LIMIT; every other parameter out of range, a reserved field that is not 0, a chrom outside the
 * genome or an item that is not start <= end <= len is MIMEO_ERR_ARG, with a message that starts with
 * "mimeo_terminal_repeats:" and names the item.  n == 0 returns MIMEO_OK at once (path_first holds one zero).  The results
 * are exact integers and depend on nothing but the sequence, the items and the parameters: not on how the jobs are cut into
 * launches (the traceback of a job takes about w * w / 2 bytes of device memory while it runs, and a call takes a bounded
 * share of what is free).
 *
 * Two new symbols beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs them checks for the symbols.
 */
typedef struct mimeo_terminal_params {
    int32_t window;      /* bases of each end that are examined [1024]; 1 .. 4096, MIMEO_ERR_LIMIT outside   */
    int32_t match;       /* [2]  1 .. 1000                                                                  */
    int32_t mismatch;    /* [3]  penalty, 1 .. 1000; also every column with a non-ACGT base                  */
    int32_t gap_open;    /* [5]  0 .. 1000; a gap of k bases costs gap_open + k * gap_extend (as lastz's)    */
    int32_t gap_extend;  /* [2]  1 .. 1000                                                                  */
    int32_t min_score;   /* [40] >= 1: an orientation whose best score is below it reports nothing          */
    int32_t reserved[2]; /* must be 0 */
} mimeo_terminal_params;
int mimeo_terminal_params_default(mimeo_terminal_params *p);
int mimeo_terminal_repeats(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n,
                           const mimeo_terminal_params *p,
                           mimeo_alignment *out /* caller's, 2 n entries */,
                           uint64_t **path_first /* 2 n + 1 */, mimeo_path_block **blocks, uint64_t *nblocks);

/*
 * Flank repeats (kernel K18): the target-site duplication of an element.  An insertion duplicates 2 - 20 bases of the host;
 * the two copies lie immediately outside the element's two ends, in direct orientation.  Finding them is the evidence that
 * a pair of terminal repeats (mimeo_terminal_repeats) is an insertion, and it fixes the element's first and last base, which a
 * local alignment with a score cut-off cannot.
 *
 * Item [start, end) on scaffold `chrom` of G, of length L; fwd is the scaffold's forward strand.
 *   candidates   every dl, dr in [-slack, slack] and every k in [min_len, max_len]
 *   copies       p = start + dl - k is the start of the left copy, r = end + dr the start of the right copy
 *   admissible   p >= 0, r + k <= L and start + dl <= end + dr;
 *                m <= max_mismatch, with m the number of columns c in [0, k) where fwd[p + c] and fwd[r + c] are not two
 *                equal ACGT bases;
 *                columns 0 and k - 1 match;
 *                v = k - 3 m >= min_len
 *   choice       the admissible candidate with the largest v; of equal ones the smallest |dl| + |dr|, then the smallest m,
 *                then the smallest dl, then the smallest dr
 * The record: left_start = p, right_start = r, len = k, mismatches = m, dl, dr; the element is [start + dl, end + dr).  No
 * admissible candidate: the record is all zero (len == 0 tells).
 *
 * `out` is the caller's, n records.  Everything is checked before the device sees it, and reported as MIMEO_ERR_ARG with a
 * message that starts with "mimeo_flank_repeats:" and names the item: a chrom outside the genome, an item that is not
 * start <= end <= L, a parameter out of range, a reserved field that is not 0.  n == 0 returns MIMEO_OK at once.  The
 * results are exact and do not depend on how the items are batched.
 *
 * Chance (derived, not measured): with max_mismatch 0 a candidate (dl, dr) holds a duplication of at least min_len bases
 * with probability 4^-min_len, and the maximal runs of a diagonal add the factor 1 + 1/4 + ... = 4/3, so a random site has
 * at most (2 slack + 1)^2 * 4^-min_len * 4/3 admissible candidates: 0.13 at the defaults (in a restatement 0.073 of 2000 random
 * sites had one: candidates that share a diagonal come together).  A 4-base duplication is weak evidence, a 6-base one strong.
 *
 * mimeo_open_frames (kernel K19): the longest stop-free stretch of each of the six reading frames of an item.
 * Item [start, end) has m = end - start bases on a scaffold of length L.
 *   strands   sigma = 0: s[i] = fwd[start + i]; sigma = 1: s[i] = rc[L - end + i] — a window of the stored reverse complement;
 *             nothing is flipped, as in mimeo_terminal_repeats
 *   codons    in frame phi in {0, 1, 2} codon t is s[phi + 3t .. phi + 3t + 2], 0 <= t < T = max(0, (m - phi) / 3), integer
 *             division.  A codon is closed when it is TAA, TAG or TGA, or when any of its bases is not ACGT (an N run is no
 *             open frame); otherwise it is open
 *   record    out[6k + 3 sigma + phi]: the longest maximal run [t0, t1) of open codons, the earliest t0 among runs of equal
 *             length.  codons = t1 - t0; [start, end) on the plus strand is [start + phi + 3 t0, start + phi + 3 t1) for
 *             sigma = 0 and [end - phi - 3 t1, end - phi - 3 t0) for sigma = 1; met is the index within the run of its first
 *             ATG codon, and equals codons when the run has none.  A frame with no open codon has an all-zero record.
 * The checks and the message convention are those of mimeo_flank_repeats, with the prefix "mimeo_open_frames:"; flags that are
 * not 0 are MIMEO_ERR_ARG.  The results are exact and do not depend on how an item is cut into chunks.
 *
 * Three new symbols beside the old ones: MIMEO_ABI_VERSION stays 3; a host that needs them checks for the symbols.
 */
typedef struct mimeo_flank_params {
    int32_t min_len;       /* [4]  2 .. 32: shortest duplication reported (after the mismatch charge, above) */
    int32_t max_len;       /* [20] min_len .. 32                                                            */
    int32_t slack;         /* [2]  0 .. 8: how far either element boundary may move                          */
    int32_t max_mismatch;  /* [0]  0 .. 2                                                                   */
    int32_t reserved[4];   /* must be 0 */
} mimeo_flank_params;
typedef struct mimeo_flank_repeat {   /* 16 bytes */
    uint32_t left_start, right_start; /* the two copies [left_start, left_start+len), [right_start, right_start+len), plus strand */
    uint16_t len, mismatches;
    int8_t   dl, dr;                  /* the element is [start + dl, end + dr) */
    uint16_t reserved;
} mimeo_flank_repeat;
int mimeo_flank_params_default(mimeo_flank_params *p);
int mimeo_flank_repeats(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n,
                        const mimeo_flank_params *p, mimeo_flank_repeat *out /* caller's, n */);
typedef struct mimeo_open_frame { uint32_t start, end, codons, met; } mimeo_open_frame;   /* 16 bytes */
int mimeo_open_frames(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, uint32_t flags /* must be 0 */,
                      mimeo_open_frame *out /* caller's, 6 n: out[6k + 3 sigma + phi] */);

/*
 * Pairs of the last mimeo_align_pairs / mimeo_align_units call that hit a documented limit and were left
 * out: *n of them; the first min(*n, cap) are written to pair_index[] (index into the call's pair list)
 * and code[] (MIMEO_ERR_LIMIT).  Either array may be NULL.  A left-out pair is a scaffold pair: EVERY entry of the
 * list that names it is reported, once each, in no particular order — also a duplicate and an entry that asked for
 * the other strand only (mimeo_align_units).  mimeo_last_error() describes one of the groups that hit the limit,
 * with its strand ('+' or '-').
 */
int mimeo_get_failed_pairs(uint64_t *pair_index, int32_t *code, uint64_t cap, uint64_t *n);

/*
 * bedtools genomecov -bg | awk $4>=min_cov | sort | bedtools merge | awk len>=min_len
 * (A13+A14; wrappers.py:1131-1177) as one integer kernel pipeline (K7).  Intervals
 * with start >= end are ignored, ends are clipped to chrom_len[chrom].  Output is
 * sorted by (chrom, start).
 */
int mimeo_coverage_collapse(const mimeo_interval *iv, uint64_t n, const uint32_t *chrom_len,
                            uint32_t nchrom, uint32_t min_cov, uint32_t min_len,
                            mimeo_interval **out, uint64_t *nout);

/*
 * bedtools genomecov -bg alone (wrappers.py:1131-1145): the maximal runs of equal depth > 0 of the intervals, in
 * (chrom, start) order — what `bedtools genomecov -bg -i sorted.bed -g lens` prints, as records.  Serves
 * scripts/bedtools, the drop-in for the reference's --bedtools option; the library's own workflows
 * use mimeo_coverage_collapse, which never materialises the runs.
 */
typedef struct mimeo_depth_run {
    uint32_t chrom, start, end, depth;
} mimeo_depth_run;
int mimeo_coverage_bedgraph(const mimeo_interval *iv, uint64_t n, const uint32_t *chrom_len, uint32_t nchrom,
                            mimeo_depth_run **out, uint64_t *nout);

/*
 * Tandem-repeat content of genome slices: the role of `trf F 2 7 7 80 10 50 50 -m -h -ngs` in
 * wrappers.py:120-262 trfFilter (flags run_map.py:145-178).  masked[k] = number of bases of
 * iv[k] = [start, end) on scaffold `chrom` of A that the tandem scorer (K8, DESIGN.md "Tandem
 * scorer v2") marks; the host keeps a hit if 100*masked/len < maxtandem (wrappers.py:237-240).
 * match / mismatch / delta / minscore / maxperiod are TRF's weights and thresholds of the same
 * names (delta = indel penalty; delta <= 0: gap-free comparison); TRF's detection statistics PM and
 * PI have no counterpart.  `masked` is a caller-owned array of n entries.  maxperiod: 1 .. 2000
 * (TRF's own range for the argument; parity with TRF itself unpinned), MIMEO_ERR_LIMIT outside it.
 */
int mimeo_tandem_masked(const mimeo_genome *A, const mimeo_interval *iv, uint64_t n, int32_t match,
                        int32_t mismatch, int32_t delta, int32_t minscore, int32_t maxperiod, uint32_t *masked);

/*
 * The same call with the positions: besides masked[k], the bit masks the device holds for the slices, the very words
 * the counts are summed from (one device call serves both entry points).  Slice k, clipped to its scaffold, has
 * len_k = min(end, scaffold length) - start bases (0 if start is not below that: an empty or inverted slice) and owns
 * (len_k + 31) / 32 consecutive words, the slices following one another in the order of iv; bit i % 32 of a slice's
 * word i / 32 is set when base start + i is marked, and the bits from len_k on in its last word are zero.  *words is
 * allocated by the library (free with mimeo_free; never null on success, also for *nwords = 0), *nwords is their total.
 * Everything else is as for mimeo_tandem_masked.
 */
int mimeo_tandem_mask(const mimeo_genome *A, const mimeo_interval *iv, uint64_t n, int32_t match, int32_t mismatch,
                      int32_t delta, int32_t minscore, int32_t maxperiod, uint32_t *masked, uint32_t **words,
                      uint64_t *nwords);

#ifdef __cplusplus
}
#endif
#endif /* MIMEO_HIP_H */
