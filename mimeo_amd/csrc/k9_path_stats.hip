// K9 — column statistics of alignment paths (mimeo_path_stats, include/mimeo_hip.h): for every alignment the matches,
// transitions, transversions and ambiguous columns of its gap-free blocks, and the insertion / deletion runs and bases
// between them.  Nothing in the reference does this (it keeps lastz's identity column and no alignment); it is what a
// substitution-divergence estimate (Kimura's two-parameter distance) and the NM / de tags of a PAF row are made of.
//
// The bit planes hold the answer (common.h): with x the target base and y the query base of a column,
//   ambiguous     nm(x) | nm(y)                      — masked first: what lo / hi hold under an N is never looked at
//   transversion  lo(x) ^ lo(y)                      (A0 C1 G2 T3: purines have lo = 0)
//   transition    lo equal, hi(x) ^ hi(y)
//   match         lo equal, hi equal                 == the oracle's x < 4 && x == y: matches == id_n
// so 64 columns are two XORs, a few ANDs and four popcounts over two win64 windows.
//
// Work layout: one wavefront per job (path_stats_host.h: an alignment, or split_chunks chunks of a long one), four per
// workgroup.  A typical alignment has ~35 blocks of a few hundred columns: one block per lane would idle most lanes, so
// the work is flattened (the steps are path_call.h's, shared with K10).  64 blocks at a time: lane i loads block i and its chunk count ceil(len / 64), an inclusive wave
// scan gives the item offsets, and the lanes stride over the (block, 64-column chunk) items of the pass, each finding its
// block by a binary search of the scanned counts with lane shuffles.  Counters are per lane, 32 bits (an alignment has
// fewer than 2^32 columns), reduced once at the end; lane 0 writes the 32-byte result — or adds it with integer atomics
// where the alignment was cut into several jobs.  Integers only: exact, and independent of the grid, the slices, the cut
// into jobs and the order of the items.
// Coordinates are those of mimeo_path_block: t on the target's forward strand, q on the query's forward strand or, for
// qstrand == 1, on its stored reverse-complement strand (Scaffold::rc).  Nothing is flipped here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "path_call.h"

namespace mimeo {

using path_stats_host::Job;

__global__ __launch_bounds__(256) void k9_path_stats(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                     const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                     const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                     const Job *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ out) {
    PathJob<Job> J;
    if (!J.load(t_fwd, q_fwd, q_rc, aln, first, jobs, njobs)) return;
    const Job job = J.job;
    const uint32_t lane = J.lane;
    const uint64_t b0 = J.b0, b1 = J.b1;
    ColumnCounts n;
    uint32_t done = 0;   // chunks of the passes before
    // the job that starts the alignment also counts its gaps: it passes over every block, the others stop behind their chunks
    for (uint64_t p = b0; p < b1 && (done < job.c1 || job.c0 == 0); p += 64) {
        const uint64_t idx = p + lane;
        uint32_t bt = 0, bq = 0, blen = 0;
        if (idx < b1) {
            const mimeo_path_block b = blocks[idx];
            bt = b.t; bq = b.q; blen = b.len;
            if (job.c0 == 0 && idx > b0) {   // the gap in front of this block: an insertion run, a deletion run, or both
                const mimeo_path_block pb = blocks[idx - 1];
                const uint32_t dq = bq - (pb.q + pb.len), dt = bt - (pb.t + pb.len);
                if (dq) { n.ins_runs++; n.ins_bases += dq; }
                if (dt) { n.del_runs++; n.del_bases += dt; }
            }
        }
        const ChunkScan s = scan_chunks(blen, lane);   // 0 chunks for the lanes behind the last block
        // the items of this pass that belong to the job: [lo, hi) of [0, total)
        const uint32_t lo = job.c0 > done ? min(job.c0 - done, s.total) : 0u, hi = job.c1 > done ? min(job.c1 - done, s.total) : 0u;
        for_each_chunk(s, lane, bt, bq, blen, lo, hi,
                       [&](uint32_t t, uint32_t q, uint64_t mask) { n.count(win64(J.T, (int32_t)t), win64(J.Q, (int32_t)q), mask); });
        done += s.total;
    }
    uint32_t c[8];
    n.wave_sums(c);
    if (lane == 0) {
        uint32_t *dst = out + (uint64_t)job.aln * 8u;
        if (job.split) {   // the output was zeroed on the stream before the launch
#pragma unroll
            for (int k = 0; k < 8; k++) if (c[k]) atomicAdd(dst + k, c[k]);
        } else {
            uint4 *d4 = (uint4 *)dst;   // 32-byte records in a hipMalloc'ed buffer: 16-byte aligned
            d4[0] = make_uint4(c[0], c[1], c[2], c[3]);
            d4[1] = make_uint4(c[4], c[5], c[6], c[7]);
        }
    }
}

static_assert(sizeof(mimeo_column_stats) == 32 && sizeof(Job) == 16 && sizeof(mimeo_path_block) == 12, "layouts the kernel relies on");

// MIMEO_PATH_STATS_SLICE_BLOCKS: blocks per slice (default 2^24 = 192 MiB of blocks; 1: every alignment a slice of its own);
// MIMEO_PATH_STATS_SPLIT_CHUNKS: an alignment of more chunks than this is cut into jobs of this many (default 16384 = one
// megabase of columns; 0: never); MIMEO_PATH_STATS_STATS: what the call did and the HIP-event time of its kernels, on stderr.
// Results depend on none of them.
int path_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                      const mimeo_path_block *blocks, uint64_t nblocks, mimeo_column_stats *out) {
    if (!n) return 0;
    // every check on the host, before anything is uploaded: a bad path never reaches the kernel
    std::string msg;
    if (!path_stats_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, &msg)) { set_error(msg); return MIMEO_ERR_ARG; }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_PATH_STATS_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;   // 48 + 8 + 32 + 16 bytes per record: 416 MiB
    const uint64_t split_chunks = env_u64("MIMEO_PATH_STATS_SPLIT_CHUNKS", 16384);
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    PathCall pc(getenv("MIMEO_PATH_STATS_STATS") != nullptr);
    DeviceBuf &dout = pc.buf();
    int rc;
    if ((rc = pc.views(T, Q))) return rc;
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    uint64_t njobs_all = 0, chunks_all = 0;
    for (const auto &s : slices) {
        const uint64_t a0 = s.first, na = s.second - s.first;
        path_stats_host::plan_jobs(first, blocks, a0, s.second, split_chunks, jobs);
        if ((rc = pc.slice(aln, first, blocks, a0, s.second)) || (rc = dout.reserve(na * sizeof(mimeo_column_stats)))) return rc;
        // the jobs of a split alignment add to zero; every other alignment has one job, which stores its whole record
        const bool any_split = std::any_of(jobs.begin(), jobs.end(), [](const Job &j) { return j.split != 0; });
        if (any_split) HIP_TRY(hipMemsetAsync(dout.p, 0, na * sizeof(mimeo_column_stats), pc.st));
        rc = pc.run(jobs, 4, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
            hipLaunchKernelGGL(k9_path_stats, grid, dim3(256), 0, pc.st, pc.t_fwd(), pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), d_jobs, nj,
                               (uint32_t *)dout.p);
        });
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(out + a0, dout.p, na * sizeof(mimeo_column_stats), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));   // the results are here, and `jobs` may be rebuilt for the next slice
        if (pc.stats) {
            njobs_all += jobs.size();
            for (const Job &j : jobs) chunks_all += j.c1 - j.c0;
        }
    }
    if (pc.stats)
        fprintf(stderr, "[k9] path stats: %llu alignments, %llu blocks, %llu chunks, %llu jobs, slices %zu, kernels %.3f ms\n", (unsigned long long)n,
                (unsigned long long)nblocks, (unsigned long long)chunks_all, (unsigned long long)njobs_all, slices.size(), pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
