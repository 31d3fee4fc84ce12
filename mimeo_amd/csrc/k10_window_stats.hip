// K10 — column statistics of alignment paths clipped to target windows, accumulated into groups (mimeo_path_window_stats,
// include/mimeo_hip.h): what ties a divergence to a REGION — the columns of every alignment that piles up on a repeat whose
// target base lies inside the repeat.  K9 (k9_path_stats.hip) counts whole alignments; an alignment routinely runs past a
// region's ends or across several regions, and the host holds no sequence text to clip with.
//
// The rules (mimeo_hip.h has them in full), for a window [w0, w1) and block b_k with p_k the end of the block before it:
//   columns    those of b_k whose target base lies in [w0, w1); classified as in K9 from the bit planes
//   del_bases  the overlap of [p_k, b_k.t) with the window
//   del_runs, ins_runs, ins_bases   counted where w0 <= p_k < w1: a run belongs to the window that holds its first target
//              base, an insertion sits in front of target base p_k and is never split
// so every field is additive over any partition of a window, which is what lets the host cut a long window into jobs.
//
// Work layout: one wavefront per job (window_stats_host.h: an item clipped to its alignment, or a piece of split_bases target
// bases of a long one), four per workgroup, on the skeleton K9 shares (path_call.h).  The wavefront first finds, by a wave-uniform binary search of
// the alignment's blocks, the first block that ends behind w0: a window deep inside a path of hundreds of blocks does not walk
// the blocks in front of it.  From there 64 blocks per pass: lane i loads block i and the end of the block before it, counts
// the gap in front of its block, clips the block to the window, and the clipped blocks go through K9's flattening
// (path_call.h: scan_chunks, for_each_chunk).  The first block whose p_k is not below w1 ends the loop for
// the whole wavefront.  Counters are per lane, 32 bits (a job holds fewer than 2^32 target bases and one insertion run per
// block, all inside one query scaffold), reduced once at the end; lane 0 adds the non-zero fields to the group's 64-bit
// counters with integer atomics.  Integers only: exact, and independent of the grid, the slices, the cut into jobs and the
// order of the items.  Coordinates are those of mimeo_path_block; nothing is flipped.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "path_call.h"
#include "window_stats_host.h"

namespace mimeo {

using window_stats_host::Job;

__global__ __launch_bounds__(256) void k10_window_stats(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                        const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                        const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                        const Job *__restrict__ jobs, uint32_t njobs, unsigned long long *__restrict__ out) {
    PathJob<Job> J;
    if (!J.load(t_fwd, q_fwd, q_rc, aln, first, jobs, njobs)) return;
    const uint32_t lane = J.lane, w0 = J.job.w0, w1 = J.job.w1;
    const uint64_t b0 = J.b0, b1 = J.b1;
    // the first block that ends behind w0.  The host clipped the window to the alignment: w0 lies in front of the last block's
    // end, so there is one, and b1 > b0.  Every lane takes the same steps (the addresses are wave-uniform).
    const uint64_t ks = first_block_ending_behind(blocks, b0, b1 - 1, w0);
    ColumnCounts n;
    for (uint64_t p = ks;; p += 64) {
        const uint64_t idx = p + lane;
        uint32_t ct = 0, cq = 0, clen = 0;   // the block clipped to the window
        bool part = false;                   // the block takes part: p_k < w1 (the alignment's first block: t < w1)
        if (idx < b1) {
            const mimeo_path_block b = blocks[idx];
            uint32_t pend = b.t, dq = 0;     // the alignment's first block has no gap in front of it
            if (idx > b0) {
                const mimeo_path_block pb = blocks[idx - 1];
                pend = pb.t + pb.len;
                dq = b.q - (pb.q + pb.len);
            }
            part = pend < w1;
            if (part) {
                // the gap in front of this block, [pend, b.t) on the target: also that of the first block found, whose pend
                // is at most w0
                const uint32_t g0 = max(pend, w0), g1 = min(b.t, w1);
                if (g1 > g0) n.del_bases += g1 - g0;
                if (pend >= w0) {
                    if (b.t > pend) n.del_runs++;
                    if (dq) { n.ins_runs++; n.ins_bases += dq; }
                }
                const uint32_t s = max(b.t, w0), e = min(b.t + b.len, w1);
                if (e > s) { ct = s; cq = b.q + (s - b.t); clen = e - s; }
            }
        }
        const bool last = __ballot(!part) != 0ull;   // wave-uniform: the lanes behind the last block do not take part
        const ChunkScan s = scan_chunks(clen, lane);
        for_each_chunk(s, lane, ct, cq, clen, 0u, s.total,
                       [&](uint32_t t, uint32_t q, uint64_t mask) { n.count(win64(J.T, (int32_t)t), win64(J.Q, (int32_t)q), mask); });
        if (last) break;
    }
    uint32_t c[8];   // the order of mimeo_window_stats is that of mimeo_column_stats
    n.wave_sums(c);
    if (lane == 0) {   // the group buffer was zeroed on the stream before the first launch of the call
        unsigned long long *dst = out + (uint64_t)J.job.group * 8u;
#pragma unroll
        for (int k = 0; k < 8; k++) if (c[k]) atomicAdd(dst + k, (unsigned long long)c[k]);
    }
}

static_assert(sizeof(mimeo_window_stats) == 64 && sizeof(mimeo_window_item) == 16 && sizeof(Job) == 16 && sizeof(mimeo_path_block) == 12,
              "layouts the kernel relies on");

// MIMEO_WINDOW_STATS_SLICE_BLOCKS: blocks per slice (default 2^24, as K9; 1: every alignment a slice of its own);
// MIMEO_WINDOW_STATS_SPLIT_BASES: a clipped window of more target bases than this is cut into jobs of this many (default 2^20: K9's
// megabase of one wavefront; 0: never); MIMEO_WINDOW_STATS_STATS: what the call did and the HIP-event time of its kernels, on
// stderr.  Results depend on none of them.
int window_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                        const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_window_item *items, uint64_t nitems, uint64_t ngroups,
                        mimeo_window_stats *out) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad item reaches the kernel
    std::string msg;
    if (!window_stats_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, items, nitems, ngroups, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_WINDOW_STATS_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t split_bases = env_u64("MIMEO_WINDOW_STATS_SPLIT_BASES", 1ull << 20);
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    PathCall pc(getenv("MIMEO_WINDOW_STATS_STATS") != nullptr);
    DeviceBuf &dout = pc.buf();
    int rc;
    if ((rc = pc.views(T, Q)) || (rc = dout.reserve(ngroups * sizeof(mimeo_window_stats)))) return rc;
    HIP_TRY(hipMemsetAsync(dout.p, 0, ngroups * sizeof(mimeo_window_stats), pc.st));   // once per call: every job adds to it
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    std::vector<uint64_t> order, start;
    window_stats_host::bucket_items(slices, items, nitems, order, start);
    uint64_t njobs_all = 0, slices_used = 0;
    for (size_t si = 0; si < slices.size(); si++) {
        if (start[si] == start[si + 1]) continue;   // no item asks for this slice: nothing of it is uploaded
        window_stats_host::plan_jobs(first, blocks, slices[si].first, items, order.data(), start[si], start[si + 1], split_bases, jobs);
        if (jobs.empty()) continue;
        slices_used++;
        if ((rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
        rc = pc.run(jobs, 4, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
            hipLaunchKernelGGL(k10_window_stats, grid, dim3(256), 0, pc.st, pc.t_fwd(), pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), d_jobs, nj,
                               (unsigned long long *)dout.p);
        });
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` is rebuilt for the next slice
        njobs_all += jobs.size();
    }
    HIP_TRY(hipMemcpyAsync(out, dout.p, ngroups * sizeof(mimeo_window_stats), hipMemcpyDeviceToHost, pc.st));
    HIP_TRY(hipStreamSynchronize(pc.st));
    if (pc.stats)
        fprintf(stderr, "[k10] window stats: %llu items, %llu groups, %llu jobs, slices %llu of %zu, kernels %.3f ms\n", (unsigned long long)nitems,
                (unsigned long long)ngroups, (unsigned long long)njobs_all, (unsigned long long)slices_used, slices.size(), pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
