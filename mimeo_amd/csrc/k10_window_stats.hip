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
// bases of a long one), four per workgroup, on K9's skeleton.  The wavefront first finds, by a wave-uniform binary search of
// the alignment's blocks, the first block that ends behind w0: a window deep inside a path of hundreds of blocks does not walk
// the blocks in front of it.  From there 64 blocks per pass: lane i loads block i and the end of the block before it, counts
// the gap in front of its block, clips the block to the window, and the clipped blocks go through K9's flattening — an
// inclusive wave scan of the chunk counts, the lanes striding over the (block, 64-column chunk) items, each finding its block
// by a binary search of the scanned counts with lane shuffles.  The first block whose p_k is not below w1 ends the loop for
// the whole wavefront.  Counters are per lane, 32 bits (a job holds fewer than 2^32 target bases and one insertion run per
// block, all inside one query scaffold), reduced once at the end; lane 0 adds the non-zero fields to the group's 64-bit
// counters with integer atomics.  Integers only: exact, and independent of the grid, the slices, the cut into jobs and the
// order of the items.  Coordinates are those of mimeo_path_block; nothing is flipped.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "device_util.h"
#include "window_stats_host.h"

namespace mimeo {

using window_stats_host::Job;

__global__ __launch_bounds__(256) void k10_window_stats(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                        const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                        const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                        const Job *__restrict__ jobs, uint32_t njobs, unsigned long long *__restrict__ out) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);   // wave-uniform
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const uint32_t lane = threadIdx.x & 63u;
    const mimeo_alignment a = aln[job.aln];
    // the strand views come out of a device table: into global address space once per wavefront (device_util.h)
    const GStrandView T(t_fwd[a.tid]), Q((a.qstrand ? q_rc : q_fwd)[a.qid]);
    const uint64_t b0 = first[job.aln] - first[0], b1 = first[job.aln + 1] - first[0];   // the slice's blocks start at first[0]
    const uint32_t w0 = job.w0, w1 = job.w1;
    // the first block that ends behind w0.  The host clipped the window to the alignment: w0 lies in front of the last block's
    // end, so there is one, and b1 > b0.  Every lane takes the same steps (the addresses are wave-uniform).
    uint64_t ks = b0, ke = b1 - 1;
    while (ks < ke) {
        const uint64_t mid = (ks + ke) >> 1;
        const mimeo_path_block b = blocks[mid];
        if (b.t + b.len > w0) ke = mid; else ks = mid + 1;   // t + len <= the scaffold's length: no wrap in 32 bits
    }
    uint32_t n_match = 0, n_ts = 0, n_tv = 0, n_amb = 0, ins_runs = 0, ins_bases = 0, del_runs = 0, del_bases = 0;
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
                if (g1 > g0) del_bases += g1 - g0;
                if (pend >= w0) {
                    if (b.t > pend) del_runs++;
                    if (dq) { ins_runs++; ins_bases += dq; }
                }
                const uint32_t s = max(b.t, w0), e = min(b.t + b.len, w1);
                if (e > s) { ct = s; cq = b.q + (s - b.t); clen = e - s; }
            }
        }
        const bool last = __ballot(!part) != 0ull;   // wave-uniform: the lanes behind the last block do not take part
        const uint32_t chunks = (clen >> 6) + ((clen & 63u) ? 1u : 0u);
        uint32_t incl = chunks;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= (uint32_t)d) incl += v;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63), excl = incl - chunks;
        for (uint32_t base = 0; base < total; base += 64) {   // wave-uniform trip count: every lane takes part in the shuffles
            const bool active = base + lane < total;
            const uint32_t item = active ? base + lane : total - 1u;
            // block of the item = number of lanes whose inclusive count is <= item (at most 63: item < total = incl of lane 63)
            uint32_t j = 0;
#pragma unroll
            for (uint32_t s = 32; s > 0; s >>= 1)
                if ((uint32_t)__shfl((int)incl, (int)(j + s - 1u)) <= item) j += s;
            const uint32_t jt = (uint32_t)__shfl((int)ct, (int)j), jq = (uint32_t)__shfl((int)cq, (int)j);
            const uint32_t jlen = (uint32_t)__shfl((int)clen, (int)j), jex = (uint32_t)__shfl((int)excl, (int)j);
            if (active) {
                const uint32_t off = (item - jex) << 6, rem = jlen - off;   // rem >= 1: the chunk starts inside its clipped block
                const uint64_t mask = rem >= 64u ? ~0ull : (1ull << rem) - 1ull;
                // bounds: a chunk starts at the clipped start, a base of its block: below t + len <= Lt (q + len <= Lq; checked on the
                // host before anything is launched), and win64 reads the three words from that base's word on: at most two words
                // behind the strand's last, inside the PLANE_PAD = 8 zero words that follow it — as in K9.  A chunk starts at any
                // alignment mod 64 on either sequence: win64 shifts both into place.
                const Win64 wt = win64(T, (int32_t)(jt + off)), wq = win64(Q, (int32_t)(jq + off));
                const uint64_t amb = (wt.nm | wq.nm) & mask, ok = mask & ~amb;
                const uint64_t dl = wt.lo ^ wq.lo, dh = wt.hi ^ wq.hi;
                n_amb += (uint32_t)__popcll(amb);
                n_tv += (uint32_t)__popcll(ok & dl);
                n_ts += (uint32_t)__popcll(ok & ~dl & dh);
                n_match += (uint32_t)__popcll(ok & ~dl & ~dh);
            }
        }
        if (last) break;
    }
    uint32_t c[8] = {n_match, n_ts, n_tv, n_amb, ins_runs, ins_bases, del_runs, del_bases};   // the order of mimeo_window_stats
#pragma unroll
    for (int k = 0; k < 8; k++)
        for (int o = 32; o > 0; o >>= 1) c[k] += (uint32_t)__shfl_xor((int)c[k], o);
    if (lane == 0) {   // the group buffer was zeroed on the stream before the first launch of the call
        unsigned long long *dst = out + (uint64_t)job.group * 8u;
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
static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    return end && *end == 0 ? (uint64_t)v : dflt;
}

int window_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                        const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_window_item *items, uint64_t nitems, uint64_t ngroups,
                        mimeo_window_stats *out) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad item reaches the kernel
    std::vector<uint64_t> len_t(T->scaf.size()), len_q(Q->scaf.size());
    for (size_t i = 0; i < len_t.size(); i++) len_t[i] = T->scaf[i].len;
    for (size_t i = 0; i < len_q.size(); i++) len_q[i] = Q->scaf[i].len;
    std::string msg;
    if (!window_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, items, nitems, ngroups, &msg)) { set_error(msg); return MIMEO_ERR_ARG; }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_WINDOW_STATS_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t split_bases = env_u64("MIMEO_WINDOW_STATS_SPLIT_BASES", 1ull << 20);
    const uint64_t launch_jobs = 1ull << 22;   // jobs per launch: 64 MiB of jobs, 2^20 workgroups
    const bool stats = getenv("MIMEO_WINDOW_STATS_STATS") != nullptr;
    hipStream_t st = stream();
    std::vector<StrandView> vt(len_t.size()), vqf(len_q.size()), vqr(len_q.size());
    for (size_t i = 0; i < vt.size(); i++) vt[i] = T->scaf[i].fwd.view(false);
    for (size_t i = 0; i < vqf.size(); i++) { vqf[i] = Q->scaf[i].fwd.view(false); vqr[i] = Q->scaf[i].rc.view(false); }
    DeviceBuf dvt, dvqf, dvqr, da, df, db, dj, dout;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int r) {
        for (DeviceBuf *b : {&dvt, &dvqf, &dvqr, &da, &df, &db, &dj, &dout}) b->release();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        return r;
    };
#define K10_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return done(hip_fail(e__, #call, __FILE__, __LINE__)); } while (0)
    int rc;
    if ((rc = dvt.reserve(vt.size() * sizeof(StrandView) + 16)) || (rc = dvqf.reserve(vqf.size() * sizeof(StrandView) + 16)) ||
        (rc = dvqr.reserve(vqr.size() * sizeof(StrandView) + 16)) || (rc = dout.reserve(ngroups * sizeof(mimeo_window_stats))))
        return done(rc);
    K10_TRY(hipMemcpyAsync(dvt.p, vt.data(), vt.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    K10_TRY(hipMemcpyAsync(dvqf.p, vqf.data(), vqf.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    K10_TRY(hipMemcpyAsync(dvqr.p, vqr.data(), vqr.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    K10_TRY(hipMemsetAsync(dout.p, 0, ngroups * sizeof(mimeo_window_stats), st));   // once per call: every job adds to it
    if (stats) { K10_TRY(hipEventCreate(&ev[0])); K10_TRY(hipEventCreate(&ev[1])); }
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    std::vector<uint64_t> order, start;
    window_stats_host::bucket_items(slices, items, nitems, order, start);
    std::vector<Job> jobs;
    uint64_t njobs_all = 0, slices_used = 0;
    double ms_kernel = 0;
    for (size_t si = 0; si < slices.size(); si++) {
        if (start[si] == start[si + 1]) continue;   // no item asks for this slice: nothing of it is uploaded
        const uint64_t a0 = slices[si].first, na = slices[si].second - a0, k0 = first[a0], nb = first[slices[si].second] - k0;
        window_stats_host::plan_jobs(first, blocks, a0, items, order.data(), start[si], start[si + 1], split_bases, jobs);
        if (jobs.empty()) continue;
        slices_used++;
        if ((rc = da.reserve(na * sizeof(mimeo_alignment))) || (rc = df.reserve((na + 1) * 8)) || (rc = db.reserve(nb * sizeof(mimeo_path_block) + 16)) ||
            (rc = dj.reserve(std::min<uint64_t>(jobs.size(), launch_jobs) * sizeof(Job))))
            return done(rc);
        // the stream orders a slice's copies behind the launch that read the slice before
        K10_TRY(hipMemcpyAsync(da.p, aln + a0, na * sizeof(mimeo_alignment), hipMemcpyHostToDevice, st));
        K10_TRY(hipMemcpyAsync(df.p, first + a0, (na + 1) * 8, hipMemcpyHostToDevice, st));
        K10_TRY(hipMemcpyAsync(db.p, blocks + k0, nb * sizeof(mimeo_path_block), hipMemcpyHostToDevice, st));   // nb >= 1: a job's alignment has blocks
        for (uint64_t j0 = 0; j0 < jobs.size(); j0 += launch_jobs) {
            const uint64_t nj = std::min<uint64_t>(launch_jobs, jobs.size() - j0);
            K10_TRY(hipMemcpyAsync(dj.p, jobs.data() + j0, nj * sizeof(Job), hipMemcpyHostToDevice, st));
            if (stats) K10_TRY(hipEventRecord(ev[0], st));
            hipLaunchKernelGGL(k10_window_stats, dim3((uint32_t)((nj + 3) / 4)), dim3(256), 0, st, (const StrandView *)dvt.p,
                               (const StrandView *)dvqf.p, (const StrandView *)dvqr.p, (const mimeo_alignment *)da.p, (const uint64_t *)df.p,
                               (const mimeo_path_block *)db.p, (const Job *)dj.p, (uint32_t)nj, (unsigned long long *)dout.p);
            K10_TRY(hipGetLastError());
            if (stats) {
                K10_TRY(hipEventRecord(ev[1], st));
                K10_TRY(hipEventSynchronize(ev[1]));
                float ms = 0;
                K10_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
                ms_kernel += ms;
            }
        }
        K10_TRY(hipStreamSynchronize(st));   // `jobs` is rebuilt for the next slice
        njobs_all += jobs.size();
    }
    K10_TRY(hipMemcpyAsync(out, dout.p, ngroups * sizeof(mimeo_window_stats), hipMemcpyDeviceToHost, st));
    K10_TRY(hipStreamSynchronize(st));
#undef K10_TRY
    if (stats)
        fprintf(stderr, "[k10] window stats: %llu items, %llu groups, %llu jobs, slices %llu of %zu, kernels %.3f ms\n", (unsigned long long)nitems,
                (unsigned long long)ngroups, (unsigned long long)njobs_all, (unsigned long long)slices_used, slices.size(), ms_kernel);
    return done(0);
}

}  // namespace mimeo
