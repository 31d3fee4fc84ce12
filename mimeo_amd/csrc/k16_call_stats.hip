// K16 — the rows of a pile against the call (mimeo_path_call_stats, include/mimeo_hip.h "pileup v4, rows against the call"): how
// far every copy of a family is from the family's consensus.  K10 (k10_window_stats.hip) compares an alignment's query strand
// with the target's own bases; here the place of the target is taken by a supplied call — the consensus of K13 in the columns of
// the window, with the columns that K14 called at the window's sites — so that a column where the representative is the odd one
// out counts against the representative and not against every copy.
//
// The rules (mimeo_hip.h has them in full), for a job's piece [w0, w1) of an item clipped to its alignment, block b_k and p_k
// the end of the block before it:
//   under a block     call letter: the pair (call, query) is classified as in K9 from the bit planes; call '-': ins_bases
//   in a gap          call letter: del_bases; call '-': nothing
//   a run at p_k      (dq_k > 0, w0 <= p_k < w1) with a site at p_k: base j < min(dq_k, ncols) against icall column j where that
//                     is a letter; every other inserted base: ins_bases
//   a spanned site    every letter column of icall for which the item has no inserted base: del_bases
// Every field is additive over a partition of the item's [lo, hi): a run and a site belong to the piece that holds their base.
//
// k16_pack_call runs once per call and per array: a wavefront reads 64 consecutive bytes, one per lane, and four ballots are the
// four words of 64 columns — lo, hi, nm and gap — written in the layout of a strand (common.h: uint4 per 32 bases, PLANE_PAD zero
// words on either side), so that win64 reads a call at any alignment mod 64 and ColumnCounts::count takes the call's planes in
// the place of the target's; the gap plane, in the place of the seed-validity plane, masks the columns out.
//
// k16_call_stats: one wavefront per job, four per workgroup, on the skeleton of path_call.h — K10's walk: the first block that
// ends behind w0 by binary search, then 64 blocks per pass, lane i with block i and the end of the block before it.  A pass
// flattens three lists of stretches into 64-column chunks for the lanes (scan_chunks, for_each_chunk): the clipped blocks
// (classified against the call), the clipped gaps (popcounts of the complement of the gap plane) and the runs that have a site
// (classified against icall; the lane finds the site at p_k by binary search over the job's sites).  The spanned sites need no
// pass of their own: the host put the letter columns of the job's sites into the job (call_stats_host.h: iletters), and with
// `met` the inserted bases that met a letter, del_bases = gaps + site_letters - met and ins_bases = '-' under blocks + the sum
// of dq_k - met.  One wave reduction at the end; lane 0 adds the non-zero fields to out[item] with 32-bit integer atomics (the
// output is zeroed once on the stream; several jobs may feed one item).  Integers only, no LDS: exact, and independent of the
// grid, the slices, the launches and the cut into jobs.
//
// Bounds of the window reads.  The strands: K11's reason — a chunk starts at a base of its stretch, below t + len <= Lt or
// q + len <= Lq (checked on the host), and win64 reads three words from that base's word on: at most two words behind the
// strand's last, inside the PLANE_PAD = 8 zero words that follow it.  An inserted base lies below the following block's q: K14's
// reason.  The calls: a chunk starts at a column of its window (col + (t - w0) < ncols; the host checked w1 <= the window's end)
// or at a column j < ncols of its site, and the packed planes end, like a strand, with PLANE_PAD zero words.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "call_stats_host.h"
#include "path_call.h"

namespace mimeo {

using call_stats_host::Job;
using call_stats_host::SiteDesc;

// The planes of n call bytes: word w of `pw` (a uint4 {lo, hi, nm, gap}) holds the columns [32 w, 32 w + 32).  The buffer was
// zeroed on the stream; a wavefront writes the two words of its 64 columns, also where n ends inside them (zero bits follow).
__global__ __launch_bounds__(256) void k16_pack_call(const uint8_t *__restrict__ bytes, uint64_t n, uint4 *__restrict__ pw) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint64_t nwaves = (uint64_t)gridDim.x * 4u;
    for (uint64_t w = ((uint64_t)blockIdx.x * 256u + threadIdx.x) >> 6; (w << 6) < n; w += nwaves) {   // wave-uniform
        const uint64_t i = (w << 6) + lane;
        const uint32_t b = i < n ? bytes[i] : (uint32_t)'A';   // A: no bit in any plane
        const uint64_t lo = __ballot(b == 'C' || b == 'T'), hi = __ballot(b == 'G' || b == 'T'), nm = __ballot(b == 'N'), gp = __ballot(b == '-');
        if (lane < 2) {
            const uint32_t s = lane << 5;
            pw[2u * w + lane] = make_uint4((uint32_t)(lo >> s), (uint32_t)(hi >> s), (uint32_t)(nm >> s), (uint32_t)(gp >> s));
        }
    }
}

__global__ __launch_bounds__(256) void k16_call_stats(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                      const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                      const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                      const SiteDesc *__restrict__ sites, const uint4 *__restrict__ cpw, const uint4 *__restrict__ ipw,
                                                      const Job *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ out) {
    PathJob<Job> J;
    if (!J.load(t_fwd, q_fwd, q_rc, aln, first, jobs, njobs)) return;
    const uint32_t lane = J.lane, w0 = J.job.w0, w1 = J.job.w1, site0 = J.job.site0, site1 = J.job.site1;
    const uint64_t b0 = J.b0, b1 = J.b1;
    // the two calls as strands that begin at the word of the job's first column: a job has fewer than 2^31 columns of either
    const GStrandView CV(StrandView{cpw + (J.job.col >> 5), nullptr, nullptr, 0u, 0u}), IV(StrandView{ipw + (J.job.icol0 >> 5), nullptr, nullptr, 0u, 0u});
    const uint32_t cb = (uint32_t)(J.job.col & 31u), ib = (uint32_t)(J.job.icol0 & 31u);   // column of base w0; column 0 of site0
    // the first block that ends behind w0.  The host clipped the piece to the alignment: w0 lies in front of the last block's
    // end, so there is one, and b1 > b0.  Every lane takes the same steps (the addresses are wave-uniform).
    const uint64_t ks = first_block_ending_behind(blocks, b0, b1 - 1, w0);
    ColumnCounts n;
    uint32_t met = 0;   // inserted bases that met a letter of icall
    for (uint64_t p = ks;; p += 64) {
        const uint64_t idx = p + lane;
        uint32_t ct = 0, cq = 0, clen = 0;   // the block clipped to the piece
        uint32_t gt = 0, glen = 0;           // the gap in front of it, clipped
        uint32_t ri = 0, rq = 0, rlen = 0;   // the run in front of it where it has a site: its column 0 in IV, its first base, min(dq, ncols)
        bool part = false;                   // the block takes part: p_k < w1 (the alignment's first block: t < w1)
        if (idx < b1) {
            const mimeo_path_block b = blocks[idx];
            uint32_t pend = b.t, pq = 0, dq = 0;   // the alignment's first block has no gap in front of it
            if (idx > b0) {
                const mimeo_path_block pb = blocks[idx - 1];
                pend = pb.t + pb.len;
                pq = pb.q + pb.len;
                dq = b.q - pq;
            }
            part = pend < w1;
            if (part) {
                const uint32_t g0 = max(pend, w0), g1 = min(b.t, w1);
                if (g1 > g0) { gt = g0; glen = g1 - g0; }
                if (pend >= w0 && dq) {
                    n.ins_bases += dq;
                    uint32_t sl = site0, sh = site1;   // the first site of the job that is not in front of p_k
                    while (sl < sh) {
                        const uint32_t mid = sl + ((sh - sl) >> 1);
                        if (sites[mid].x < pend) sl = mid + 1; else sh = mid;
                    }
                    if (sl < site1) {
                        const SiteDesc s = sites[sl];
                        if (s.x == pend) { ri = ib + (uint32_t)(s.icol - J.job.icol0); rq = pq; rlen = min(dq, s.ncols); }
                    }
                }
                const uint32_t s = max(b.t, w0), e = min(b.t + b.len, w1);
                if (e > s) { ct = s; cq = b.q + (s - b.t); clen = e - s; }
            }
        }
        const bool last = __ballot(!part) != 0ull;   // wave-uniform: the lanes behind the last block do not take part
        const ChunkScan s = scan_chunks(clen, lane);
        for_each_chunk(s, lane, ct, cq, clen, 0u, s.total, [&](uint32_t t, uint32_t q, uint64_t mask) {
            const Win64 c = win64(CV, (int32_t)(cb + (t - w0)));
            n.ins_bases += (uint32_t)__popcll(mask & c.sv);   // a base where the call has none
            n.count(c, win64(J.Q, (int32_t)q), mask & ~c.sv);
        });
        if (__ballot(glen != 0u)) {
            const ChunkScan g = scan_chunks(glen, lane);
            for_each_chunk(g, lane, gt, 0u, glen, 0u, g.total, [&](uint32_t t, uint32_t, uint64_t mask) {
                n.del_bases += (uint32_t)__popcll(mask & ~win64(CV, (int32_t)(cb + (t - w0))).sv);
            });
        }
        if (__ballot(rlen != 0u)) {
            const ChunkScan r = scan_chunks(rlen, lane);
            for_each_chunk(r, lane, ri, rq, rlen, 0u, r.total, [&](uint32_t i, uint32_t q, uint64_t mask) {
                const Win64 c = win64(IV, (int32_t)i);
                met += (uint32_t)__popcll(mask & ~c.sv);
                n.count(c, win64(J.Q, (int32_t)q), mask & ~c.sv);
            });
        }
        if (last) break;
    }
    uint32_t c[8];   // the order of mimeo_column_stats
    n.wave_sums(c);
    for (int o = 32; o > 0; o >>= 1) met += (uint32_t)__shfl_xor((int)met, o);
    if (lane == 0) {   // the output was zeroed on the stream before the first launch of the call
        uint32_t *dst = out + (uint64_t)J.job.item * 8u;
        // the order of mimeo_call_stats; met <= the sum of dq_k, and met <= site_letters: the letters under the runs' bases
        const uint32_t v[6] = {c[0], c[1], c[2], c[3], c[5] - met, c[7] + J.job.site_letters - met};
#pragma unroll
        for (int k = 0; k < 6; k++) if (v[k]) atomicAdd(dst + k, v[k]);
    }
}

static_assert(sizeof(mimeo_call_stats) == 32 && sizeof(Job) == 48 && sizeof(SiteDesc) == 16 && sizeof(mimeo_path_block) == 12, "layouts the kernels rely on");

// MIMEO_CALL_STATS_SLICE_BLOCKS: blocks per slice (default 2^24, as K9; 1: every alignment a slice of its own);
// MIMEO_CALL_STATS_JOB_COLUMNS: target columns of a job, at most (default 2^16; 0 or more than 2^20: the default);
// MIMEO_CALL_STATS_STATS: what the call did and the HIP-event time of its kernels, on stderr.  Results depend on none of them.
int path_call_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                           const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                           uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, const uint8_t *call, const uint8_t *icall, mimeo_call_stats *out) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad window, item, site or byte reaches the kernels
    std::string msg;
    if (!call_stats_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, windows, nwin, items, nitems, sites, nsites, &msg) ||
        !call_stats_host::validate_calls(windows, nwin, sites, nsites, call, icall, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    if (!nitems) return 0;
    const call_stats_host::Plan plan = call_stats_host::plan_call(windows, nwin, sites, nsites, icall);
    const uint64_t ncols = plan.ncols(), nicols = plan.nicols();
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_CALL_STATS_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t job_columns = env_u64("MIMEO_CALL_STATS_JOB_COLUMNS", call_stats_host::DEFAULT_JOB_COLUMNS);
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    PathCall pc(getenv("MIMEO_CALL_STATS_STATS") != nullptr);
    DeviceBuf &draw = pc.buf(), &dcpw = pc.buf(), &dipw = pc.buf(), &dsites = pc.buf(), &dout = pc.buf();
    // the planes of `len` columns: whole wavefronts of 64, PLANE_PAD words on either side
    auto plane_bytes = [](uint64_t len) { return (2u * ((len + 63u) >> 6) + 2u * PLANE_PAD) * sizeof(uint4); };
    int rc;
    if ((rc = pc.views(T, Q)) || (rc = draw.reserve(std::max(ncols, nicols) + 16)) || (rc = dcpw.reserve(plane_bytes(ncols))) ||
        (rc = dipw.reserve(plane_bytes(nicols))) || (rc = dsites.reserve(nsites * sizeof(SiteDesc) + 16)) || (rc = dout.reserve(nitems * sizeof(mimeo_call_stats))))
        return rc;
    HIP_TRY(hipMemsetAsync(dout.p, 0, nitems * sizeof(mimeo_call_stats), pc.st));   // once per call: every job adds to it
    if (nsites) HIP_TRY(hipMemcpyAsync(dsites.p, plan.site.data(), nsites * sizeof(SiteDesc), hipMemcpyHostToDevice, pc.st));
    // the two calls to planes, one after the other through one staging buffer: the stream orders the second copy behind the first kernel
    const std::pair<const uint8_t *, uint64_t> arrays[2] = {{call, ncols}, {icall, nicols}};
    DeviceBuf *planes[2] = {&dcpw, &dipw};
    for (int k = 0; k < 2; k++) {
        const uint64_t len = arrays[k].second;
        HIP_TRY(hipMemsetAsync(planes[k]->p, 0, plane_bytes(len), pc.st));
        if (!len) continue;
        HIP_TRY(hipMemcpyAsync(draw.p, arrays[k].first, len, hipMemcpyHostToDevice, pc.st));
        uint4 *pw = (uint4 *)planes[k]->p + PLANE_PAD;
        if ((rc = pc.timed([&] {
                hipLaunchKernelGGL(k16_pack_call, dim3((uint32_t)std::min<uint64_t>((len + 255) / 256, 1u << 20)), dim3(256), 0, pc.st, (const uint8_t *)draw.p, len, pw);
            })))
            return rc;
    }
    const uint4 *cpw = (const uint4 *)dcpw.p + PLANE_PAD, *ipw = (const uint4 *)dipw.p + PLANE_PAD;
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    std::vector<uint64_t> order, start;
    window_stats_host::bucket_items(slices, items, nitems, order, start);
    uint64_t njobs_all = 0, slices_used = 0;
    for (size_t si = 0; si < slices.size(); si++) {
        if (start[si] == start[si + 1]) continue;   // no item asks for this slice: nothing of it is uploaded
        call_stats_host::plan_jobs(plan, windows, first, blocks, slices[si].first, items, order.data(), start[si], start[si + 1], job_columns, jobs);
        if (jobs.empty()) continue;
        slices_used++;
        if ((rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
        rc = pc.run(jobs, 4, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
            hipLaunchKernelGGL(k16_call_stats, grid, dim3(256), 0, pc.st, pc.t_fwd(), pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), (const SiteDesc *)dsites.p,
                               cpw, ipw, d_jobs, nj, (uint32_t *)dout.p);
        });
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` is rebuilt for the next slice
        njobs_all += jobs.size();
    }
    HIP_TRY(hipMemcpyAsync(out, dout.p, nitems * sizeof(mimeo_call_stats), hipMemcpyDeviceToHost, pc.st));
    HIP_TRY(hipStreamSynchronize(pc.st));
    for (uint64_t k = 0; k < nitems; k++) stack_host::query_stretch(first, blocks, items[k], &out[k].q_lo, &out[k].q_hi);   // the device left them zero
    if (pc.stats)
        fprintf(stderr, "[k16] call stats: %llu items, %llu sites, %llu jobs, slices %llu of %zu, launches %llu, kernels %.3f ms\n", (unsigned long long)nitems,
                (unsigned long long)nsites, (unsigned long long)njobs_all, (unsigned long long)slices_used, slices.size(), (unsigned long long)pc.launches,
                pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
