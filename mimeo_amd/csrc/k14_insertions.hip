// K14 — the insertion columns of a pileup and a base called from each (mimeo_path_insertions, include/mimeo_hip.h "pileup v2,
// insertion columns"): what K13 (k13_pileup.hip) counts in ins_runs / ins_bases and leaves out of its call.  A site is the
// position in front of one target base of one window; the rows that insert there (a block b_k, k > 0, whose gap starts at
// p_k == x with dq_k > 0 query bases skipped) pile their inserted bases up left-aligned in the site's columns.
//
// Work layout.  The access pattern is not K13's: the sites are sparse, and a run of query bases has no target column under it.
// The host (insert_host.h) cuts the sorted sites into tiles — runs of sites of one window with at most TILE_COLS columns between
// them — and buckets a slice's items onto the tiles of whose sites they hold some; a job is a tile with a run of at most JOB_ITEMS
// of its entries.  One workgroup of four wavefronts takes a job: it zeroes the tile's five counter planes and the tile's site
// results in LDS, the wavefronts take the entries round-robin, and for an entry a wavefront goes over the entry's sites 64 per
// pass: lane i takes site s0 + i, finds the first block that ends behind x by binary search (path_call.h) and tests k > b0,
// p_k == x, dq_k > 0.  The lanes that hold a run are balloted and broadcast one by one, wave-uniformly — the run's query start,
// dq, the site's LDS offset and ncols — and a run goes 64 inserted bases per step: one win64 of the query at the wave-uniform
// start gives the planes, lane j takes bit j, picks its class and adds 1 at plane[class][off + j], consecutive lanes on
// consecutive banks (K13's lesson: the lanes are the columns, the walk is wave-uniform).  One lane adds the site's runs, bases,
// longer and max_len.  Every LDS update is a non-returning atomic: four wavefronts share the tile.  After a barrier the
// workgroup adds the tile's non-zero counters to the batch's counts in global memory with integer atomics (max for max_len).  A
// tile may be fed by several jobs, launches and slices; the batch's counts are zeroed once on the stream.  k14_ins_call then
// reads a column's five counts and its site's voters and writes the byte.
// Integers only: exact, and independent of the grid, the slices, the batches, the cut into jobs and the order of the items.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "insert_host.h"
#include "path_call.h"

namespace mimeo {

using insert_host::Entry;
using insert_host::Job;
using insert_host::SiteDesc;
using insert_host::TILE_COLS;

constexpr uint32_t IPLANE = TILE_COLS + 8;   // words between two counter planes in LDS: column i of plane c lies on bank (i + 8 c) mod 64
enum { I_N = 4, R_RUNS = 0, R_BASES = 1, R_LONGER = 2, R_MAX = 3 };   // plane 0 .. 3: A C G T; the fields of mimeo_insert_result

__global__ __launch_bounds__(256) void k14_ins_pileup(const StrandView *__restrict__ q_fwd, const StrandView *__restrict__ q_rc,
                                                      const mimeo_alignment *__restrict__ aln, const uint64_t *__restrict__ first,
                                                      const mimeo_path_block *__restrict__ blocks, const SiteDesc *__restrict__ sites,
                                                      const Entry *__restrict__ entries, const Job *__restrict__ jobs, uint32_t njobs,
                                                      uint32_t *__restrict__ counts, uint32_t *__restrict__ results) {
    __shared__ uint32_t cnt[5 * IPLANE];
    __shared__ uint32_t res[4 * TILE_COLS];   // a tile has at most TILE_COLS sites: every site has a column
    if (blockIdx.x >= njobs) return;   // never: the grid is the number of jobs
    const Job job = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < 5 * IPLANE; i += 256) cnt[i] = 0;
    for (uint32_t i = threadIdx.x; i < 4u * job.nsites; i += 256) res[i] = 0;
    __syncthreads();
    for (uint32_t e = wave; e < job.nitems; e += 4) {   // wave-uniform
        const Entry en = entries[job.item0 + e];         // job.site0 <= s0 < s1 <= job.site0 + job.nsites (insert_host.h)
        const mimeo_alignment a = aln[en.aln];
        const GStrandView Q((a.qstrand ? q_rc : q_fwd)[a.qid]);
        const uint64_t b0 = first[en.aln] - first[0], b1 = first[en.aln + 1] - first[0];   // the slice's blocks start at first[0]; b1 > b0
        for (uint32_t s = en.s0; s < en.s1; s += 64) {
            uint32_t qs = 0, dq = 0, off = 0, nc = 0;
            bool run = false;
            if (s + lane < en.s1) {
                const SiteDesc d = sites[s + lane];
                // the first block that ends behind x; x lies in front of the last block's end (the host clipped the item to the
                // alignment), so there is one, and the test on b1 never fails
                const uint64_t k = first_block_ending_behind(blocks, b0, b1, d.x);
                if (k > b0 && k < b1) {
                    const mimeo_path_block pb = blocks[k - 1], b = blocks[k];
                    qs = pb.q + pb.len;
                    dq = b.q - qs;
                    off = d.off - job.icol0;
                    nc = d.ncols;
                    run = pb.t + pb.len == d.x && dq > 0;   // p_k == x: not inside a deletion, not inside a block
                }
            }
            for (uint64_t m = __ballot(run); m; m &= m - 1) {   // wave-uniform: one run after the other
                const int j = __builtin_ctzll(m);
                const uint32_t jqs = (uint32_t)__builtin_amdgcn_readlane((int)qs, j), jdq = (uint32_t)__builtin_amdgcn_readlane((int)dq, j);
                const uint32_t joff = (uint32_t)__builtin_amdgcn_readlane((int)off, j), jnc = (uint32_t)__builtin_amdgcn_readlane((int)nc, j);
                if (lane == 0) {
                    uint32_t *r = res + 4u * (s + (uint32_t)j - job.site0);
                    atomicAdd(r + R_RUNS, 1u);
                    atomicAdd(r + R_BASES, jdq);
                    if (jdq > jnc) atomicAdd(r + R_LONGER, 1u);
                    atomicMax(r + R_MAX, jdq);
                }
                // the run's inserted bases, clipped to the site's columns, 64 per step.  Bounds of the window read: an inserted
                // base lies below the following block's q, hence below q + len <= Lq (checked on the host), and win64 reads the
                // three words from that base's word on: at most two words behind the strand's last, inside the PLANE_PAD = 8 zero
                // words that follow it.  Bounds of the LDS add: joff + o + lane < joff + jnc <= job.ncols <= TILE_COLS.
                const uint32_t end = min(jdq, jnc);
                for (uint32_t o = 0; o < end; o += 64) {
                    const Win64 w = win64(Q, (int32_t)(jqs + o));
                    if (o + lane < end) {
                        const uint32_t cls = ((w.nm >> lane) & 1ull) ? (uint32_t)I_N : (uint32_t)(((w.lo >> lane) & 1ull) | (((w.hi >> lane) & 1ull) << 1));
                        atomicAdd(&cnt[cls * IPLANE + joff + o + lane], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    // the batch's counts are laid out as the output: five counters per column, four results per site
    uint32_t *dst = counts + (uint64_t)job.icol0 * 5u;
    for (uint32_t i = threadIdx.x; i < (uint32_t)job.ncols * 5u; i += 256) {
        const uint32_t c = i / 5u, v = cnt[(i - c * 5u) * IPLANE + c];
        if (v) atomicAdd(dst + i, v);
    }
    uint32_t *rdst = results + (uint64_t)job.site0 * 4u;
    for (uint32_t i = threadIdx.x; i < (uint32_t)job.nsites * 4u; i += 256) {
        const uint32_t v = res[i];
        if (v) { if ((i & 3u) == R_MAX) atomicMax(rdst + i, v); else atomicAdd(rdst + i, v); }
    }
}

// The call byte of every insertion column of a batch (mimeo_hip.h "Call, per insertion column"): a thread per column.  The
// column's site is the last one whose first column is not behind it: a binary search over the batch's sites, whose `off` rise.
__global__ __launch_bounds__(256) void k14_ins_call(const SiteDesc *__restrict__ sites, uint32_t nsites, uint32_t ncols, const uint32_t *__restrict__ counts,
                                                    uint8_t *__restrict__ call) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= ncols) return;
    uint32_t lo = 0, hi = nsites;   // sites[lo].off <= i < sites[hi].off; sites[0].off == 0
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (sites[mid].off <= i) lo = mid; else hi = mid;
    }
    const uint32_t voters = sites[lo].voters;
    const uint32_t *c = counts + (uint64_t)i * 5u;
    const uint32_t v[4] = {c[0], c[1], c[2], c[3]}, n = c[4];
    uint32_t best = 0;
#pragma unroll
    for (uint32_t b = 1; b < 4; b++) if (v[b] > v[best]) best = b;   // among equal counts the order is A, C, G, T
    const uint32_t top = v[best];
    const uint64_t total = (uint64_t)v[0] + v[1] + v[2] + v[3] + n;
    const uint64_t vg = voters > total ? voters - total : 0;
    call[i] = top > vg ? (uint8_t)(0x54474341u /* 'A' 'C' 'G' 'T' */ >> (best << 3)) : (top == 0 && n > vg) ? (uint8_t)'N' : (uint8_t)'-';
}

static_assert(sizeof(mimeo_insert_site) == 16 && sizeof(mimeo_insert_result) == 16 && sizeof(mimeo_insert_column) == 20 && sizeof(Job) == 20 &&
                  sizeof(Entry) == 12 && sizeof(SiteDesc) == 16 && sizeof(mimeo_path_block) == 12,
              "layouts the kernels rely on");
static_assert(TILE_COLS % 64 == 0 && TILE_COLS <= 0xFFFFu && (5 * IPLANE + 4 * TILE_COLS) * 4 <= 64 * 1024, "the tile: whole wavefronts, Job::ncols, static LDS");

// MIMEO_INSERT_SLICE_BLOCKS: blocks per slice (default 2^24, as K9; 1: every alignment a slice of its own);
// MIMEO_INSERT_JOB_ITEMS: entries of a job, at most (default 64); MIMEO_INSERT_COLUMNS: insertion columns per batch (default
// 2^22: 80 MiB of counts; at most 2^28; a tile goes in whole); MIMEO_INSERT_STATS: what the call did and the HIP-event time of
// its kernels, on stderr.  Results depend on none of them.
int path_insertions_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                           const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                           uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, mimeo_insert_result *res, mimeo_insert_column *icols,
                           uint8_t *icall) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad window, item or site reaches the kernels
    std::string msg;
    if (!insert_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, windows, nwin, items, nitems, sites, nsites, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    if (!res && !icols && !icall) return 0;
    const insert_host::Sites plan = insert_host::plan_sites(sites, nsites, nwin);
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_INSERT_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t job_items = env_u64("MIMEO_INSERT_JOB_ITEMS", insert_host::JOB_ITEMS);
    const uint64_t batch_columns = std::min(std::max<uint64_t>(1, env_u64("MIMEO_INSERT_COLUMNS", 1ull << 22)), insert_host::MAX_BATCH_COLUMNS);
    const uint64_t run_entries = 1ull << 22;   // entries of one upload: 48 MiB
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    std::vector<SiteDesc> desc;
    insert_host::TileItems ti;
    insert_host::Batch batch;
    PathCall pc(getenv("MIMEO_INSERT_STATS") != nullptr);
    DeviceBuf &dcnt = pc.buf(), &dres = pc.buf(), &dcall = pc.buf(), &dsites = pc.buf(), &dent = pc.buf();
    int rc;
    if ((rc = pc.views(T, Q))) return rc;
    std::vector<std::pair<uint64_t, uint64_t>> slices;
    std::vector<uint64_t> order, start;
    if (nitems) {
        slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
        window_stats_host::bucket_items(slices, items, nitems, order, start);
    }
    uint64_t njobs_all = 0, nbatches = 0, slice_uploads = 0;
    for (uint64_t tile0 = 0; tile0 < plan.tiles.size(); tile0 = batch.tile1) {
        batch = insert_host::plan_batch(plan, tile0, batch_columns);
        nbatches++;
        insert_host::batch_sites(plan, batch, sites, desc);
        if ((rc = dcnt.reserve(batch.ncols * sizeof(mimeo_insert_column))) || (rc = dres.reserve(batch.nsites * sizeof(mimeo_insert_result))) ||
            (rc = dsites.reserve(batch.nsites * sizeof(SiteDesc))))
            return rc;
        HIP_TRY(hipMemsetAsync(dcnt.p, 0, batch.ncols * sizeof(mimeo_insert_column), pc.st));   // once per batch: every job adds to them
        HIP_TRY(hipMemsetAsync(dres.p, 0, batch.nsites * sizeof(mimeo_insert_result), pc.st));
        HIP_TRY(hipMemcpyAsync(dsites.p, desc.data(), batch.nsites * sizeof(SiteDesc), hipMemcpyHostToDevice, pc.st));
        for (size_t si = 0; si < slices.size(); si++) {
            bool uploaded = false;
            for (uint64_t i0 = start[si]; i0 < start[si + 1];) {
                i0 = insert_host::bucket_tiles(plan, batch, first, blocks, slices[si].first, sites, items, order.data(), i0, start[si + 1], run_entries, ti);
                if (ti.entries.empty()) continue;   // no item of the run holds a site of the batch: nothing of the slice is uploaded for it
                insert_host::plan_jobs(plan, batch, ti, job_items, jobs);
                if (!uploaded && (rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
                slice_uploads += !uploaded;
                uploaded = true;
                if ((rc = dent.reserve(ti.entries.size() * sizeof(Entry)))) return rc;
                HIP_TRY(hipMemcpyAsync(dent.p, ti.entries.data(), ti.entries.size() * sizeof(Entry), hipMemcpyHostToDevice, pc.st));
                rc = pc.run(jobs, 1, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
                    hipLaunchKernelGGL(k14_ins_pileup, grid, dim3(256), 0, pc.st, pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), (const SiteDesc *)dsites.p,
                                       (const Entry *)dent.p, d_jobs, nj, (uint32_t *)dcnt.p, (uint32_t *)dres.p);
                });
                if (rc) return rc;
                HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` and `ti` are rebuilt for the next run
                njobs_all += jobs.size();
            }
        }
        if (icall) {
            if ((rc = dcall.reserve(batch.ncols))) return rc;
            if ((rc = pc.timed([&] {
                    hipLaunchKernelGGL(k14_ins_call, dim3((uint32_t)((batch.ncols + 255) / 256)), dim3(256), 0, pc.st, (const SiteDesc *)dsites.p, (uint32_t)batch.nsites,
                                       (uint32_t)batch.ncols, (const uint32_t *)dcnt.p, (uint8_t *)dcall.p);
                })))
                return rc;
            HIP_TRY(hipMemcpyAsync(icall + batch.icol0, dcall.p, batch.ncols, hipMemcpyDeviceToHost, pc.st));
        }
        if (icols) HIP_TRY(hipMemcpyAsync(icols + batch.icol0, dcnt.p, batch.ncols * sizeof(mimeo_insert_column), hipMemcpyDeviceToHost, pc.st));
        if (res) HIP_TRY(hipMemcpyAsync(res + batch.site0, dres.p, batch.nsites * sizeof(mimeo_insert_result), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));   // the batch is out, and `batch` and `desc` may be rebuilt
    }
    if (pc.stats)
        fprintf(stderr, "[k14] insertions: %llu items, %llu sites, %llu columns, %llu tiles, %llu jobs, slices %llu of %zu, batches %llu, launches %llu, kernels %.3f ms\n",
                (unsigned long long)nitems, (unsigned long long)nsites, (unsigned long long)plan.nicols(), (unsigned long long)plan.tiles.size(),
                (unsigned long long)njobs_all, (unsigned long long)slice_uploads, slices.size(), (unsigned long long)nbatches, (unsigned long long)pc.launches,
                pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
