// K12 — repeat families: regions linked through alignment paths (mimeo_link_regions, include/mimeo_hip.h "family linking v1").
// An item is an alignment row and a region r of its target scaffold with the window [w0, w1) the row covers of it.  Rule A
// (the window covers min_cover_pct of r) is decided on the host (link_regions_host.h: an item that fails makes no job); the
// kernel does B and C: the window is projected through the path's blocks onto the query scaffold's plus strand, and every
// region s != r of that scaffold of which the projection covers min_cover_pct joins r's family and counts in links[r].
//
// Work layout: one lane per job.  A job is three dependent binary searches (the first block that ends behind w0, the last
// block that starts in front of w1, the first region of the query scaffold that ends behind the projection) and a short loop
// over the regions under the projection: not a wavefront's worth.  Jobs arrive in the order of the call's items inside a
// slice — by record, then region, as formats.region_items makes them — so neighbouring lanes walk the same path.
//
// Union-find: parent[nreg] lives on the device for the whole call, across slices and launches.  parent[x] <= x always, a root
// is its own parent, and a hook always puts the LARGER root under the smaller (one compare-and-swap on parent[hi], expected
// value hi); where it fails somebody else hooked hi first and the lane starts again from find.  No lane ever waits for another
// lane's progress: the lanes of a wavefront run in lockstep, and every retry follows somebody's successful hook.  find halves
// the path with atomicMin, so a parent only ever decreases and stays an ancestor.  The root of a component is therefore its
// smallest member whatever the order of the hooks: the labels depend on the set of links alone.  The parents are read with
// agent-scope atomic loads: a CU's vector L1 is not refreshed by another CU's stores.  A second small kernel writes
// family[i] = root(i).  links[] are 64-bit integer atomics.  Integers only: exact, and independent of the grid, the slices and
// the order of the items.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "link_regions_host.h"
#include "path_call.h"

namespace mimeo {

using link_regions_host::Job;

__device__ __forceinline__ uint32_t k12_parent(const uint32_t *parent, uint32_t x) {
    return __hip_atomic_load(parent + x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// the root of x, halving the path on the way; every index read is a value of parent[] or x itself: below nreg
__device__ __forceinline__ uint32_t k12_find(uint32_t *parent, uint32_t x) {
    for (;;) {
        const uint32_t p = k12_parent(parent, x);
        if (p == x) return x;
        const uint32_t g = k12_parent(parent, p);
        if (g != p) atomicMin(parent + x, g);   // g < p < x: still an ancestor, and parent[x] only decreases
        x = p;
    }
}

__device__ __forceinline__ void k12_unite(uint32_t *parent, uint32_t a, uint32_t b) {
    for (;;) {
        a = k12_find(parent, a);
        b = k12_find(parent, b);
        if (a == b) return;
        const uint32_t hi = a > b ? a : b, lo = a > b ? b : a;
        if (atomicCAS(parent + hi, hi, lo) == hi) return;   // lost: hi was hooked by another lane meanwhile — find again
    }
}

__global__ __launch_bounds__(256) void k12_link_regions(const mimeo_alignment *__restrict__ aln, const uint64_t *__restrict__ first,
                                                        const mimeo_path_block *__restrict__ blocks, const Job *__restrict__ jobs, uint32_t njobs,
                                                        const mimeo_interval *__restrict__ regions, const uint32_t *__restrict__ chrom_first,
                                                        const uint32_t *__restrict__ chrom_of_scaf, const uint32_t *__restrict__ scaf_len, uint32_t pct,
                                                        uint32_t *parent, unsigned long long *links) {
    const uint32_t jid = blockIdx.x * 256u + threadIdx.x;
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const mimeo_alignment a = aln[job.aln];
    const uint64_t b0 = first[job.aln] - first[0], b1 = first[job.aln + 1] - first[0];   // the slice's blocks start at first[0]; b1 > b0 (host)
    const uint32_t w0 = job.w0, w1 = job.w1;                                              // w0 < w1 (rule A, host)
    // B: the first block that ends behind w0 ...
    const uint64_t ks = first_block_ending_behind(blocks, b0, b1, w0);
    if (ks == b1) return;   // the window lies behind the alignment
    const mimeo_path_block bs = blocks[ks];
    const uint32_t s = max(bs.t, w0);
    if (s >= w1) return;    // ... starts behind the window: the window lies in a deletion, or in front of the alignment
    // ... and the last block that starts in front of w1: block ks does
    uint64_t lo = ks, hi = b1 - 1;
    while (lo < hi) {
        const uint64_t mid = (lo + hi + 1) >> 1;
        if (blocks[mid].t < w1) lo = mid; else hi = mid - 1;
    }
    const mimeo_path_block be = blocks[lo];
    const uint32_t q_lo = bs.q + (s - bs.t), q_hi = be.q + (min(be.t + be.len, w1) - be.t);   // q_lo < q_hi <= the query scaffold's length
    const uint32_t Lq = scaf_len[a.qid];
    const uint32_t p0 = a.qstrand ? Lq - q_hi : q_lo, p1 = a.qstrand ? Lq - q_lo : q_hi;      // the projection on the plus strand
    // C: the regions of the query scaffold under [p0, p1): the first one that ends behind p0 (the regions are disjoint and sorted:
    // their ends are sorted like their starts)
    const uint32_t c = chrom_of_scaf[a.qid];
    uint32_t r0 = chrom_first[c];
    const uint32_t r1 = chrom_first[c + 1];
    uint32_t rh = r1;
    while (r0 < rh) {
        const uint32_t mid = r0 + ((rh - r0) >> 1);
        if (regions[mid].end > p0) rh = mid; else r0 = mid + 1;
    }
    uint32_t nlinks = 0;
    for (uint32_t k = r0; k < r1; k++) {
        const mimeo_interval v = regions[k];
        if (v.start >= p1) break;
        const uint64_t ov = (uint64_t)(min(v.end, p1) - max(v.start, p0));   // > 0: v ends behind p0 and starts in front of p1
        if (100ull * ov >= (uint64_t)pct * (uint64_t)(v.end - v.start) && k != job.region) {
            k12_unite(parent, job.region, k);
            nlinks++;
        }
    }
    if (nlinks) atomicAdd(links + job.region, (unsigned long long)nlinks);
}

__global__ __launch_bounds__(256) void k12_init(uint32_t *parent, uint32_t nreg) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < nreg) parent[i] = i;
}

// family[i] = root(i); nothing is hooked any more, so the walk only reads
__global__ __launch_bounds__(256) void k12_flatten(const uint32_t *__restrict__ parent, uint32_t nreg, uint32_t *__restrict__ family) {
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= nreg) return;
    uint32_t x = i;
    for (;;) {
        const uint32_t p = k12_parent(parent, x);
        if (p == x) break;
        x = p;
    }
    family[i] = x;
}

static_assert(sizeof(mimeo_interval) == 12 && sizeof(mimeo_window_item) == 16 && sizeof(Job) == 16 && sizeof(mimeo_path_block) == 12,
              "layouts the kernel relies on");

// MIMEO_LINK_SLICE_BLOCKS: blocks per slice (default 2^24, as K9 and K10; 1: every alignment a slice of its own);
// MIMEO_LINK_STATS: what the call did and the HIP-event time of its kernels, on stderr.  Results depend on neither.
int link_regions_device(const mimeo_genome *T, const mimeo_alignment *aln, uint64_t n, const uint64_t *first, const mimeo_path_block *blocks,
                        uint64_t nblocks, const mimeo_interval *regions, uint64_t nreg, const uint32_t *chrom_of_scaf, const mimeo_window_item *items,
                        uint64_t nitems, uint32_t min_cover_pct, uint32_t *family, uint64_t *links) {
    // every check on the host, before anything is uploaded: no bad path, region or item reaches the kernel
    const std::vector<uint64_t> len_t = scaffold_lengths(T);
    std::string msg;
    std::vector<uint32_t> chrom;
    if (!link_regions_host::validate(len_t, aln, n, first, blocks, nblocks, regions, nreg, chrom_of_scaf, items, nitems, min_cover_pct, chrom, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_LINK_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const std::vector<uint32_t> chrom_first = link_regions_host::chrom_offsets(regions, nreg, chrom.size());
    const std::vector<uint32_t> scaf_len(len_t.begin(), len_t.end());   // scaffolds are below 2^31 bases
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    PathCall pc(getenv("MIMEO_LINK_STATS") != nullptr);
    DeviceBuf &dreg = pc.buf(), &dcf = pc.buf(), &dcs = pc.buf(), &dsl = pc.buf(), &dpar = pc.buf(), &dfam = pc.buf(), &dlnk = pc.buf();
    int rc;
    if ((rc = dreg.reserve(nreg * sizeof(mimeo_interval) + 16)) || (rc = dcf.reserve(chrom_first.size() * 4)) || (rc = dcs.reserve(chrom.size() * 4 + 16)) ||
        (rc = dsl.reserve(scaf_len.size() * 4 + 16)) || (rc = dpar.reserve(nreg * 4)) || (rc = dfam.reserve(nreg * 4)) || (rc = dlnk.reserve(nreg * 8)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dreg.p, regions, nreg * sizeof(mimeo_interval), hipMemcpyHostToDevice, pc.st));
    HIP_TRY(hipMemcpyAsync(dcf.p, chrom_first.data(), chrom_first.size() * 4, hipMemcpyHostToDevice, pc.st));
    HIP_TRY(hipMemcpyAsync(dcs.p, chrom.data(), chrom.size() * 4, hipMemcpyHostToDevice, pc.st));
    HIP_TRY(hipMemcpyAsync(dsl.p, scaf_len.data(), scaf_len.size() * 4, hipMemcpyHostToDevice, pc.st));
    HIP_TRY(hipMemsetAsync(dlnk.p, 0, nreg * 8, pc.st));   // once per call: every job adds to it
    const dim3 reg_grid((uint32_t)((nreg + 255) / 256));
    if ((rc = pc.timed([&] { hipLaunchKernelGGL(k12_init, reg_grid, dim3(256), 0, pc.st, (uint32_t *)dpar.p, (uint32_t)nreg); }))) return rc;
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    std::vector<uint64_t> order, start;
    window_stats_host::bucket_items(slices, items, nitems, order, start);
    uint64_t njobs_all = 0, slices_used = 0;
    for (size_t si = 0; si < slices.size(); si++) {
        if (start[si] == start[si + 1]) continue;   // no item asks for this slice: nothing of it is uploaded
        link_regions_host::plan_jobs(first, slices[si].first, regions, items, order.data(), start[si], start[si + 1], min_cover_pct, jobs);
        if (jobs.empty()) continue;
        slices_used++;
        if ((rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
        rc = pc.run(jobs, 256, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {   // one lane per job
            hipLaunchKernelGGL(k12_link_regions, grid, dim3(256), 0, pc.st, pc.aln(), pc.first(), pc.blocks(), d_jobs, nj, (const mimeo_interval *)dreg.p,
                               (const uint32_t *)dcf.p, (const uint32_t *)dcs.p, (const uint32_t *)dsl.p, min_cover_pct, (uint32_t *)dpar.p,
                               (unsigned long long *)dlnk.p);
        });
        if (rc) return rc;
        HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` is rebuilt for the next slice
        njobs_all += jobs.size();
    }
    rc = pc.timed([&] { hipLaunchKernelGGL(k12_flatten, reg_grid, dim3(256), 0, pc.st, (const uint32_t *)dpar.p, (uint32_t)nreg, (uint32_t *)dfam.p); });
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(family, dfam.p, nreg * 4, hipMemcpyDeviceToHost, pc.st));
    HIP_TRY(hipMemcpyAsync(links, dlnk.p, nreg * 8, hipMemcpyDeviceToHost, pc.st));
    HIP_TRY(hipStreamSynchronize(pc.st));
    if (pc.stats)
        fprintf(stderr, "[k12] link regions: %llu items, %llu regions, %llu jobs, slices %llu of %zu, launches %llu, kernels %.3f ms\n",
                (unsigned long long)nitems, (unsigned long long)nreg, (unsigned long long)njobs_all, (unsigned long long)slices_used, slices.size(),
                (unsigned long long)pc.launches, pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
