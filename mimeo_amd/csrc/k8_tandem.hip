// K8 — tandem-repeat scorer: the role of `trf F 2 7 7 80 10 50 50 -m -h -ngs` in mimeo map
// (reference src/mimeo/wrappers.py:120-262 trfFilter; flags src/mimeo/run_map.py:145-178).
// The reference only uses TRF's masked output to compute, per hit, the percentage of bases
// replaced by N and keeps the hit if it is below --maxtandem (wrappers.py:237-240).
//
// PARITY UNPINNED: TRF is an external heuristic program that is absent here; this is a
// specification of our own (DESIGN.md "Tandem scorer v2"), restated on the CPU in
// oracle/pipeline.py.  Like TRF it scores a candidate period p by aligning the sequence with a copy of itself p
// bases back, with TRF's three weights: +match, -mismatch, -delta per inserted or deleted base.  For every period
// p = 1 .. maxperiod the slice is aligned locally (scores restart at 0) with itself on the diagonals p - b .. p + b
// (b = 0 for p = 1, 1 for p < 5, else 2: a copy may drift by that many bases through indels):
//   H[j][d] = max(0, H[j-1][d] + s(S[j], S[j-d]), H[j-1][d-1] - delta, H[j][d+1] - delta)
// (ties: diagonal move, then the insertion, then the deletion); a path that reaches a new best >= minscore marks
// everything from the first base of its earlier copy to the base it has reached.  The masked set is the union over
// the periods.  delta <= 0 switches the indel moves off (b = 0): the gap-free scorer of round 1.  TRF's detection
// statistics (PM, PI) have no counterpart: every period is simply tried.
//
// One wavefront per slice, lane = period: each lane streams the slice 32 bases at a time with bit-parallel
// self-comparison masks per diagonal; qualified stretches are OR-ed into a per-slice bitmask.  maxperiod 65 .. 2000
// (TRF's own upper end): one wavefront per (slice, block of 64 periods), k8_tandem_mask_wide below.
#include "device_util.h"

namespace mimeo {

__device__ __forceinline__ void mark_range(uint32_t *__restrict__ bits, uint32_t a, uint32_t b) {
    // set bits [a, b) of the slice's mask
    while (a < b) {
        uint32_t w = a >> 5, lo = a & 31u, n = min(32u - lo, b - a);
        uint32_t m = (n == 32u ? 0xFFFFFFFFu : ((1u << n) - 1u)) << lo;
        atomicOr(&bits[w], m);
        a += n;
    }
}

constexpr int TBAND = 5;   // diagonals per period at most (b = 2)
struct TCell { int32_t h; uint32_t start, best, mend; };   // score; first base of the earlier copy; best on the path; masked up to

__global__ __launch_bounds__(256) void k8_tandem_mask(const StrandView *__restrict__ views,
                                                      const mimeo_interval *__restrict__ iv, uint64_t n,
                                                      const uint64_t *__restrict__ word_off, int match, int mismatch, int delta,
                                                      int minscore, int maxperiod, uint32_t *__restrict__ bits) {
    const uint64_t wid = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 6;
    if (wid >= n) return;
    const uint32_t p = (threadIdx.x & 63u) + 1u;
    if ((int)p > maxperiod) return;
    const mimeo_interval v = iv[wid];
    const StrandView S = views[v.chrom];
    const uint32_t end = min(v.end, S.len);
    if (v.start >= end) return;
    const uint32_t L = end - v.start;
    const uint32_t b = delta > 0 ? (p == 1 ? 0u : (p < 5 ? 1u : 2u)) : 0u, nd = 2 * b + 1, d0 = p - b;   // diagonals d0 .. d0 + nd - 1
    if (L <= d0) return;
    uint32_t *mybits = bits + word_off[wid];
    TCell cur[TBAND], prev[TBAND];
#pragma unroll
    for (int k = 0; k < TBAND; k++) prev[k] = TCell{0, 0, 0, 0};
    for (uint32_t j0 = (d0 / 32u) * 32u; j0 < L; j0 += 32) {
        const Win32 a = win32(S, (int32_t)(v.start + j0));
        uint32_t eq[TBAND];
#pragma unroll
        for (int k = 0; k < TBAND; k++) {
            eq[k] = 0;
            if ((uint32_t)k < nd) {
                const Win32 c = win32(S, (int32_t)(v.start + j0) - (int32_t)(d0 + k));
                eq[k] = ~((a.lo ^ c.lo) | (a.hi ^ c.hi)) & ~(a.nm | c.nm);
            }
        }
        const uint32_t cnt = min(32u, L - j0);
        for (uint32_t t = 0; t < cnt; t++) {
            const uint32_t j = j0 + t;
#pragma unroll
            for (int k = TBAND - 1; k >= 0; k--) {
                if ((uint32_t)k >= nd) continue;
                const uint32_t d = d0 + (uint32_t)k;
                TCell c{0, 0, 0, 0};
                if (j >= d) {
                    // diagonal move (a fresh path starts at the earlier copy's base j - d)
                    const TCell &pd = prev[k];
                    const int32_t sc = ((eq[k] >> t) & 1u) ? match : -mismatch;
                    c.h = pd.h + sc;
                    c.start = pd.h > 0 ? pd.start : j - d;
                    c.best = pd.h > 0 ? pd.best : 0;
                    c.mend = pd.h > 0 ? pd.mend : 0;
                    if (k > 0 && prev[k - 1].h - delta > c.h) { c = prev[k - 1]; c.h -= delta; }          // insertion: (j-1, d-1)
                    if ((uint32_t)k + 1 < nd && cur[k + 1].h - delta > c.h) { c = cur[k + 1]; c.h -= delta; }  // deletion: (j, d+1)
                    if (c.h <= 0) c = TCell{0, 0, 0, 0};
                    else if ((uint32_t)c.h > c.best) {
                        c.best = (uint32_t)c.h;
                        if (c.h >= minscore) {
                            mark_range(mybits, max(c.mend, c.start), j + 1);
                            c.mend = j + 1;
                        }
                    }
                }
                cur[k] = c;
            }
#pragma unroll
            for (int k = 0; k < TBAND; k++) prev[k] = cur[k];
        }
    }
}

// maxperiod beyond 64: one wavefront per job (slice, block) of host_plan::tandem_jobs, lane = period p = 64 * block + lane + 1,
// the same band, cells and recurrence as k8_tandem_mask, statement for statement.  What differs:
//  * the wave walks ONE j0, from (first diagonal of the block / 32) * 32 on.  A lane that starts before its own
//    (d0 / 32) * 32 only adds cells with j < d, which are zero.
//  * with the indel moves on, every lane of a block >= 1 has b = 2 and neighbouring periods share four of their five
//    diagonals: lane l compares the window with its own diagonal p alone, the masks of p - 2 .. p + 2 come from the lanes
//    l - 2 .. l + 2 (ds_bpermute), and the four diagonals beyond the block's ends (64 * block - 1, 64 * block,
//    64 * block + 65, 64 * block + 66) are loaded by the lanes 0 .. 3: one or two windows per lane and 32 bases instead of
//    six (470 -> 450 ms at maxperiod 2000).  Block 0 (b = 0, 1, 2 by period) and delta <= 0 (one
//    diagonal per lane) load per lane as k8_tandem_mask does.
//  * so no lane leaves early: one beyond maxperiod, or with L <= d0, still hands its mask to its neighbours; nd = 0 keeps
//    it from scoring.
// Loads before the slice: j0 >= 64 * block - 32 in a block >= 1 and the largest diagonal read is 64 * block + 66, so no
// window starts more than 98 bases before v.start (block 0: j0 = 0, diagonal <= 66); the planes have 256 zero bases
// (PLANE_PAD) in front.  The waves of a slice's blocks OR into the same mask words: mark_range is atomic.
__global__ __launch_bounds__(256) void k8_tandem_mask_wide(const StrandView *__restrict__ views,
                                                           const mimeo_interval *__restrict__ iv,
                                                           const host_plan::TandemJob *__restrict__ jobs, uint32_t njobs,
                                                           const uint64_t *__restrict__ word_off, int match, int mismatch,
                                                           int delta, int minscore, int maxperiod, uint32_t *__restrict__ bits) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);   // wave-uniform: scalar loads below
    if (jid >= njobs) return;
    const host_plan::TandemJob job = jobs[jid];
    const mimeo_interval v = iv[job.slice];
    const StrandView S = views[v.chrom];
    const uint32_t end = min(v.end, S.len);
    if (v.start >= end) return;
    const uint32_t L = end - v.start;
    const uint32_t lane = threadIdx.x & 63u, P0 = job.block * host_plan::TANDEM_BLOCK, p = P0 + lane + 1u;
    const uint32_t b = delta > 0 ? (p == 1 ? 0u : (p < 5 ? 1u : 2u)) : 0u, d0 = p - b;   // diagonals d0 .. d0 + nd - 1
    const uint32_t nd = (int)p <= maxperiod ? 2 * b + 1 : 0u;
    const bool share = job.block > 0 && delta > 0;
    const uint32_t dx = P0 - 1u + (lane < 2u ? lane : 64u + (lane & 3u));   // lanes 0 .. 3: the diagonals beyond the block's ends
    uint32_t *mybits = bits + word_off[job.slice];
    TCell cur[TBAND], prev[TBAND];
#pragma unroll
    for (int k = 0; k < TBAND; k++) prev[k] = TCell{0, 0, 0, 0};
    for (uint32_t j0 = (host_plan::tandem_block_first_diagonal(job.block, delta) / 32u) * 32u; j0 < L; j0 += 32) {
        const Win32 a = win32(S, (int32_t)(v.start + j0));
        uint32_t eq[TBAND];
        if (share) {
            const Win32 c = win32(S, (int32_t)(v.start + j0) - (int32_t)p);
            const uint32_t own = ~((a.lo ^ c.lo) | (a.hi ^ c.hi)) & ~(a.nm | c.nm);
            uint32_t ext = 0;
            if (lane < 4u) {
                const Win32 x = win32(S, (int32_t)(v.start + j0) - (int32_t)dx);
                ext = ~((a.lo ^ x.lo) | (a.hi ^ x.hi)) & ~(a.nm | x.nm);
            }
#pragma unroll
            for (int k = 0; k < TBAND; k++) {
                const uint32_t i = lane + (uint32_t)k;   // diagonal P0 - 1 + i: lane i - 2's own for 2 <= i <= 65, else one of the four
                const uint32_t o = (uint32_t)__shfl((int)own, (int)((i - 2u) & 63u));
                const uint32_t x = (uint32_t)__shfl((int)ext, (int)(i < 2u ? i : (i - 64u) & 3u));
                eq[k] = (i >= 2u && i <= 65u) ? o : x;
            }
        } else {
#pragma unroll
            for (int k = 0; k < TBAND; k++) {
                eq[k] = 0;
                if ((uint32_t)k < nd) {
                    const Win32 c = win32(S, (int32_t)(v.start + j0) - (int32_t)(d0 + k));
                    eq[k] = ~((a.lo ^ c.lo) | (a.hi ^ c.hi)) & ~(a.nm | c.nm);
                }
            }
        }
        const uint32_t cnt = min(32u, L - j0);
        for (uint32_t t = 0; t < cnt; t++) {
            const uint32_t j = j0 + t;
#pragma unroll
            for (int k = TBAND - 1; k >= 0; k--) {
                if ((uint32_t)k >= nd) continue;
                const uint32_t d = d0 + (uint32_t)k;
                TCell c{0, 0, 0, 0};
                if (j >= d) {
                    // diagonal move (a fresh path starts at the earlier copy's base j - d)
                    const TCell &pd = prev[k];
                    const int32_t sc = ((eq[k] >> t) & 1u) ? match : -mismatch;
                    c.h = pd.h + sc;
                    c.start = pd.h > 0 ? pd.start : j - d;
                    c.best = pd.h > 0 ? pd.best : 0;
                    c.mend = pd.h > 0 ? pd.mend : 0;
                    if (k > 0 && prev[k - 1].h - delta > c.h) { c = prev[k - 1]; c.h -= delta; }          // insertion: (j-1, d-1)
                    if ((uint32_t)k + 1 < nd && cur[k + 1].h - delta > c.h) { c = cur[k + 1]; c.h -= delta; }  // deletion: (j, d+1)
                    if (c.h <= 0) c = TCell{0, 0, 0, 0};
                    else if ((uint32_t)c.h > c.best) {
                        c.best = (uint32_t)c.h;
                        if (c.h >= minscore) {
                            mark_range(mybits, max(c.mend, c.start), j + 1);
                            c.mend = j + 1;
                        }
                    }
                }
                cur[k] = c;
            }
#pragma unroll
            for (int k = 0; k < TBAND; k++) prev[k] = cur[k];
        }
    }
}

__global__ void k8_tandem_count(const mimeo_interval *__restrict__ iv, uint64_t n, const uint64_t *__restrict__ word_off,
                                const uint32_t *__restrict__ bits, uint32_t *__restrict__ masked) {
    const uint64_t wid = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (wid >= n) return;
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t c = 0;
    for (uint64_t w = word_off[wid] + lane; w < word_off[wid + 1]; w += 64) c += __popc(bits[w]);
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) masked[wid] = c;
}

int tandem_masked_device(const mimeo_genome *A, const mimeo_interval *h_iv, uint64_t n, int match, int mismatch, int delta,
                         int minscore, int maxperiod, uint32_t *h_masked, std::vector<uint32_t> *h_words) {
    if (h_words) h_words->clear();
    if (!n) return 0;
    if (maxperiod < 1 || maxperiod > host_plan::TANDEM_MAXPERIOD) { set_error("tandem scorer: maxperiod must be in 1..2000"); return MIMEO_ERR_LIMIT; }
    const bool wide = maxperiod > (int)host_plan::TANDEM_BLOCK;
    if (wide && n > 0xFFFFFFFFull) { set_error("tandem scorer: more than 2^32 - 1 slices in one call"); return MIMEO_ERR_LIMIT; }
    hipStream_t st = stream();
    std::vector<StrandView> views(A->scaf.size());
    for (size_t i = 0; i < views.size(); i++) views[i] = A->scaf[i].fwd.view(false);
    std::vector<uint64_t> off(n + 1, 0);
    std::vector<uint32_t> lengths;   // of the slices, for the job list of the wide kernel
    for (uint64_t i = 0; i < n; i++) {
        if (h_iv[i].chrom >= views.size()) { set_error("tandem scorer: chromosome id out of range"); return MIMEO_ERR_ARG; }
        uint32_t e = std::min<uint32_t>(h_iv[i].end, views[h_iv[i].chrom].len);
        uint64_t L = h_iv[i].start < e ? e - h_iv[i].start : 0;
        off[i + 1] = off[i] + (L + 31) / 32;
        if (wide) lengths.push_back((uint32_t)L);
    }
    std::vector<host_plan::TandemJob> jobs;
    if (wide) jobs = host_plan::tandem_jobs(lengths, maxperiod, delta);
    DeviceBuf dv, di, dof, db, dm, dj;
    int rc;
    if ((wide && (rc = dj.reserve(std::min<uint64_t>(jobs.size(), host_plan::TANDEM_CHUNK_JOBS) * sizeof(host_plan::TandemJob) + 16))) ||
        (rc = dv.reserve(views.size() * sizeof(StrandView) + 16)) || (rc = di.reserve(n * sizeof(mimeo_interval))) ||
        (rc = dof.reserve((n + 1) * 8)) || (rc = db.reserve(off[n] * 4 + 16)) || (rc = dm.reserve(n * 4)))
        return rc;
    HIP_TRY(hipMemcpyAsync(dv.p, views.data(), views.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(di.p, h_iv, n * sizeof(mimeo_interval), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dof.p, off.data(), (n + 1) * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(db.p, 0, off[n] * 4 + 16, st));
    HIP_TRY(hipMemsetAsync(dm.p, 0, n * 4, st));
    const uint32_t nb = (uint32_t)((n * 64 + 255) / 256);
    if (!wide)
        hipLaunchKernelGGL(k8_tandem_mask, dim3(nb), dim3(256), 0, st, (const StrandView *)dv.p, (const mimeo_interval *)di.p, n,
                           (const uint64_t *)dof.p, match, mismatch, delta, minscore, maxperiod, (uint32_t *)db.p);
    // the job list goes up TANDEM_CHUNK_JOBS jobs at a time, so it never takes more than TANDEM_CHUNK_BYTES = 64 MiB of device
    // memory (plus the quarter of slack DeviceBuf adds); the stream orders a chunk's copy behind the launch that read the
    // chunk before
    for (uint64_t j0 = 0; j0 < jobs.size(); j0 += host_plan::TANDEM_CHUNK_JOBS) {
        const uint64_t nj = std::min<uint64_t>(jobs.size() - j0, host_plan::TANDEM_CHUNK_JOBS);
        HIP_TRY(hipMemcpyAsync(dj.p, jobs.data() + j0, nj * sizeof(host_plan::TandemJob), hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k8_tandem_mask_wide, dim3((uint32_t)((nj * 64 + 255) / 256)), dim3(256), 0, st, (const StrandView *)dv.p,
                           (const mimeo_interval *)di.p, (const host_plan::TandemJob *)dj.p, (uint32_t)nj, (const uint64_t *)dof.p, match,
                           mismatch, delta, minscore, maxperiod, (uint32_t *)db.p);
    }
    hipLaunchKernelGGL(k8_tandem_count, dim3(nb), dim3(256), 0, st, (const mimeo_interval *)di.p, n,
                       (const uint64_t *)dof.p, (const uint32_t *)db.p, (uint32_t *)dm.p);
    HIP_TRY(hipMemcpyAsync(h_masked, dm.p, n * 4, hipMemcpyDeviceToHost, st));
    if (h_words) {   // the words k8_tandem_count has just summed: slice k owns off[k] .. off[k + 1]
        h_words->resize(off[n]);
        if (off[n]) HIP_TRY(hipMemcpyAsync(h_words->data(), db.p, off[n] * 4, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    HIP_TRY(hipGetLastError());
    for (DeviceBuf *b : {&dv, &di, &dof, &db, &dm, &dj}) b->release();
    return 0;
}

}  // namespace mimeo
