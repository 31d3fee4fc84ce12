// K6: paths out, the blocks of every returned alignment in dense order (paths_pass, dense_paths_device); overview in k6_gapped.hip.
#include <cstring>   // rocPRIM's headers call memset without including it
#include <rocprim/rocprim.hpp>

#include "k6.h"

namespace mimeo {

// ---- paths out (mimeo_align_units_paths) ----------------------------------------------------------------------------------
// The path of a returned alignment = the blocks of its left half, then those of its right half (both sorted by t, strand
// coordinates), two consecutive blocks merged when the second continues the first on its diagonal — at the anchor, when both
// halves leave it diagonally.  Under the path rule every extended half has its blocks already; under the box rule one trace
// pass after the last round makes those of the alignments that are returned (paths_pass); gap-free mode writes one block per
// alignment (k6_ungapped_paths).  accrank, compacted as k6_finish compacts the alignments (k6_kept_ranks), names the halves.

// box rule: the two halves of every accepted alignment with score >= thresh, as jobs for k6_trace.  One thread per group;
// jobs == nullptr: count only (ctr[0]), else the list (ctr[1]: its fill)
__global__ void k6_kept_jobs(const Group *__restrict__ groups, uint32_t ngroups, const mimeo_alignment *__restrict__ aln,
                             const uint2 *__restrict__ anchors, const uint32_t *__restrict__ accrank, int32_t thresh,
                             DpJob *__restrict__ jobs, unsigned int *__restrict__ ctr) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    const Group &G = groups[g];
    const uint64_t b0 = G.hsp_begin;
    uint32_t n = 0;
    for (uint32_t e = 0; e < G.nacc; e++) n += aln[b0 + e].score >= thresh ? 1u : 0u;
    if (!n) return;
    if (!jobs) { atomicAdd(&ctr[0], 2u * n); return; }
    unsigned int j = atomicAdd(&ctr[1], 2u * n);
    for (uint32_t e = 0; e < G.nacc; e++) {
        if (aln[b0 + e].score < thresh) continue;
        const uint32_t rank = accrank[b0 + e];
        const uint2 a = anchors[b0 + rank];
        const uint32_t slot = 2u * (uint32_t)(b0 + rank);
        jobs[j++] = DpJob{g, a.x, a.y, -1, slot, 0};
        jobs[j++] = DpJob{g, a.x, a.y, +1, slot + 1, 0};
    }
}

// after k6_finish and k6_dense_offsets: the left half slot of every returned alignment, in dense order
__global__ __launch_bounds__(64) void k6_path_slots(const Group *__restrict__ groups, const uint32_t *__restrict__ accrank,
                                                    uint32_t *__restrict__ halfslot) {
    const Group &G = groups[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < G.naln; k += 64) halfslot[G.job0 + k] = 2u * (uint32_t)(G.hsp_begin + accrank[G.hsp_begin + k]);
}

// the halves of dense alignment d (an untraced half: no blocks; its group has failed) and block i of the two together
struct PathHalves { uint2 L, R; };
__device__ __forceinline__ PathHalves path_halves(const uint32_t *__restrict__ halfslot, const uint2 *__restrict__ pidx, uint32_t d) {
    const uint32_t hs = halfslot[d];
    PathHalves H{pidx[hs], pidx[hs + 1u]};
    if (H.L.x == PATH_UNTRACED) H.L = make_uint2(0u, 0u);
    if (H.R.x == PATH_UNTRACED) H.R = make_uint2(0u, 0u);
    return H;
}
__device__ __forceinline__ PathBlock path_block(const PathBlock *__restrict__ arena, const PathHalves &H, uint32_t i) {
    return i < H.L.y ? arena[H.L.x + i] : arena[H.R.x + (i - H.L.y)];
}
__device__ __forceinline__ bool path_continues(const PathBlock &a, const PathBlock &b) { return a.t + a.len == b.t && a.q + a.len == b.q; }

// count pass: one wavefront per alignment, lanes stride over its blocks; a block counts unless it continues the one before
constexpr int PATH_WAVES = 4;
__global__ __launch_bounds__(64 * PATH_WAVES) void k6_path_count(const uint32_t *__restrict__ halfslot, const uint2 *__restrict__ pidx,
                                                                 const PathBlock *__restrict__ arena, uint32_t ndense,
                                                                 uint32_t *__restrict__ cnt) {
    const uint32_t d = blockIdx.x * PATH_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (d >= ndense) return;   // wave-uniform
    const PathHalves H = path_halves(halfslot, pidx, d);
    const uint32_t n = H.L.y + H.R.y;
    uint32_t c = 0;
    for (uint32_t i = lane; i < n; i += 64u)
        if (i == 0 || !path_continues(path_block(arena, H, i - 1u), path_block(arena, H, i))) c++;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o);
    if (lane == 0) cnt[d] = c;
}
// write pass: alignment d's blocks at out[first[d] ..); the lane of a block that starts an output block adds up the blocks
// that continue it (at most the two at the anchor, as a half's own blocks never touch)
__global__ __launch_bounds__(64 * PATH_WAVES) void k6_path_write(const uint32_t *__restrict__ halfslot, const uint2 *__restrict__ pidx,
                                                                 const PathBlock *__restrict__ arena, uint32_t ndense,
                                                                 const unsigned long long *__restrict__ first,
                                                                 PathBlock *__restrict__ out) {
    const uint32_t d = blockIdx.x * PATH_WAVES + (threadIdx.x >> 6), lane = threadIdx.x & 63u;
    if (d >= ndense) return;   // wave-uniform
    const PathHalves H = path_halves(halfslot, pidx, d);
    const uint32_t n = H.L.y + H.R.y;
    PathBlock *dst = out + first[d];
    uint32_t run = 0;
    for (uint32_t i0 = 0; i0 < n; i0 += 64u) {
        const uint32_t i = i0 + lane;
        PathBlock b{0, 0, 0};
        bool start = false;
        if (i < n) {
            b = path_block(arena, H, i);
            start = i == 0 || !path_continues(path_block(arena, H, i - 1u), b);
        }
        const uint64_t ball = __ballot(start);
        if (start) {
            for (uint32_t j = i + 1u; j < n; j++) {
                const PathBlock nb = path_block(arena, H, j);
                if (!path_continues(b, nb)) break;
                b.len += nb.len;
            }
            dst[run + (uint32_t)__popcll(ball & ((1ull << lane) - 1ull))] = b;
        }
        run += (uint32_t)__popcll(ball);
    }
}

// after gapped_device(want_paths) and dense_alignments_device: the paths of the ndense dense alignments, in their order.
// first: ndense + 1 offsets into blocks
int dense_paths_device(const Group *d_groups, uint32_t ngroups, uint64_t ndense, DeviceBuf &first, DeviceBuf &blocks, uint64_t *nblocks) {
    hipStream_t st = stream();
    int rc;
    *nblocks = 0;
    if ((rc = first.reserve((size_t)(ndense + 1) * 8))) return rc;
    if (!ndense) { HIP_TRY(hipMemsetAsync(first.p, 0, 8, st)); return 0; }
    if (ndense >= (1ull << 32)) { set_error("paths: more than 2^32 alignments in one batch"); return MIMEO_ERR_LIMIT; }
    if ((rc = g_k6.pcnt.reserve((size_t)(ndense + 1) * 4)) || (rc = g_k6.pslot.reserve((size_t)ndense * 4))) return rc;
    HIP_TRY(hipMemsetAsync(g_k6.pcnt.p, 0, (size_t)(ndense + 1) * 4, st));
    const uint32_t nd = (uint32_t)ndense;
    const dim3 grid((nd + PATH_WAVES - 1) / PATH_WAVES), block(64 * PATH_WAVES);
    hipLaunchKernelGGL(k6_path_slots, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint32_t *)g_k6.accrank.p, (uint32_t *)g_k6.pslot.p);
    hipLaunchKernelGGL(k6_path_count, grid, block, 0, st, (const uint32_t *)g_k6.pslot.p, (const uint2 *)g_k6.pidx.p, (const PathBlock *)g_k6.arena.p, nd,
                       (uint32_t *)g_k6.pcnt.p);
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, (uint32_t *)g_k6.pcnt.p, (unsigned long long *)first.p, 0ull, (size_t)ndense + 1,
                                    rocprim::plus<unsigned long long>(), st));
    if ((rc = g_k6.ptmp.reserve(tb ? tb : 1))) return rc;
    HIP_TRY(rocprim::exclusive_scan(g_k6.ptmp.p, tb, (uint32_t *)g_k6.pcnt.p, (unsigned long long *)first.p, 0ull, (size_t)ndense + 1,
                                    rocprim::plus<unsigned long long>(), st));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, (const unsigned long long *)first.p + ndense, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *nblocks = total;
    if (!total) return 0;
    if ((rc = blocks.reserve((size_t)total * sizeof(PathBlock)))) return rc;
    hipLaunchKernelGGL(k6_path_write, grid, block, 0, st, (const uint32_t *)g_k6.pslot.p, (const uint2 *)g_k6.pidx.p, (const PathBlock *)g_k6.arena.p, nd,
                       (const unsigned long long *)first.p, (PathBlock *)blocks.p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// paths out under the box rule, after the last round: one trace pass over the two halves of every accepted alignment with
// score >= hspthresh (k6_kept_jobs), through the slices of trace_round; k6_trace<false>'s agreement check stays an error
int paths_pass(Group *d_groups, uint32_t ngroups, const mimeo_params *p, int32_t cap, const mimeo_alignment *d_aln, uint64_t budget, bool k6_stats) {
    hipStream_t st = stream();
    int rc;
    unsigned int *ctr = (unsigned int *)g_k6.cnt.p;
    HIP_TRY(hipMemsetAsync(g_k6.cnt.p, 0, 16, st));
    const dim3 grid((ngroups + 63) / 64), block(64);
    hipLaunchKernelGGL(k6_kept_jobs, grid, block, 0, st, (const Group *)d_groups, ngroups, d_aln, (const uint2 *)g_k6.anchors.p,
                       (const uint32_t *)g_k6.accrank.p, p->hspthresh, (DpJob *)nullptr, ctr);
    unsigned int njobs = 0;
    HIP_TRY(hipMemcpyAsync(&njobs, ctr, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!njobs) return 0;
    if ((rc = g_k6.kjobs.reserve((size_t)njobs * sizeof(DpJob)))) return rc;
    hipLaunchKernelGGL(k6_kept_jobs, grid, block, 0, st, (const Group *)d_groups, ngroups, d_aln, (const uint2 *)g_k6.anchors.p,
                       (const uint32_t *)g_k6.accrank.p, p->hspthresh, (DpJob *)g_k6.kjobs.p, ctr);
    TraceStats ts{};
    if ((rc = trace_round(d_groups, (const DpJob *)g_k6.kjobs.p, njobs, p, cap, budget, ts, false, BoundCtx{}))) return rc;
    if (k6_stats)
        fprintf(stderr, "[k6] paths out: traceback of %u halves %.3f ms, slices %u, %llu path blocks, pool %.1f MB, largest half %.3f MB\n", njobs, ts.ms,
                ts.slices, (unsigned long long)ts.arena_used, g_k6.pool.cap / 1048576.0, ts.largest / 1048576.0);
    return 0;
}

}  // namespace mimeo
