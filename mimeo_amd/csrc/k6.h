// K6, shared by its files (overview: k6_gapped.hip): the records that cross kernels, the DP kernels' cross-lane helpers, the bounds of a bounded
// extension, the stage's buffers.  No relocatable device code: a kernel is launched from the file that defines it, shared device code is here and in k6_band.h.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "device_util.h"

namespace mimeo {

constexpr int32_t NEG = -(1 << 30);
constexpr int32_t NEGH = -(1 << 29);

struct Cell {
    int32_t s;
    uint32_t nm, nx;
};
struct HalfResult {
    int32_t score;
    uint32_t i, j, nm, nx, overflow;
    uint32_t maxcols, rows;  // widest live band (columns from the window base) and rows evaluated: tuning statistics
    uint32_t base_lo, base_hi;  // k6_dp_any: what its rebased 32-bit cells stand above (score = base + score), 0 elsewhere
};
struct DpJob {
    uint32_t group, at, aq;
    int32_t dir;
    uint32_t slot, pad;  // index of this half's HalfResult: 2 * (hsp_begin + anchor rank) + side
};

// score of a half extension: the identical-suffix shortcut (rows == 0, i > 0) carries 64 bits
__device__ __forceinline__ int64_t half_score(const HalfResult &r) {
    return (r.rows == 0 && r.i > 0) ? (int64_t)(((uint64_t)r.maxcols << 32) | (uint32_t)r.score)
                                    : (int64_t)r.score + (int64_t)(((uint64_t)r.base_hi << 32) | r.base_lo);
}

__device__ __forceinline__ Cell cmax_left(const Cell &l, const Cell &r) { return r.s > l.s ? r : l; }  // ties -> left

// Cross-lane movement with DPP (VALU latency) instead of ds_bpermute (LDS-crossbar latency): the DP
// keeps rank == lane, so every scan / neighbour access is a fixed lane pattern.
// gfx9 DPP controls: row_shr:n = 0x110+n, wave_shr:1 = 0x138, row_bcast:15 = 0x142, row_bcast:31 = 0x143.
template <int CTRL, int RMASK>
__device__ __forceinline__ Cell dpp_cell(const Cell &c) {
    Cell o;  // lanes without a valid source keep the identity (NEG, 0, 0)
    o.s = __builtin_amdgcn_update_dpp(NEG, c.s, CTRL, RMASK, 0xf, false);
    o.nm = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.nm, CTRL, RMASK, 0xf, false);
    o.nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.nx, CTRL, RMASK, 0xf, false);
    return o;
}
// inclusive max-scan over the 64 lanes, ties to the lower lane
__device__ __forceinline__ Cell wave_incl_maxscan(Cell v) {
    v = cmax_left(dpp_cell<0x111, 0xf>(v), v);
    v = cmax_left(dpp_cell<0x112, 0xf>(v), v);
    v = cmax_left(dpp_cell<0x114, 0xf>(v), v);
    v = cmax_left(dpp_cell<0x118, 0xf>(v), v);
    v = cmax_left(dpp_cell<0x142, 0xa>(v), v);
    v = cmax_left(dpp_cell<0x143, 0xc>(v), v);
    return v;
}
struct Best4 {
    int32_t s;
    uint32_t j, nm, nx;
};
template <int CTRL, int RMASK>
__device__ __forceinline__ Best4 dpp_best(const Best4 &c) {
    Best4 o;
    o.s = __builtin_amdgcn_update_dpp(NEG, c.s, CTRL, RMASK, 0xf, false);
    o.j = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.j, CTRL, RMASK, 0xf, false);
    o.nm = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.nm, CTRL, RMASK, 0xf, false);
    o.nx = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.nx, CTRL, RMASK, 0xf, false);
    return o;
}
__device__ __forceinline__ Best4 bmax_left(const Best4 &l, const Best4 &r) { return r.s > l.s ? r : l; }
// row maximum with the smallest column on ties: columns grow with the lane, so "ties to the lower
// lane" is "smallest column"; the total ends up in lane 63
__device__ __forceinline__ Best4 wave_best(Best4 v) {
    v = bmax_left(dpp_best<0x111, 0xf>(v), v);
    v = bmax_left(dpp_best<0x112, 0xf>(v), v);
    v = bmax_left(dpp_best<0x114, 0xf>(v), v);
    v = bmax_left(dpp_best<0x118, 0xf>(v), v);
    v = bmax_left(dpp_best<0x142, 0xa>(v), v);
    v = bmax_left(dpp_best<0x143, 0xc>(v), v);
    Best4 t;
    t.s = __builtin_amdgcn_readlane(v.s, 63); t.j = (uint32_t)__builtin_amdgcn_readlane((int)v.j, 63);
    t.nm = (uint32_t)__builtin_amdgcn_readlane((int)v.nm, 63); t.nx = (uint32_t)__builtin_amdgcn_readlane((int)v.nx, 63);
    return t;
}

struct PathBlock {
    uint32_t t, q, len;
};
static_assert(sizeof(PathBlock) == sizeof(mimeo_path_block), "PathBlock is what mimeo_align_units_paths hands out");
constexpr uint32_t PATH_UNTRACED = 0xFFFFFFFFu;  // pidx[slot].x of a half whose traceback did not fit the trace pool
struct PathView {
    const uint2 *pidx;       // per half slot (as HalfResult): first block in blk, block count
    const PathBlock *blk;    // block arena of the call
    uint32_t *accrank;       // per alignment slot hsp_begin + e: rank of its anchor (written by k6_resolve)
};

// the blocks of a half are sorted by t: how many start at or below t (the last of them is the one that may hold t)
template <class TT>
__device__ __forceinline__ uint32_t blocks_upto(const PathBlock *blk, uint32_t n, TT t) {
    uint32_t lo = 0, hi = n;   // first block that starts above t
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((TT)blk[mid].t <= t) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// ---- bounds (mimeo_params.bound_extensions; path rule only) -------------------------------------------------------------
// A half extension of an anchor (at, aq) is bounded by the diagonal steps of the alignments accepted so far in its group
// (alignment specification v1, rule 7): with d0 = aq - at and, for the target base t of DP row i, dL / dR the nearest
// earlier diagonals q - t at or below / at or above d0, cell (i, j) lives only if dL < q_j - t < dR.  In the DP's own
// diagonal index k = j - i that is an open interval (kmin, kmax), piecewise constant in i: it changes only where a block
// of an earlier path starts or ends.  The DP kernels carry the interval and the next row where it may change as
// wave-uniform scalars and ask bounds_at() again when they get there: one lane per accepted alignment whose box holds
// the row, one binary search in that alignment's blocks.  Nothing is precomputed, so rows a half never reaches cost nothing.
struct BoundCtx {
    const mimeo_alignment *aln;   // the alignments of group g at aln[hsp_begin .. + nacc), strand coordinates
    const uint2 *anchors;
    PathView P;
};
constexpr long long K_INF = 1ll << 40;   // beyond every diagonal difference
struct RowBound {
    long long kmin, kmax;   // cell (i, j) is allowed iff kmin < j - i < kmax
    uint32_t next;          // first row above i where the interval may differ
    uint32_t any;           // some earlier path has a diagonal step in row i
};
struct HalfSweep {   // what a bounded half extension looked at (k6_resolve: is the result still valid?)
    int32_t klo, khi;    // smallest / largest k = j - i of a live cell in rows >= 1 (strip granularity in k6_dp1: a superset)
    uint32_t nacc;       // alignments of the group it was bounded by (the group's nacc when its DP ran)
    uint32_t nbound;     // rows in which an earlier path set a bound
};
__device__ __forceinline__ long long wave_uniform_ll(long long v) {
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(unsigned long long)v);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)((unsigned long long)v >> 32));
    return (long long)(((unsigned long long)hi << 32) | lo);
}
// wave-cooperative; every lane returns the same.  Row i >= 1 of the half (at, aq, dir); i is at most the half's target length.
__device__ __forceinline__ RowBound bounds_at(const BoundCtx &B, uint64_t b0, uint32_t nacc, uint32_t at, uint32_t aq, int dir, uint32_t i) {
    const long long t = dir > 0 ? (long long)at + i - 1 : (long long)at - i;
    const long long d0 = (long long)aq - (long long)at;
    long long kmin = -K_INF, kmax = K_INF;
    long long nt = dir > 0 ? K_INF : -1;   // next target base, in the direction of travel, where a block starts or ends
    for (uint32_t e = threadIdx.x & 63u; e < nacc; e += 64u) {
        const mimeo_alignment o = B.aln[b0 + e];
        long long c;
        if (t >= (long long)o.tstart && t < (long long)o.tend) {
            const uint32_t rank = B.P.accrank[b0 + e];
            const uint2 an = B.anchors[b0 + rank];
            const uint32_t side = t >= (long long)an.x ? 1u : 0u;
            const uint2 ix = B.P.pidx[2u * (b0 + rank) + side];
            const bool traced = ix.x != PATH_UNTRACED;
            const uint32_t n = traced ? ix.y : 0u;
            const PathBlock *blk = B.P.blk + (traced ? ix.x : 0u);
            const uint32_t lo = blocks_upto(blk, n, t);
            PathBlock b{0, 0, 0};
            if (lo) b = blk[lo - 1];
            if (lo && t - (long long)b.t < (long long)b.len) {   // the row holds a diagonal step of this alignment
                const long long d = (long long)b.q - (long long)b.t, k = dir > 0 ? d - d0 : d0 - d;
                if (k <= 0) kmin = max(kmin, k);
                if (k >= 0) kmax = min(kmax, k);
                c = dir > 0 ? (long long)b.t + b.len : (long long)b.t - 1;
            } else if (dir > 0) {
                c = lo < n ? (long long)blk[lo].t : (side == 0 ? (long long)an.x : (long long)o.tend);
            } else {
                c = lo ? (long long)b.t + b.len - 1 : (side == 1 ? (long long)an.x - 1 : (long long)o.tstart - 1);
            }
        } else if (dir > 0) {
            c = (long long)o.tstart > t ? (long long)o.tstart : K_INF;
        } else {
            c = (long long)o.tend <= t ? (long long)o.tend - 1 : -1;
        }
        nt = dir > 0 ? min(nt, c) : max(nt, c);
    }
    for (int o = 32; o > 0; o >>= 1) {
        kmin = max(kmin, __shfl_xor(kmin, o));
        kmax = min(kmax, __shfl_xor(kmax, o));
        const long long on = __shfl_xor(nt, o);
        nt = dir > 0 ? min(nt, on) : max(nt, on);
    }
    RowBound r;
    r.kmin = wave_uniform_ll(kmin); r.kmax = wave_uniform_ll(kmax);
    nt = wave_uniform_ll(nt);
    const long long nrow = dir > 0 ? nt - (long long)at + 1 : (long long)at - nt;   // the row that consumes target base nt
    r.next = nrow > 0xFFFFFFFEll ? 0xFFFFFFFFu : (uint32_t)nrow;
    r.any = (r.kmin > -K_INF || r.kmax < K_INF) ? 1u : 0u;
    return r;
}
// may a bounded half take the identical-suffix shortcut?  Only when no accepted alignment reaches into its rows
__device__ __forceinline__ bool bounds_none(const BoundCtx &B, uint64_t b0, uint32_t nacc, uint32_t at, int dir) {
    bool hit = false;
    for (uint32_t e = threadIdx.x & 63u; e < nacc; e += 64u) {
        const mimeo_alignment o = B.aln[b0 + e];
        if (o.tend > o.tstart && (dir > 0 ? o.tend > at : o.tstart < at)) hit = true;
    }
    return __ballot(hit) == 0;
}

// ---- host side: the stage's device buffers, grown on demand and kept between calls; the functions that cross files
struct K6Buffers {
    DeviceBuf anchors, packed, jobs, res, cnt, astate, ovf_list, any;
    // path rule: per half slot (first block, count), per alignment slot the anchor's rank, the block arena, the trace pool
    DeviceBuf pidx, accrank, arena, pool, tjobs, tres, tctr;
    DeviceBuf kjobs, pcnt, pslot, ptmp;   // paths out: jobs of the box rule's trace pass; block counts, half slots, scan scratch
    DeviceBuf sweep;   // bounded extensions: per half slot what its DP swept (HalfSweep)
};
extern K6Buffers g_k6;   // k6_gapped.hip
// cap: the score beyond which 32-bit DP cells are rebased.  dp_round: k6_dp.hip; arena_reserve, trace_round: k6_trace.hip; paths_pass: k6_paths.hip
int dp_round(Group *d_groups, uint32_t n, const mimeo_params *p, int32_t cap, bool bounded, const BoundCtx &bc, unsigned int *novf, unsigned int *nrestart);
int arena_reserve(uint64_t blocks, uint64_t used);
struct TraceStats { uint64_t arena_used, largest; float ms; uint32_t slices; };   // blocks in the arena, largest traceback of one half (bytes), kernel time, pool slices
int trace_round(Group *d_groups, const DpJob *d_jobs, uint32_t h0, const mimeo_params *p, int32_t cap, uint64_t budget, TraceStats &ts, bool bounded, BoundCtx bc);
int paths_pass(Group *d_groups, uint32_t ngroups, const mimeo_params *p, int32_t cap, const mimeo_alignment *d_aln, uint64_t budget, bool k6_stats);

}  // namespace mimeo
