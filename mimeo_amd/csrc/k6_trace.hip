#include "k6_band.h"

namespace mimeo {

// ---- K6: traceback of a half extension (k6_trace, its pool slices and the block arena: trace_round; overview in k6_gapped.hip) ----
// Re-runs one half's DP over rows 1 .. i* (row r depends only on the rows above it, so they are the rows of the first
// run) with the row loop of k6_dp_any (band_dp, k6_band.h: the same recurrences, pruning, tie-breaks and rebase, in one
// text), storing one traceback byte per computed cell, checks the
// re-run against its HalfResult (best score and cell; matches / mismatches along the walked path) and walks back from
// the best cell into gap-free blocks.  Traceback bits and the walk are those of the study oracle (box_vs_path.c):
//   TB_HD     H took D (strictly better than the diagonal)      TB_CI     C took I (strictly better than H)
//   TB_DOPEN  D opened from C of the row above                  TB_IOPEN  I opened from H of the column to the left
// One workgroup of 256 threads per half; the two DP rows (scores only: counts come from the walk) live in LDS when the
// band bound fits TR_LDS_COLS, else in a ring in the job's slice of the trace pool.  Pool slice of a job (trace_layout):
// traceback bytes (row r at (r - 1) * W, column j at j - row_lo[r]) | row_lo[1 .. i*] | block scratch | ring.
enum : uint8_t { TB_HD = 1, TB_CI = 2, TB_DOPEN = 4, TB_IOPEN = 8 };
constexpr int TR_THREADS = 256;
constexpr uint32_t TR_LDS_COLS = 2048;
enum : uint32_t { TR_NONE = 0, TR_DIAG = 1, TR_DP = 2, TR_UNTRACED = 3 };
struct TraceJob {
    unsigned long long off;  // byte offset of the job's slice in the pool
    uint32_t W, R;           // columns per traceback row (bound of every row's band); ring columns (power of two)
    uint32_t mode, cap;      // TR_*; block capacity of the scratch
};
struct TraceLayout { unsigned long long rowlo, blk, ring, total; };
__host__ __device__ inline unsigned long long tr_align(unsigned long long x) { return (x + 255ull) & ~255ull; }
__host__ __device__ inline TraceLayout trace_layout(uint32_t rows, uint32_t W, uint32_t R, uint32_t cap) {
    TraceLayout L;
    L.rowlo = tr_align((unsigned long long)rows * W);
    L.blk = L.rowlo + tr_align(4ull * (rows + 1ull));
    L.ring = L.blk + tr_align(12ull * cap);
    L.total = L.ring + (R > TR_LDS_COLS ? tr_align(16ull * R) : 0ull);
    return L;
}
// errors of the trace (ctr[1]): the re-run or the walk disagrees with the first run; ctr[2] = the half's slot
enum : uint32_t { TRERR_DP = 1, TRERR_WALK = 2, TRERR_ROOM = 3 };

// band_dp's payload: scores only in the two rows; one traceback byte per cell, the scan carries the column an insertion opened at
struct TraceRows {
    int32_t *ring;       // C, D of one row, C, D of the other: R columns each
    uint32_t R, M, W;    // ring columns, R - 1, columns of a traceback row
    uint32_t *rowlo;
    uint8_t *tb, *trow;  // trow: the row's traceback bytes, indexed by column
    __device__ __forceinline__ BandRows rows(uint32_t par, uint32_t i, uint32_t lo) {
        trow = tb + (size_t)(i - 1u) * W - lo;
        if (threadIdx.x == 0) rowlo[i] = lo;
        int32_t *p = ring + 2u * R * par, *n = ring + 2u * R * (par ^ 1u);
        return BandRows{p, p + R, n, n + R};
    }
    __device__ __forceinline__ void init(uint32_t j, int32_t c) { ring[j & M] = c; ring[R + (j & M)] = NEG; }
    __device__ __forceinline__ Cell h(uint32_t j, bool, bool dopen, bool, bool, bool hd) const { trow[j] = (dopen ? TB_DOPEN : 0) | (hd ? TB_HD : 0); return Cell{0, j, 0}; }
    __device__ __forceinline__ Cell htag(uint32_t j) const { return Cell{0, j, 0}; }
    __device__ __forceinline__ Cell c(uint32_t j, const Cell &, const Cell &ia, bool ci) const {
        trow[j] |= ((ia.s > NEGH && ia.nm + 1u == j) ? TB_IOPEN : 0) | (ci ? TB_CI : 0);   // I(j) opened from H(j - 1)
        return Cell{0, 0, 0};
    }
};

// BOUND: the re-run is bounded as the first run was (the group's nacc has not moved since: same round, before k6_resolve)
template <bool BOUND>
__global__ __launch_bounds__(TR_THREADS) void k6_trace(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                       const TraceJob *__restrict__ tjobs, uint32_t k0,
                                                       const HalfResult *__restrict__ res, uint8_t *__restrict__ pool,
                                                       PathBlock *__restrict__ arena, unsigned long long arena_cap,
                                                       uint2 *__restrict__ pidx, unsigned int *__restrict__ ctr,
                                                       int32_t O, int32_t E, int32_t Y, int32_t cap, BoundCtx B) {
    __shared__ int32_t s_ring[4 * TR_LDS_COLS];
    __shared__ uint32_t s_nb, s_off, s_bad;
    const uint32_t k = k0 + blockIdx.x;
    const DpJob job = jobs[k];
    const TraceJob J = tjobs[k];
    const HalfResult hr = res[job.slot];
    const Group &G = groups[job.group];
    const GStrandView T = G.T, Q = G.Q;
    const uint32_t at = job.at, aq = job.aq;
    const int dir = job.dir;
    const uint32_t tid = threadIdx.x;
    if (J.mode != TR_DP) {
        if (tid == 0) {
            uint2 ix = make_uint2(0u, 0u);
            if (J.mode == TR_UNTRACED) ix.x = PATH_UNTRACED;
            if (J.mode == TR_DIAG) {   // identical-suffix shortcut: the diagonal of its length
                const unsigned int o = atomicAdd(&ctr[0], 1u);
                if (o >= arena_cap) { ctr[1] = TRERR_ROOM; ctr[2] = job.slot; }
                else {
                    const uint32_t n = hr.i;
                    arena[o] = dir > 0 ? PathBlock{at, aq, n} : PathBlock{at - n, aq - n, n};
                    ix = make_uint2(o, 1u);
                }
            }
            pidx[job.slot] = ix;
        }
        return;
    }
    const uint32_t W = J.W, M = J.R - 1u;
    const TraceLayout Lay = trace_layout(hr.i, W, J.R, J.cap);
    uint8_t *tb = pool + J.off;
    uint32_t *rowlo = (uint32_t *)(pool + J.off + Lay.rowlo);
    PathBlock *scratch = (PathBlock *)(pool + J.off + Lay.blk);
    if (tid == 0) s_bad = 0;
    TraceRows rows{J.R <= TR_LDS_COLS ? s_ring : (int32_t *)(pool + J.off + Lay.ring), J.R, M, W, rowlo, tb};
    // the re-run ends at the row of the first run's best cell: a row without a live cell before it leaves the best cell short of it
    HalfSweep sw;   // what k6_dp_any hands to k6_resolve: computed under BOUND and dropped here (no register more than the parent)
    const HalfResult r = band_dp<TR_THREADS, BOUND>(rows, G, job, hr.i, O, E, Y, cap, B, sw);
    if (tid == 0 && (r.overflow || r.i != hr.i || r.j != hr.j || half_score(r) != half_score(hr))) { ctr[1] = TRERR_DP; ctr[2] = job.slot; s_bad = 1; }
    __syncthreads();
    if (s_bad) { if (tid == 0) pidx[job.slot] = make_uint2(0u, 0u); return; }
    // walk back from the best cell (one lane); states 0 = C, 1 = H, 2 = D, 3 = I
    if (tid == 0) {
        uint32_t i = hr.i, j = hr.j, nm = 0, nx = 0, nb = 0, st = 0, bt = 0, bq = 0, bl = 0, pt = 0;
        bool ok = true;
        unsigned long long guard = 3ull * ((unsigned long long)i + j) + 3ull;
        while ((i || j) && ok) {
            if (!guard--) { ok = false; break; }
            if (i == 0) { j--; continue; }   // row 0: an insertion chain back to the origin
            const uint32_t rl = rowlo[i];
            if (j < rl || j - rl >= W) { ok = false; break; }
            const uint8_t b = tb[(size_t)(i - 1u) * W + (j - rl)];
            if (st == 0) st = (b & TB_CI) ? 3u : 1u;
            else if (st == 1) {
                if (b & TB_HD) st = 2;
                else {
                    const uint32_t t = dir > 0 ? at + i - 1u : at - i, q = dir > 0 ? aq + j - 1u : aq - j;
                    const Base1 x = base_at(T, (int32_t)t), y = base_at(Q, (int32_t)q);
                    if (!((x.lo ^ y.lo) | (x.hi ^ y.hi) | x.nm | y.nm)) nm++; else nx++;
                    // the diagonal steps of a half come in t order (descending for dir > 0): extend the block or start one
                    if (bl && (dir > 0 ? t + 1u == pt : t == pt + 1u) && (int32_t)(t - q) == (int32_t)(bt - bq)) {
                        bl++;
                        if (dir > 0) { bt = t; bq = q; }
                    } else {
                        if (bl) { if (nb >= J.cap) { ok = false; break; } scratch[nb++] = PathBlock{bt, bq, bl}; }
                        bt = t; bq = q; bl = 1;
                    }
                    pt = t;
                    i--; j--; st = 0;
                }
            } else if (st == 2) { st = (b & TB_DOPEN) ? 0u : 2u; i--; }
            else { st = (b & TB_IOPEN) ? 1u : 3u; j--; }
        }
        if (ok && bl) { if (nb >= J.cap) ok = false; else scratch[nb++] = PathBlock{bt, bq, bl}; }
        if (!ok || nm != hr.nm || nx != hr.nx) { ctr[1] = TRERR_WALK; ctr[2] = job.slot; nb = 0; ok = false; }
        if (ok && dir > 0)   // sorted by t
            for (uint32_t a = 0, z = nb ? nb - 1u : 0u; a < z; a++, z--) { const PathBlock t = scratch[a]; scratch[a] = scratch[z]; scratch[z] = t; }
        unsigned int o = 0;
        if (nb) {
            o = atomicAdd(&ctr[0], nb);
            if (o + (unsigned long long)nb > arena_cap) { ctr[1] = TRERR_ROOM; ctr[2] = job.slot; nb = 0; }
        }
        s_nb = nb; s_off = o;
        pidx[job.slot] = make_uint2(nb ? o : 0u, nb);
    }
    __syncthreads();
    for (uint32_t e = tid; e < s_nb; e += TR_THREADS) arena[s_off + e] = scratch[e];
}

// the HalfResults of a round's jobs, in job order (read back to plan the traceback slices)
__global__ void k6_trace_gather(const DpJob *__restrict__ jobs, uint32_t n, const HalfResult *__restrict__ res,
                                HalfResult *__restrict__ out) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) out[k] = res[jobs[k].slot];
}

// the block arena grows with its contents (block offsets stay valid)
int arena_reserve(uint64_t blocks, uint64_t used) {
    const size_t bytes = (size_t)blocks * sizeof(PathBlock);
    if (bytes <= g_k6.arena.cap) return 0;
    DeviceBuf nb;
    int rc = nb.reserve(std::max(bytes, 2 * g_k6.arena.cap));
    if (rc) return rc;
    if (used) HIP_TRY(hipMemcpyAsync(nb.p, g_k6.arena.p, (size_t)used * sizeof(PathBlock), hipMemcpyDeviceToDevice, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    g_k6.arena.release();
    g_k6.arena = nb;
    return 0;
}

// path rule, after the DP kernels of a round: the traceback of every half of the h0 jobs in d_jobs (the round's; under the box
// rule with paths asked for, the halves of the alignments that are returned: paths_pass), in slices of jobs whose
// tracebacks fit the pool together.  A half whose traceback alone exceeds the pool gets no path (PATH_UNTRACED): k6_resolve
// fails its group if the anchor is accepted, as for a band beyond the DP limit.
int trace_round(Group *d_groups, const DpJob *d_jobs, uint32_t h0, const mimeo_params *p, int32_t cap, uint64_t budget, TraceStats &ts, bool bounded, BoundCtx bc) {
    hipStream_t st = stream();
    int rc;
    if ((rc = g_k6.tres.reserve((size_t)h0 * sizeof(HalfResult)))) return rc;
    hipLaunchKernelGGL(k6_trace_gather, dim3((h0 + 255) / 256), dim3(256), 0, st, d_jobs, h0, (const HalfResult *)g_k6.res.p,
                       (HalfResult *)g_k6.tres.p);
    std::vector<HalfResult> hr(h0);
    HIP_TRY(hipMemcpyAsync(hr.data(), g_k6.tres.p, (size_t)h0 * sizeof(HalfResult), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int32_t O = p->gap_open, E = p->gap_extend, Y = p->ydrop;
    const uint32_t ext = (uint32_t)((Y + 200) / E) + 2u, hi0 = Y >= O + E ? (uint32_t)((Y - O) / E) : 0u;
    std::vector<TraceJob> tj(h0);
    std::vector<uint32_t> cut{0};   // slice boundaries
    uint64_t fill = 0, need_max = 0, blocks = 0;
    for (uint32_t k = 0; k < h0; k++) {
        const HalfResult &r = hr[k];
        TraceJob J{0, 0, 0, TR_NONE, 0};
        if (!r.overflow && r.i) {
            if (r.rows == 0) { J.mode = TR_DIAG; blocks += 1; }
            else {
                J.W = std::max(r.maxcols, hi0 + 1u) + ext + 2u;
                J.R = 1u;
                while (J.R < J.W + 2u) J.R <<= 1;
                J.cap = std::min(r.i, r.j) + 1u;
                const uint64_t need = trace_layout(r.i, J.W, J.R, J.cap).total;
                ts.largest = std::max(ts.largest, need);
                if (need > budget) J.mode = TR_UNTRACED;
                else {
                    J.mode = TR_DP;
                    blocks += J.cap;
                    if (fill + need > budget) { cut.push_back(k); fill = 0; }
                    J.off = fill;
                    fill += need;
                    need_max = std::max(need_max, fill);
                }
            }
        }
        tj[k] = J;
    }
    cut.push_back(h0);
    if ((rc = g_k6.tjobs.reserve((size_t)h0 * sizeof(TraceJob)))) return rc;
    HIP_TRY(hipMemcpyAsync(g_k6.tjobs.p, tj.data(), (size_t)h0 * sizeof(TraceJob), hipMemcpyHostToDevice, st));
    if (need_max && (rc = g_k6.pool.reserve(need_max))) return rc;
    if ((rc = arena_reserve(ts.arena_used + blocks + 1, ts.arena_used))) return rc;
    static hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!e0) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); }
    HIP_TRY(hipEventRecord(e0, st));
    bc.P.blk = (const PathBlock *)g_k6.arena.p;   // the arena may just have grown
    const auto trace = bounded ? k6_trace<true> : k6_trace<false>;
    for (size_t c = 0; c + 1 < cut.size(); c++)
        if (cut[c + 1] > cut[c] && ++ts.slices)
            hipLaunchKernelGGL(trace, dim3(cut[c + 1] - cut[c]), dim3(TR_THREADS), 0, st, (const Group *)d_groups,
                               d_jobs, (const TraceJob *)g_k6.tjobs.p, cut[c], (const HalfResult *)g_k6.res.p,
                               (uint8_t *)g_k6.pool.p, (PathBlock *)g_k6.arena.p, (unsigned long long)(g_k6.arena.cap / sizeof(PathBlock)),
                               (uint2 *)g_k6.pidx.p, (unsigned int *)g_k6.tctr.p, O, E, Y, cap, bc);
    HIP_TRY(hipEventRecord(e1, st));
    unsigned int c3[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(c3, g_k6.tctr.p, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    ts.ms += t;
    if (c3[1]) {
        char msg[200];
        snprintf(msg, sizeof msg, "internal: K6 traceback of half slot %u %s", c3[2],
                 c3[1] == TRERR_DP ? "disagrees with its DP result (score or end cell)"
                 : c3[1] == TRERR_WALK ? "disagrees with its DP result (matches / mismatches along the path)" : "outgrew the block arena");
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    ts.arena_used = c3[0];
    return 0;
}

}  // namespace mimeo
