// K5 (overview: k5_chain.hip) — wave chain DP for large groups: the predecessor query answered from a Fenwick tree (maximum) over
// the group's HSPs ranked by query end, into which an HSP is put once the sweep over the target has passed its end.  DESIGN.md §4
// K5 "Large groups" has the algorithm (waves, tiles, the window) and its measurements.  Names used below: E = the HSPs ordered by
// target end; tcnt[k] / qcnt[k] = how many target / query ends are <= tstart[k] / qstart[k]; qpos[i] = rank of i by query end; a
// step takes the HSPs [a, b), and E[.. tcnt[a]) are in the tree before it.  Tree nodes and candidates are (chain score << 24 |
// 2^24-1 - member): a chain scores less than 100 * 2^32 < 2^39 (its HSPs do not overlap).
#include <vector>

#include "k5.h"

namespace mimeo {

// The instruction scheduler moves nothing across.  Eight of them cut a step of k5_chain_wave where the development clocks stood
// until they were removed: without the cuts the step was 1 % slower, with four of the eight as well (profiles/r22_ab_k5.json).
#define CW_REGION_END() __builtin_amdgcn_sched_barrier(0)
struct WaveStep { uint32_t tcnt, end; };   // end: bit 31 = a wave (no member precedes another)
constexpr uint32_t CW_THREADS = 512, CW_PURE = 0x80000000u;

__global__ void k5w_end_keys(const mimeo_hsp *__restrict__ hs, const uint64_t *__restrict__ gkey, uint64_t n, int query, uint64_t *__restrict__ key,
                             uint32_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const mimeo_hsp &h = hs[i];
    key[i] = (gkey[i] & 0xFFFFFFFF00000000ull) | (uint64_t)((query ? h.qstart : h.tstart) + h.length);
    val[i] = (uint32_t)i;
}
// per HSP of a large group: its rank by query end (from the sorted order), the two counts and the step that begins at it
__global__ void k5w_prepare(const Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs, const uint64_t *__restrict__ gkey,
                            const uint64_t *__restrict__ kte, const uint64_t *__restrict__ kqe, const uint32_t *__restrict__ vq, uint64_t n,
                            uint32_t big_min, uint32_t *__restrict__ qpos, uint32_t *__restrict__ qcnt, WaveStep *__restrict__ step) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    {   // i as a position of the query-end order
        const Group &G = groups[kqe[i] >> 32];
        if (G.hsp_end - G.hsp_begin > big_min) qpos[vq[i]] = (uint32_t)(i - G.hsp_begin) + 1u;
    }
    const uint64_t gk = gkey[i] & 0xFFFFFFFF00000000ull;
    const Group &G = groups[gk >> 32];
    const uint64_t b0 = G.hsp_begin, e0 = G.hsp_end;
    const uint32_t ng = (uint32_t)(e0 - b0), a = (uint32_t)(i - b0);
    if (ng <= big_min) return;
    const mimeo_hsp &h = hs[i];
    const uint32_t tc = (uint32_t)(bisect(kte, b0, e0, gk | h.tstart, true) - b0);   // < ng: the HSP itself ends behind its start
    qcnt[i] = (uint32_t)(bisect(kqe, b0, e0, gk | h.qstart, true) - b0);
    const uint64_t next_end = gk | (uint32_t)kte[b0 + tc];
    const uint32_t wave_end = (uint32_t)(bisect(gkey, i, e0, next_end, false) - b0);   // first HSP that starts at or behind that end
    const uint32_t tile_end = min(a + (uint32_t)CH_TILE, ng);
    step[i] = WaveStep{tc, wave_end >= tile_end ? (wave_end | CW_PURE) : tile_end};
}

// development statistics (MIMEO_K5_STATS): one thread per large group walks its steps
constexpr int CW_STATS = 7;
__global__ void k5w_stats(const Group *__restrict__ groups, const uint32_t *__restrict__ list, uint32_t nlist, const WaveStep *__restrict__ step,
                          unsigned long long *__restrict__ out) {
    const uint32_t li = blockIdx.x * blockDim.x + threadIdx.x;
    if (li >= nlist) return;
    const Group &G = groups[list[li]];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t n = (uint32_t)(G.hsp_end - G.hsp_begin);
    unsigned long long tiles = 0, waves = 0, wave_members = 0, window = 0, chunks = 0, maxwin = 0;
    uint32_t a = 0, c = 0;
    while (a < n) {
        const WaveStep s = step[b0 + a];
        const uint32_t b = s.end & ~CW_PURE;
        if (s.end & CW_PURE) { waves++; wave_members += b - a; }
        else {
            tiles++;
            const uint32_t w = step[b0 + b - 1].tcnt - c;
            window += w; chunks += (w + 63) / 64; maxwin = w > maxwin ? w : maxwin;
        }
        c = s.tcnt; a = b;
    }
    unsigned long long *o = out + (size_t)li * CW_STATS;
    o[0] = n; o[1] = tiles; o[2] = waves; o[3] = wave_members; o[4] = window; o[5] = chunks; o[6] = maxwin;
}

__device__ __forceinline__ unsigned long long cw_pack(long long best, uint32_t member) {   // 0 = no predecessor (only a positive chain is one)
    return best > 0 ? (((unsigned long long)best << 24) | (unsigned long long)(CW_MAX - 1u - member)) : 0ull;
}
// The tree: ranks in blocks of 2^bshift (1024 at least, 4096 blocks at most); inside a block a Fenwick tree (maximum) in global
// memory, changed by L2 atomics, over the blocks one in LDS.  Query = prefix maximum over the first cnt ranks: CW_BITS plain loads
// whatever cnt is, all issued before the first is waited for; the caller invalidates the vector L1 behind the barrier that ends a step.
constexpr int CW_BITS = 12;
constexpr uint32_t CW_BLOCKS = 4096;
struct WaveTree {
    unsigned long long *fen;    // the group's nodes: block j at fen[j << bshift ..]
    unsigned long long *blk;    // LDS: node j (1-based) at blk[j - 1]
    uint32_t n, bshift, nblk;
};
struct WaveQuery { unsigned long long v[CW_BITS], w[CW_BITS]; };
__device__ __forceinline__ void cw_query_issue(const WaveTree &T, uint32_t cnt, WaveQuery &Q) {
    const uint32_t q = cnt >> T.bshift, base = q << T.bshift;
    uint32_t x = cnt - base, j = q;
#pragma unroll
    for (int it = 0; it < CW_BITS; it++) {   // straight-line code: the loads in flight together
        const unsigned long long ld = T.fen[x ? base + x - 1u : 0u];
        Q.v[it] = x ? ld : 0ull;
        x &= x - 1u;
    }
#pragma unroll
    for (int it = 0; it < CW_BITS; it++) {
        const unsigned long long ld = T.blk[j ? j - 1u : 0u];
        Q.w[it] = j ? ld : 0ull;
        j &= j - 1u;
    }
}
__device__ __forceinline__ unsigned long long cw_query_reduce(WaveQuery &Q) {
#pragma unroll
    for (int it = 0; it < CW_BITS; it++) Q.v[it] = Q.w[it] > Q.v[it] ? Q.w[it] : Q.v[it];
#pragma unroll
    for (int st = 1; st < CW_BITS; st <<= 1)
#pragma unroll
        for (int it = 0; it + st < CW_BITS; it += 2 * st) Q.v[it] = Q.v[it + st] > Q.v[it] ? Q.v[it + st] : Q.v[it];
    return Q.v[0];
}
__device__ __forceinline__ void cw_insert(const WaveTree &T, uint32_t pos, unsigned long long v) {   // pos: rank, 1-based
    if (!v) return;
    const uint32_t r0 = pos - 1u, b = r0 >> T.bshift, base = b << T.bshift, bsz = 1u << T.bshift;
    for (uint32_t x = (r0 - base) + 1u; x <= bsz && base + x <= T.n; x += x & (0u - x))
        __hip_atomic_fetch_max(T.fen + (base + x - 1u), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    for (uint32_t j = b + 1u; j <= T.nblk; j += j & (0u - j))
        __hip_atomic_fetch_max(T.blk + (j - 1u), v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}
__device__ __forceinline__ unsigned long long readlane64(unsigned long long v, int lane) {   // lane: wave-uniform
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane), hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((unsigned long long)hi << 32) | lo;
}

// the HSPs in target-end order, as the sweep needs them: (target end, query end, rank by query end); their chain values
// (packed with the member, 0 = not final yet) lie beside them in the same order, written when a member is finalised, so
// that the window and the insertions read two sequential streams
__global__ void k5w_end_records(const Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs, const uint64_t *__restrict__ kte, const uint32_t *__restrict__ E,
                                const uint32_t *__restrict__ qpos, uint64_t n, uint32_t big_min, uint4 *__restrict__ erec, uint32_t *__restrict__ epos) {
    const uint64_t x = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (x >= n) return;
    const Group &G = groups[kte[x] >> 32];
    if (G.hsp_end - G.hsp_begin <= big_min) return;
    const uint32_t i = E[x];
    const mimeo_hsp &h = hs[i];
    erec[x] = make_uint4((uint32_t)kte[x], h.qstart + h.length, qpos[i], 0u);
    epos[i] = (uint32_t)x;
}

// the members of a tile as every wavefront keeps them in its registers (lane = member), fetched a step ahead: a step calls fetch for
// the tile behind it early, but behind the loads it waits for itself (loads return in order)
struct TileAhead {
    mimeo_hsp h;
    uint32_t q = 0, c = 0, e = 0;   // qcnt, tcnt, position in the target-end order
    __device__ __forceinline__ void fetch(const mimeo_hsp *__restrict__ hs, const uint32_t *__restrict__ qcnt, const WaveStep *__restrict__ step,
                                          const uint32_t *__restrict__ epos, uint64_t b0, uint32_t first, uint32_t n, uint32_t lane) {
        h.tstart = h.qstart = 0xFFFFFFFFu; h.length = 0; h.score = 0;
        if (first + lane < n) { const uint64_t i = b0 + first + lane; h = hs[i]; q = qcnt[i]; c = step[i].tcnt; e = epos[i]; }
    }
};

__global__ __launch_bounds__(CW_THREADS) void k5_chain_wave(Group *__restrict__ groups, const uint32_t *__restrict__ list, mimeo_hsp *__restrict__ hs,
                                                            long long *__restrict__ best, unsigned long long *__restrict__ fen_all,
                                                            int *__restrict__ pred, const uint4 *__restrict__ erec_all, unsigned long long *__restrict__ beste_all,
                                                            const uint32_t *__restrict__ epos, const uint32_t *__restrict__ qcnt,
                                                            const WaveStep *__restrict__ step) {
    constexpr uint32_t NW = CW_THREADS / 64;
    __shared__ long long s_best[NW];
    __shared__ uint32_t s_idx[NW];
    __shared__ uint32_t s_m;
    __shared__ unsigned long long s_part[NW][CH_TILE];
    __shared__ unsigned long long s_blk[CW_BLOCKS];
    Group &G = groups[list[blockIdx.x]];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t n = (uint32_t)(G.hsp_end - G.hsp_begin), tid = threadIdx.x, lane = tid & 63u, wv_no = tid >> 6;
    unsigned long long *fen = fen_all + b0, *beste = beste_all + b0;
    const uint4 *erec = erec_all + b0;
    uint32_t bshift = 10;
    while (((n - 1u) >> bshift) >= CW_BLOCKS) bshift++;   // n < 2^24: 12 at most
    const WaveTree T{fen, s_blk, n, bshift, ((n - 1u) >> bshift) + 1u};
    for (uint32_t k = tid; k < n; k += CW_THREADS) { fen[k] = 0ull; beste[k] = 0ull; }
    for (uint32_t k = tid; k < CW_BLOCKS; k += CW_THREADS) s_blk[k] = 0ull;
    __threadfence();
    __syncthreads();
    uint32_t a = 0, c = 0;   // E[.. c) are in the tree, visibly
    WaveStep s = step[b0];
    TileAhead nx;
    nx.fetch(hs, qcnt, step, epos, b0, 0, n, lane);
    while (a < n) {
        const uint32_t ca = s.tcnt, b = s.end & ~CW_PURE;
        const bool pure = (s.end & CW_PURE) != 0;
        CW_REGION_END();
        if (b < n) s = step[b0 + b];   // the next step's header: in flight during this one
        const mimeo_hsp hk = nx.h;
        const uint32_t qk = nx.q, ck = nx.c, ek = nx.e;
        if (pure) {
            nx.fetch(hs, qcnt, step, epos, b0, b, n, lane);
            // a wave: every HSP that ended at or before its first start goes into the tree, then one query per member
            for (uint32_t x = c + tid; x < ca; x += CW_THREADS) cw_insert(T, erec[x].z, beste[x]);
            __threadfence();
            __syncthreads();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            for (uint32_t k = a + tid; k < b; k += CW_THREADS) {
                WaveQuery Q;
                cw_query_issue(T, qcnt[b0 + k], Q);
                const unsigned long long m = cw_query_reduce(Q);
                const long long bk = (long long)(m >> 24) + hs[b0 + k].score;
                best[b0 + k] = bk;
                pred[b0 + k] = m ? (int)(CW_MAX - 1u - (uint32_t)(m & (CW_MAX - 1u))) : -1;
                beste_all[epos[b0 + k]] = cw_pack(bk, k);
            }
            CW_REGION_END();
        } else {
            // a tile of up to 64 members.  Window = E[c .. tcnt of the last member): the HSPs that are not in the tree for
            // sure.  It is dealt to the wavefronts 1 ..; a share is two coalesced loads, every lane tests the entries
            // that can matter against its own member.  The entries in front of ca — ends at or before the
            // tile's first start, final since the step before — go into the tree on the way: legal predecessors of every
            // member in the target, tested here as well, so it does not matter when a query sees them.
            const uint32_t k = a + lane, cnt = b - a;
            const bool live = k < b;
            const uint32_t ts_last = (uint32_t)__builtin_amdgcn_readlane((int)hk.tstart, (int)(cnt - 1u));
            const uint32_t cend = (uint32_t)__builtin_amdgcn_readlane((int)ck, (int)(cnt - 1u));
            unsigned long long m = 0;
            if (wv_no == 0) {
                WaveQuery Q;
                cw_query_issue(T, live ? qk : 0u, Q);   // wavefront 0 asks the tree
                nx.fetch(hs, qcnt, step, epos, b0, b, n, lane);
                m = cw_query_reduce(Q);
                CW_REGION_END();
            } else {
                bool fetched = false;
                if (cend > c) {
                    // the window in equal shares (8 entries at least) for the other wavefronts
                    constexpr uint32_t H = NW - 1u;
                    const uint32_t per = max((cend - c + H - 1u) / H, 8u), w_begin = c + (wv_no - 1u) * per, w_end = min(cend, w_begin + per);
                    for (uint32_t w0 = w_begin; w0 < w_end; w0 += (uint32_t)CH_TILE) {
                        uint4 r = make_uint4(0xFFFFFFFFu, 0xFFFFFFFFu, 0u, 0u);
                        unsigned long long v = 0;
                        if (w0 + lane < w_end) { r = erec[w0 + lane]; v = beste[w0 + lane]; }
                        if (!fetched) { nx.fetch(hs, qcnt, step, epos, b0, b, n, lane); fetched = true; }
                        if (w0 + lane < min(w_end, ca)) cw_insert(T, r.z, v);
                        const bool use = v != 0ull && r.x <= ts_last;   // 0: a member of this tile (not final)
                        for (unsigned long long mask = __ballot(use); mask; mask &= mask - 1ull) {
                            const int jj = __ffsll((long long)mask) - 1;
                            const unsigned long long vj = readlane64(v, jj);
                            const uint32_t tej = (uint32_t)__builtin_amdgcn_readlane((int)r.x, jj), qej = (uint32_t)__builtin_amdgcn_readlane((int)r.y, jj);
                            if (tej <= hk.tstart && qej <= hk.qstart) m = vj > m ? vj : m;
                        }
                    }
                }
                if (!fetched) nx.fetch(hs, qcnt, step, epos, b0, b, n, lane);
            }
            CW_REGION_END();
            if (wv_no) s_part[wv_no][lane] = m;
            // LDS only: the insertions may still be on their way (they are waited for at the end of the step)
            asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory");
            CW_REGION_END();
            if (wv_no == 0) {
                for (uint32_t w = 1; w < NW; w++) { const unsigned long long o = s_part[w][lane]; m = o > m ? o : m; }
                // members of the tile in front of a member, in ascending order (a member is final once those before it are done)
                const uint32_t te = hk.tstart + hk.length, qe = hk.qstart + hk.length;
                for (unsigned long long mask = __ballot(live && lane + 1u < cnt && te <= ts_last); mask; mask &= mask - 1ull) {
                    const int jj = __ffsll((long long)mask) - 1;
                    const long long bj = (long long)readlane64((unsigned long long)((long long)(m >> 24) + hk.score), jj);
                    const uint32_t tej = (uint32_t)__builtin_amdgcn_readlane((int)te, jj), qej = (uint32_t)__builtin_amdgcn_readlane((int)qe, jj);
                    if (live && lane > (uint32_t)jj && tej <= hk.tstart && qej <= hk.qstart) {
                        const unsigned long long v = cw_pack(bj, a + (uint32_t)jj);
                        m = v > m ? v : m;
                    }
                }
                if (live) {
                    const long long bk = (long long)(m >> 24) + hk.score;
                    best[b0 + k] = bk;
                    pred[b0 + k] = m ? (int)(CW_MAX - 1u - (uint32_t)(m & (CW_MAX - 1u))) : -1;
                    beste_all[ek] = cw_pack(bk, k);
                }
            }
            CW_REGION_END();
            __threadfence();   // stores and insertions done
            CW_REGION_END();
        }
        __syncthreads();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");   // the vector L1 may hold tree nodes from before this step's insertions
        CW_REGION_END();
        c = ca;
        a = b;
    }
    chain_tail(G, hs, best, pred, b0, n, s_best, s_idx, &s_m);
}

int chain_wave_groups(Group *d_groups, uint32_t ngroups, const uint32_t *d_list, uint32_t nlist, mimeo_hsp *d_sorted, uint64_t nhsps,
                      long long *d_best, unsigned long long *d_fen, int *d_pred, uint32_t big_min, bool stats) {
    K5Scratch &S = g_k5;
    const hipStream_t st = stream();
    if (int rc = S.reserve(KTE, EPOS, nhsps)) return rc;
    const dim3 blk(256), grd((uint32_t)((nhsps + 255) / 256));
    const int gbits = 32 - __builtin_clz(std::max(ngroups, 2u) - 1u);   // the group word of the keys: smallest g >= 1 with 2^g >= ngroups
    hipLaunchKernelGGL(k5w_end_keys, grd, blk, 0, st, d_sorted, S.u64(GKEY), nhsps, 0, S.u64(KEYS), S.u32(VALS));
    if (int rc = S.sort_pairs(KEYS, KTE, VALS, TE_ORDER, nhsps, 0, 32 + gbits)) return rc;
    hipLaunchKernelGGL(k5w_end_keys, grd, blk, 0, st, d_sorted, S.u64(GKEY), nhsps, 1, S.u64(KEYS), S.u32(VALS));
    if (int rc = S.sort_pairs(KEYS, KQE, VALS, QE_ORDER, nhsps, 0, 32 + gbits)) return rc;
    hipLaunchKernelGGL(k5w_prepare, grd, blk, 0, st, d_groups, d_sorted, S.u64(GKEY), S.u64(KTE), S.u64(KQE), S.u32(QE_ORDER), nhsps, big_min,
                       S.u32(QPOS), S.u32(QCNT), S.as<WaveStep>(STEP));
    if (stats) {
        DeviceBuf sb;
        if (int rc = sb.reserve((size_t)nlist * CW_STATS * 8)) return rc;
        hipLaunchKernelGGL(k5w_stats, dim3((nlist + 63) / 64), dim3(64), 0, st, d_groups, d_list, nlist, S.as<WaveStep>(STEP), (unsigned long long *)sb.p);
        std::vector<unsigned long long> hv((size_t)nlist * CW_STATS);
        HIP_TRY(hipStreamSynchronize(st));
        HIP_TRY(hipMemcpy(hv.data(), sb.p, hv.size() * 8, hipMemcpyDeviceToHost));
        sb.release();
        for (uint32_t g = 0; g < nlist; g++) {
            const unsigned long long *v = &hv[(size_t)g * CW_STATS];
            fprintf(stderr, "[k5w] group %u: n %llu tiles %llu waves %llu (members %llu) window entries %llu chunks %llu widest %llu\n", g, v[0], v[1],
                    v[2], v[3], v[4], v[5], v[6]);
        }
    }
    hipLaunchKernelGGL(k5w_end_records, grd, blk, 0, st, d_groups, d_sorted, S.u64(KTE), S.u32(TE_ORDER), S.u32(QPOS), nhsps, big_min, S.as<uint4>(EREC),
                       S.u32(EPOS));
    hipLaunchKernelGGL(k5_chain_wave, dim3(nlist), dim3(CW_THREADS), 0, st, d_groups, d_list, d_sorted, d_best, d_fen, d_pred, S.as<uint4>(EREC),
                       S.as<unsigned long long>(BESTE), S.u32(EPOS), S.u32(QCNT), S.as<WaveStep>(STEP));
    return 0;
}

}  // namespace mimeo
