// K5 — lastz `--chain` (reference call site src/mimeo/wrappers.py:1031 `--chain`); DESIGN.md §4 K5.
// Work unit = one group = one (target scaffold, query scaffold, strand), one workgroup owns it: sort the HSPs of all groups by
// (group, tstart, qstart, length); chain DP forward in tiles of 64, tiles and members visited in ascending order and only a strict
// improvement replacing a predecessor, so ties go to the earliest predecessor and the earliest chain end; flag the chain and order
// the chained HSPs by (score desc, tstart, qstart, length), the order in which K6 turns them into anchors.
// Shared device code and the scratch: k5.h; the wave kernel for large groups: k5_wave.hip; here the rest.
#include <cstring>

#include <rocprim/rocprim.hpp>

#include "k5.h"

namespace mimeo {

K5Scratch g_k5;
void release_k5_buffers() { g_k5.release(); }

int K5Scratch::sort_pairs(K5Buf key_in, K5Buf key_out, K5Buf val_in, K5Buf val_out, uint64_t n, unsigned bit0, unsigned bit1) {
    size_t tb = 0;   // one pointer type for inputs and outputs: one set of rocPRIM kernels
    HIP_TRY(rocprim::radix_sort_pairs(nullptr, tb, u64(key_in), u64(key_out), u32(val_in), u32(val_out), (size_t)n, bit0, bit1, stream()));
    if (int rc = buf[TMP].reserve(tb + 16)) return rc;
    HIP_TRY(rocprim::radix_sort_pairs(buf[TMP].p, tb, u64(key_in), u64(key_out), u32(val_in), u32(val_out), (size_t)n, bit0, bit1, stream()));
    return 0;
}

// sort plumbing: key1 = (qstart, length), key2 = (group = unit of the batch, tstart); the HSPs arrive in no order,
// tagged with their unit (K4 works on the whole batch at once)
__global__ void k5_key1(const mimeo_hsp *__restrict__ in, uint64_t n, uint64_t *__restrict__ key, uint32_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    key[i] = ((uint64_t)in[i].qstart << 32) | in[i].length;
    val[i] = (uint32_t)i;
}
__global__ void k5_key2(const mimeo_hsp *__restrict__ in, const uint32_t *__restrict__ unit, const uint32_t *__restrict__ perm,
                        uint64_t n, uint64_t *__restrict__ key) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t src = perm[i];
    key[i] = ((uint64_t)unit[src] << 32) | in[src].tstart;
}
// the sorted keys carry the group in their high word: a group's HSP range is where that word changes (groups
// without HSPs keep the empty range the host gave them)
__global__ void k5_group_ranges(const uint64_t *__restrict__ key, uint64_t n, Group *__restrict__ groups) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint32_t g = (uint32_t)(key[i] >> 32);
    if (i == 0 || (uint32_t)(key[i - 1] >> 32) != g) groups[g].hsp_begin = i;
    if (i + 1 == n || (uint32_t)(key[i + 1] >> 32) != g) groups[g].hsp_end = i + 1;
}
__global__ void k5_gather(const mimeo_hsp *__restrict__ in, const uint32_t *__restrict__ perm, uint64_t n,
                          mimeo_hsp *__restrict__ hs) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    mimeo_hsp h = in[perm[i]];
    h.flags = 0;
    hs[i] = h;
}

// the tile kernel.  skip_large: groups of more than big_min HSPs are the large-group kernels' (k5_big_list has listed them);
// do_chain = 0 (no chaining asked for): every HSP of the group is an anchor
__global__ __launch_bounds__(CH_THREADS) void k5_chain(Group *__restrict__ groups,
                                                       mimeo_hsp *__restrict__ hs, long long *__restrict__ best,
                                                       long long *__restrict__ cand, int *__restrict__ pred,
                                                       int do_chain, uint32_t big_min, int skip_large) {
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t n = (uint32_t)(G.hsp_end - G.hsp_begin);
    const uint32_t tid = threadIdx.x;
    __shared__ long long s_best[CH_THREADS / 64];
    __shared__ uint32_t s_idx[CH_THREADS / 64];
    __shared__ uint32_t s_m;
    __shared__ uint32_t s_te[CH_TILE], s_qe[CH_TILE];
    __shared__ long long s_b[CH_TILE];
    __shared__ uint32_t s_sqe[CH_TILE], s_pmi[CH_TILE], s_maxte;
    __shared__ long long s_pmb[CH_TILE];
    if (n == 0) { if (tid == 0) G.nchain = 0; return; }
    if (do_chain && skip_large && n > big_min) return;
    if (do_chain) {   // hs[b0 .. b0+n) arrives sorted by (tstart, qstart, length) (device-wide radix sorts, chain_device)
        const TileLds L{s_te, s_qe, s_b, s_sqe, s_pmi, s_pmb, &s_maxte};
        for (uint32_t k = tid; k < n; k += CH_THREADS) { cand[b0 + k] = 0; pred[b0 + k] = -1; }
        __syncthreads();
        CHAIN_TILE_SWEEP(0, n, n, L)
        chain_tail(G, hs, best, pred, b0, n, s_best, s_idx, &s_m);
    } else {
        for (uint32_t k = tid; k < n; k += CH_THREADS) hs[b0 + k].flags = 1;
        if (tid == 0) G.nchain = n;
    }
}

// ---- two-level chain DP for large groups ------------------------------------------------------------------------------
// k5_chain makes one pass over ALL later HSPs of the group per tile of 64: n^2 / 64 visits, each with its 40 bytes from
// global memory — 13 s for the 1.35 * 10^6 HSPs of one strand of a 150 Mbp self pair, on one CU.  Here the HSPs are
// taken in BLOCKS of 2048: inside a block the tiles relax only the rest of the block (L2-resident); the finished block is
// then summarised once — its members ordered by query end with the running best over that order, beside the per-tile
// summaries it already has — and ONE pass over the later HSPs relaxes them against the whole block: a binary search
// over 2048 members when the HSP starts behind all of them in the target, tile by tile (exactly k5_chain's step)
// otherwise.  32 times fewer passes; predecessors and ties as in k5_chain: the maximum over the eligible members of a
// block with the smallest member on ties is what its 32 tiles, visited in order with strict improvements, arrive at.
constexpr uint32_t CH_BLOCK = 2048;   // 32 tiles
constexpr size_t CH_BIG_LDS = (size_t)CH_BLOCK * 48 + 1024;
__global__ __launch_bounds__(CH_THREADS) void k5_chain_big(Group *__restrict__ groups, const uint32_t *__restrict__ big_list,
                                                           const unsigned int *__restrict__ nbig, mimeo_hsp *__restrict__ hs,
                                                           long long *__restrict__ best, long long *__restrict__ cand, int *__restrict__ pred) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    long long *B_b = reinterpret_cast<long long *>(lds), *T_pmb = B_b + CH_BLOCK, *S_pmb = T_pmb + CH_BLOCK;
    uint32_t *B_te = reinterpret_cast<uint32_t *>(S_pmb + CH_BLOCK), *B_qe = B_te + CH_BLOCK, *T_sqe = B_qe + CH_BLOCK, *T_pmi = T_sqe + CH_BLOCK,
             *S_sqe = T_pmi + CH_BLOCK, *S_pmi = S_sqe + CH_BLOCK, *T_maxte = S_pmi + CH_BLOCK;
    unsigned long long *skey = reinterpret_cast<unsigned long long *>(S_pmb);   // sort scratch: the block summary's slot until it is written
    __shared__ long long s_best[CH_THREADS / 64];
    __shared__ uint32_t s_idx[CH_THREADS / 64];
    __shared__ uint32_t s_m, s_blkmaxte;
    const uint32_t tid = threadIdx.x;
    const TileLds LB{B_te, B_qe, B_b, T_sqe, T_pmi, T_pmb, T_maxte};   // the block's tiles, one slot each
    for (uint32_t li = blockIdx.x; li < *nbig; li += gridDim.x) {
        Group &G = groups[big_list[li]];
        const uint64_t b0 = G.hsp_begin;
        const uint32_t n = (uint32_t)(G.hsp_end - G.hsp_begin);
        for (uint32_t k = tid; k < n; k += CH_THREADS) { cand[b0 + k] = 0; pred[b0 + k] = -1; }
        __syncthreads();
        for (uint32_t blk0 = 0; blk0 < n; blk0 += CH_BLOCK) {
            const uint32_t blk1 = min(n, blk0 + CH_BLOCK), cntB = blk1 - blk0;
            // 1. the block's tiles, relaxing inside the block only
            CHAIN_TILE_SWEEP(blk0, blk1, blk1, LB.at((t0 - blk0) / CH_TILE))
            if (blk1 >= n) break;   // nothing behind the last block
            // 2. the block's summary: members by (query end, member) — bitonic sort of 2048 keys — and the running best
            for (uint32_t e = tid; e < CH_BLOCK; e += CH_THREADS)
                skey[e] = e < cntB ? (((unsigned long long)B_qe[e] << 32) | e) : ~0ull;
            __syncthreads();
            for (uint32_t k = 2; k <= CH_BLOCK; k <<= 1)
                for (uint32_t j = k >> 1; j > 0; j >>= 1) {
                    const uint32_t i = ((tid & ~(j - 1u)) << 1) | (tid & (j - 1u)), l = i | j;
                    const unsigned long long a = skey[i], b = skey[l];
                    if ((a > b) == ((i & k) == 0)) { skey[i] = b; skey[l] = a; }
                    __syncthreads();
                }
            unsigned long long key2[2];
            for (int h = 0; h < 2; h++) key2[h] = skey[tid + h * CH_THREADS];
            uint32_t mte = 0;
            for (uint32_t e = tid; e < cntB; e += CH_THREADS) mte = max(mte, B_te[e]);
            for (int o = 32; o > 0; o >>= 1) mte = max(mte, (uint32_t)__shfl_xor((int)mte, o));
            if ((tid & 63) == 0) s_idx[tid >> 6] = mte;
            __syncthreads();   // every key is read before its slot becomes a running best
            if (tid == 0) { uint32_t m = 0; for (int w = 0; w < CH_THREADS / 64; w++) m = max(m, s_idx[w]); s_blkmaxte = m; }
            for (int h = 0; h < 2; h++) {
                const uint32_t e = tid + h * CH_THREADS, idx = (uint32_t)key2[h];
                const bool live = key2[h] != ~0ull;
                S_sqe[e] = live ? (uint32_t)(key2[h] >> 32) : 0xFFFFFFFFu;
                S_pmi[e] = live ? idx : 0xFFFFFFFFu;
                S_pmb[e] = live ? B_b[idx] : INT64_MIN;
            }
            __syncthreads();
            for (uint32_t o = 1; o < CH_BLOCK; o <<= 1) {   // inclusive running maximum, ties to the smaller member
                long long ub[2]; uint32_t ui[2];
                for (int h = 0; h < 2; h++) {
                    const uint32_t e = tid + h * CH_THREADS;
                    ub[h] = e >= o ? S_pmb[e - o] : INT64_MIN; ui[h] = e >= o ? S_pmi[e - o] : 0xFFFFFFFFu;
                }
                __syncthreads();
                for (int h = 0; h < 2; h++) {
                    const uint32_t e = tid + h * CH_THREADS;
                    if (e >= o && (ub[h] > S_pmb[e] || (ub[h] == S_pmb[e] && ui[h] < S_pmi[e]))) { S_pmb[e] = ub[h]; S_pmi[e] = ui[h]; }
                }
                __syncthreads();
            }
            // 3. one pass over the HSPs behind the block
            const uint32_t blkmaxte = s_blkmaxte, nsub = (cntB + CH_TILE - 1) / CH_TILE;
            for (uint32_t k = blk1 + tid; k < n; k += CH_THREADS) {
                const mimeo_hsp &hk = hs[b0 + k];
                const uint32_t ts = hk.tstart, qs = hk.qstart;
                long long c = cand[b0 + k];
                int pk = -2;
                if (blkmaxte <= ts) {
                    chain_summary_search(S_sqe, S_pmb, S_pmi, cntB, blk0, qs, c, pk);
                } else {
                    for (uint32_t s = 0; s < nsub; s++)
                        chain_tile_relax(LB.at(s), min((uint32_t)CH_TILE, cntB - s * CH_TILE), blk0 + s * CH_TILE, ts, qs, c, pk);
                }
                if (pk != -2) { cand[b0 + k] = c; pred[b0 + k] = pk; }
            }
            __syncthreads();
        }
        chain_tail(G, hs, best, pred, b0, n, s_best, s_idx, &s_m);
        __syncthreads();
    }
}

// the large groups (more than big_min HSPs): list_wave = the wave kernel's (fewer than 2^24 HSPs), list_two_level = k5_chain_big's
__global__ void k5_big_list(const Group *__restrict__ groups, uint32_t ngroups, uint32_t big_min, int all_two_level, uint32_t *__restrict__ list_wave,
                            uint32_t *__restrict__ list_two_level, unsigned int *__restrict__ cnt) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    const uint64_t n = groups[g].hsp_end - groups[g].hsp_begin;
    if (n <= big_min) return;
    if (n < CW_MAX && !all_two_level) list_wave[atomicAdd(cnt, 1u)] = g;
    else list_two_level[atomicAdd(cnt + 1, 1u)] = g;
}

// Anchor order: the HSPs already lie in (group, tstart, qstart, length) order, so one STABLE radix sort by
// (group, not chained, -score) leaves every group's chained HSPs in anchor order at the front of its range.
__global__ void k5_rank_keys(const mimeo_hsp *__restrict__ hs, const uint64_t *__restrict__ gkey, uint64_t n, uint64_t *__restrict__ key,
                             uint32_t *__restrict__ val) {
    const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const uint64_t MAXS = (1ull << 40) - 1ull;
    const int64_t sc = hs[i].score;
    const uint64_t inv = MAXS - (uint64_t)(sc < 0 ? 0 : (sc > (int64_t)MAXS ? (int64_t)MAXS : sc));
    key[i] = ((gkey[i] >> 32) << 41) | ((hs[i].flags & 1u) ? 0ull : (1ull << 40)) | inv;
    val[i] = (uint32_t)i;
}
__global__ void k5_write_order(const uint32_t *__restrict__ val, const uint64_t *__restrict__ key, const Group *__restrict__ groups,
                               uint64_t n, uint32_t *__restrict__ order) {
    const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= n) return;
    order[r] = val[r] - (uint32_t)groups[key[r] >> 41].hsp_begin;   // index inside the group
}

// switches read once per call (tests change them between calls); DESIGN.md §5 has the variables
struct K5Switches { uint32_t big_min; bool use_large, all_two_level, stats; };   // all_two_level: every large group goes to k5_chain_big
static K5Switches k5_switches() {
    const char *mode = getenv("MIMEO_K5_BIG"), *bm = getenv("MIMEO_K5_BIG_MIN");
    char *end = nullptr;
    const long long v = bm && *bm ? strtoll(bm, &end, 10) : 0;   // missing, empty, no number or < 1: the default
    return {v >= 1 && *end == 0 ? (uint32_t)std::min<long long>(v, 0xFFFFFFFFll) : CH_BIG, !getenv("MIMEO_K5_NO_BIG"), mode && !strcmp(mode, "old"),
            getenv("MIMEO_K5_STATS") != nullptr};
}

int chain_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_hsps, const uint32_t *d_hsp_unit, uint64_t nhsps,
                 int do_chain, mimeo_hsp *d_sorted, long long *d_best, long long *d_cand, int *d_pred, uint32_t *d_order) {
    if (!ngroups || !nhsps) return 0;
    if (nhsps >= (1ull << 32)) { set_error("more than 2^32 HSPs in one batch"); return MIMEO_ERR_LIMIT; }
    const K5Switches sw = k5_switches();
    K5Scratch &S = g_k5;
    hipStream_t st = stream();
    int rc;
    if ((rc = S.reserve(KEYS, PERM, nhsps))) return rc;
    const dim3 blk(256), grd((uint32_t)((nhsps + 255) / 256));
    hipLaunchKernelGGL(k5_key1, grd, blk, 0, st, d_hsps, nhsps, S.u64(KEYS), S.u32(PERM));
    if ((rc = S.sort_pairs(KEYS, GKEY, PERM, VALS, nhsps, 0, 64))) return rc;
    hipLaunchKernelGGL(k5_key2, grd, blk, 0, st, d_hsps, d_hsp_unit, S.u32(VALS), nhsps, S.u64(KEYS));
    if ((rc = S.sort_pairs(KEYS, GKEY, VALS, PERM, nhsps, 0, 64))) return rc;
    hipLaunchKernelGGL(k5_group_ranges, grd, blk, 0, st, S.u64(GKEY), nhsps, d_groups);
    hipLaunchKernelGGL(k5_gather, grd, blk, 0, st, d_hsps, S.u32(PERM), nhsps, d_sorted);
    const bool large = do_chain && sw.use_large;
    if (large) {   // large groups: the wave kernel (k5_chain_big beyond 2^24 HSPs, or all of them under MIMEO_K5_BIG=old)
        if ((rc = S.buf[LARGE].reserve(((size_t)2 * ngroups + 4) * 4))) return rc;
        unsigned int *cnt = S.as<unsigned int>(LARGE);   // [0]: the wave kernel's groups, [1]: k5_chain_big's
        uint32_t *list_wave = S.u32(LARGE) + 4, *list_two_level = list_wave + ngroups;
        HIP_TRY(hipMemsetAsync(cnt, 0, 8, st));
        hipLaunchKernelGGL(k5_big_list, dim3((ngroups + 255) / 256), dim3(256), 0, st, d_groups, ngroups, sw.big_min, sw.all_two_level ? 1 : 0,
                           list_wave, list_two_level, cnt);
        unsigned int h[2] = {0, 0};
        HIP_TRY(hipMemcpyAsync(h, cnt, 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (h[1]) {
            if (!S.big_lds_set) {
                HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(k5_chain_big), hipFuncAttributeMaxDynamicSharedMemorySize, (int)CH_BIG_LDS));
                S.big_lds_set = true;
            }
            hipLaunchKernelGGL(k5_chain_big, dim3(std::min(h[1], 256u)), dim3(CH_THREADS), CH_BIG_LDS, st, d_groups, list_two_level, cnt + 1, d_sorted,
                               d_best, d_cand, d_pred);
        }
        if (h[0] && (rc = chain_wave_groups(d_groups, ngroups, list_wave, h[0], d_sorted, nhsps, d_best, (unsigned long long *)d_cand, d_pred,
                                            sw.big_min, sw.stats)))
            return rc;
    }
    hipLaunchKernelGGL(k5_chain, dim3(ngroups), dim3(CH_THREADS), 0, st, d_groups, d_sorted, d_best, d_cand, d_pred, do_chain, sw.big_min, large ? 1 : 0);
    // anchor order by one stable sort over 54 key bits
    hipLaunchKernelGGL(k5_rank_keys, grd, blk, 0, st, d_sorted, S.u64(GKEY), nhsps, S.u64(KEYS), S.u32(VALS));
    if ((rc = S.sort_pairs(KEYS, RANK_KEY, VALS, ANCHOR_PERM, nhsps, 0, 64))) return rc;
    hipLaunchKernelGGL(k5_write_order, grd, blk, 0, st, S.u32(ANCHOR_PERM), S.u64(RANK_KEY), d_groups, nhsps, d_order);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mimeo
