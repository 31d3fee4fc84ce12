// K5, shared by its files (overview: k5_chain.hip): the tile step of the chain DP, the chain end, the stage's scratch.  No relocatable device code: a kernel is launched from the file that defines it, shared device code is here.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "device_util.h"

namespace mimeo {

constexpr int CH_THREADS = 1024;
constexpr int CH_TILE = 64;  // HSPs finalised per step of the chain DP (one wavefront)

// Summaries of a finalised tile of 64 HSPs (a slice of larger arrays in the two-level kernel)
struct TileLds {
    uint32_t *te, *qe;       // members in index order: target end, query end
    long long *b;            // ... final chain score
    uint32_t *sqe, *pmi;     // the same tile ordered by query end, with the running best (and its member) over that order: an HSP
    long long *pmb;          //   that starts behind every member in the target finds its best predecessor by one binary search
    uint32_t *maxte;
    // the tile `tiles` tiles further on in the same arrays
    __device__ __forceinline__ TileLds at(uint32_t tiles) const {
        const uint32_t o = tiles * CH_TILE;
        return TileLds{te + o, qe + o, b + o, sqe + o, pmi + o, pmb + o, maxte + tiles};
    }
};

// a. wavefront 0 finalises HSPs t0 .. t0+63 of the group: every earlier tile has already relaxed them
__device__ __forceinline__ void chain_tile_final(const mimeo_hsp *__restrict__ hs, long long *__restrict__ best, const long long *__restrict__ cand,
                                                 int *__restrict__ pred, uint64_t b0, uint32_t n, uint32_t t0, const TileLds &L) {
    const uint32_t tid = threadIdx.x;
    const uint32_t j = t0 + tid;
    const bool live = j < n;
    mimeo_hsp hj;
    hj.tstart = hj.qstart = 0xFFFFFFFFu; hj.length = 0; hj.score = 0;
    long long cj = 0;
    int pj = -1;
    if (live) { hj = hs[b0 + j]; cj = cand[b0 + j]; pj = pred[b0 + j]; }
    const uint32_t te = hj.tstart + hj.length, qe = hj.qstart + hj.length;
    const uint32_t cnt = min((uint32_t)CH_TILE, n - t0);
    for (uint32_t jj = 0; jj + 1 < cnt; jj++) {
        const long long bj = __shfl(cj + hj.score, (int)jj);  // final: members before jj are done
        const uint32_t tej = (uint32_t)__shfl((int)te, (int)jj), qej = (uint32_t)__shfl((int)qe, (int)jj);
        if (live && tid > jj && tej <= hj.tstart && qej <= hj.qstart && bj > cj) { cj = bj; pj = (int)(t0 + jj); }
    }
    const long long bfin = cj + hj.score;
    if (live) {
        best[b0 + j] = bfin;
        pred[b0 + j] = pj;
        L.te[tid] = te; L.qe[tid] = qe; L.b[tid] = bfin;
    }
    // bitonic sort of the 64 members by (query end, member) with shuffles; dead lanes sort to the end
    uint32_t kq = live ? qe : 0xFFFFFFFFu, ki = tid;
    long long kb = live ? bfin : INT64_MIN;
    for (uint32_t k = 2; k <= 64; k <<= 1)
        for (uint32_t jx = k >> 1; jx > 0; jx >>= 1) {
            const uint32_t oq = (uint32_t)__shfl_xor((int)kq, (int)jx), oi = (uint32_t)__shfl_xor((int)ki, (int)jx);
            const long long ob = __shfl_xor(kb, (int)jx);
            const bool up = (tid & k) == 0, lower = (tid & jx) == 0;
            const bool mine_less = kq < oq || (kq == oq && ki < oi);
            const bool keep = (lower == up) ? mine_less : !mine_less;   // keep the smaller in the lower lane of an ascending pair
            if (!keep) { kq = oq; ki = oi; kb = ob; }
        }
    // inclusive running maximum of the final values in that order; ties to the smaller member
    long long pb = kb;
    uint32_t pi = ki;
    for (int o = 1; o < 64; o <<= 1) {
        const long long ub = __shfl_up(pb, o);
        const uint32_t ui = (uint32_t)__shfl_up((int)pi, o);
        if (tid >= (uint32_t)o && (ub > pb || (ub == pb && ui < pi))) { pb = ub; pi = ui; }
    }
    L.sqe[tid] = kq; L.pmb[tid] = pb; L.pmi[tid] = pi;
    uint32_t mte = live ? te : 0u;
    for (int o = 32; o > 0; o >>= 1) mte = max(mte, (uint32_t)__shfl_xor((int)mte, o));
    if (tid == 0) *L.maxte = mte;
}

// first position of the sorted a[lo .. hi) whose key is above `key` (upper) or not below it (lower)
template <class T, class I>
__device__ __forceinline__ I bisect(const T *a, I lo, I hi, T key, bool upper) {
    while (lo < hi) { const I mid = (lo + hi) >> 1; if (upper ? a[mid] <= key : a[mid] < key) lo = mid + 1; else hi = mid; }
    return lo;
}

// The one summary search: cnt finalised members (a tile's, or a block's in the two-level kernel) ordered by query end in sqe, with
// the running best over that order in pmb and its member in pmi, all ending in front of the HSP in the target.  The best that also
// ends in front of it in the query = the running best at the last sorted member with query end <= qs.  Member m is HSP base + m.
__device__ __forceinline__ void chain_summary_search(const uint32_t *sqe, const long long *pmb, const uint32_t *pmi, uint32_t cnt, uint32_t base,
                                                     uint32_t qs, long long &c, int &pk) {
    const uint32_t lo = bisect(sqe, 0u, cnt, qs, true);  // number of sorted members with query end <= qs
    if (lo && pmb[lo - 1] > c) { c = pmb[lo - 1]; pk = (int)(base + pmi[lo - 1]); }
}

// the best predecessor of an HSP (ts, qs) among the cnt members of a finalised tile whose first member is HSP t0: strict
// improvements of (c, pk) only, members in ascending order.  The search runs over all CH_TILE slots, not over cnt: the dead lanes of
// a short tile sort to the end with key 0xFFFFFFFF and carry the running best (and its member) of the last live one forward, so a
// search that ends among them reads what slot cnt - 1 holds; the constant count keeps the search a fixed six steps.
__device__ __forceinline__ void chain_tile_relax(const TileLds &L, uint32_t cnt, uint32_t t0, uint32_t ts, uint32_t qs, long long &c, int &pk) {
    if (*L.maxte <= ts) {
        chain_summary_search(L.sqe, L.pmb, L.pmi, CH_TILE, t0, qs, c, pk);
    } else {
        for (uint32_t ii = 0; ii < cnt; ii++)
            if (L.te[ii] <= ts && L.qe[ii] <= qs && L.b[ii] > c) { c = L.b[ii]; pk = (int)(t0 + ii); }
    }
}

// The tile sweep: finalise the tiles of [t_begin, t_end) in ascending order and relax the HSPs of [.., relax_end) behind
// each against its final values; L_AT = the summaries of the tile at t0.  The whole workgroup runs it, with hs, best, cand,
// pred, b0, n and tid as the kernels name them.  A macro: as an inlined function the same text compiles to another
// schedule, which cost k5_chain 1.6 % (profiles/r22_ab_k5.json, series 1).
#define CHAIN_TILE_SWEEP(t_begin, t_end, relax_end, L_AT)                                                    \
    for (uint32_t t0 = (t_begin); t0 < (t_end); t0 += CH_TILE) {                                             \
        const TileLds Lt = L_AT;                                                                             \
        if (tid < CH_TILE) chain_tile_final(hs, best, cand, pred, b0, n, t0, Lt);                            \
        __syncthreads();                                                                                     \
        const uint32_t cnt = min((uint32_t)CH_TILE, n - t0);                                                 \
        for (uint32_t k = t0 + CH_TILE + tid; k < (relax_end); k += CH_THREADS) { /* everybody relaxes */    \
            const mimeo_hsp &hk = hs[b0 + k];                                                                \
            long long c = cand[b0 + k];                                                                      \
            int pk = -2;                                                                                     \
            chain_tile_relax(Lt, cnt, t0, hk.tstart, hk.qstart, c, pk);                                      \
            if (pk != -2) { cand[b0 + k] = c; pred[b0 + k] = pk; }                                           \
        }                                                                                                    \
        __syncthreads();                                                                                     \
    }

// chain end = argmax of best (earliest on ties), flags along its predecessors; G.nchain
__device__ __forceinline__ void chain_tail(Group &G, mimeo_hsp *__restrict__ hs, const long long *__restrict__ best, const int *__restrict__ pred,
                                           uint64_t b0, uint32_t n, long long *s_best, uint32_t *s_idx, uint32_t *s_m) {
    const uint32_t tid = threadIdx.x;
    long long mb = INT64_MIN;
    uint32_t mi = 0xFFFFFFFFu;
    for (uint32_t k = tid; k < n; k += blockDim.x) {
        long long v = best[b0 + k];
        if (v > mb) { mb = v; mi = k; }
    }
    for (int o = 32; o > 0; o >>= 1) {
        long long ob = __shfl_xor(mb, o);
        uint32_t oi = __shfl_xor(mi, o);
        if (ob > mb || (ob == mb && oi < mi)) { mb = ob; mi = oi; }
    }
    if ((tid & 63) == 0) { s_best[tid >> 6] = mb; s_idx[tid >> 6] = mi; }
    __syncthreads();
    if (tid == 0) {
        for (int w = 1; w < (int)(blockDim.x / 64); w++)
            if (s_best[w] > mb || (s_best[w] == mb && s_idx[w] < mi)) { mb = s_best[w]; mi = s_idx[w]; }
        uint32_t m = 0;
        for (int k = (int)mi; k >= 0; k = pred[b0 + k]) { hs[b0 + k].flags = 1; m++; }
        *s_m = m;
    }
    __syncthreads();
    if (tid == 0) G.nchain = *s_m;
}

// groups beyond CH_BIG HSPs are the large-group kernels'; the wave kernel takes those below CW_MAX
constexpr uint32_t CH_BIG = 32768, CW_MAX = 1u << 24;

// The stage's device buffers, grown on demand and kept between calls (K5 runs on the calling thread only), n = HSPs of the
// batch.  A second name is an alias: the same buffer, holding something else once its first content is done with.
enum K5Buf {
    KEYS, VALS,               // (8n, 4n) the unsorted pairs of the next sort (the first sort's values go PERM -> VALS).  Free between
                              //   the second sort and k5_rank_keys: the wave path prepares its two end-key sorts here meanwhile
    GKEY, RANK_KEY = GKEY,    // (8n) sorted keys: from the second sort on (group, tstart) of every sorted HSP; the last sort
                              //   writes the sorted rank keys over them
    PERM, ANCHOR_PERM = PERM, // (4n) sorted values: the source index of every sorted HSP until k5_gather has run; the last
                              //   sort writes the anchor order here
    KTE, BESTE = KTE,         // wave path: the HSPs' (group, target end) keys, sorted; done with once k5w_end_records has run:
                              //   k5_chain_wave keeps the chain values in target-end order here
    KQE, TE_ORDER, QE_ORDER,  // ... their (group, query end) keys, sorted; the HSPs in either order
    QPOS, QCNT, STEP, EREC, EPOS,   // ... what k5w_prepare and k5w_end_records make of them
    LARGE,                    // two counters and the two lists of large groups
    TMP,                      // rocPRIM's temporary storage
    K5_NBUF
};
constexpr size_t K5_ELEM[] = {8, 4, 8, 4, 8, 8, 4, 4, 4, 4, 8, 16, 4, 0, 0};   // bytes per HSP, in the enum's order (0: sized by its user)
static_assert(sizeof(K5_ELEM) / sizeof(K5_ELEM[0]) == K5_NBUF, "one size per buffer");
struct K5Scratch {
    DeviceBuf buf[K5_NBUF];
    bool big_lds_set = false;   // k5_chain_big's dynamic LDS limit is raised once per process
    template <class T> T *as(K5Buf b) const { return (T *)buf[b].p; }
    uint64_t *u64(K5Buf b) const { return as<uint64_t>(b); }
    uint32_t *u32(K5Buf b) const { return as<uint32_t>(b); }
    int reserve(K5Buf first, K5Buf last, uint64_t n) {
        for (int b = first; b <= last; b++)
            if (int rc = buf[b].reserve(n * K5_ELEM[b])) return rc;
        return 0;
    }
    // one stable device-wide radix sort by the key bits [bit0, bit1); asks rocPRIM what this very sort needs and reserves it (k5_chain.hip)
    int sort_pairs(K5Buf key_in, K5Buf key_out, K5Buf val_in, K5Buf val_out, uint64_t n, unsigned bit0, unsigned bit1);
    void release() { for (DeviceBuf &b : buf) b.release(); }
};
extern K5Scratch g_k5;   // k5_chain.hip

// k5_wave.hip: prepares the nlist large groups (more than big_min HSPs) of d_list (two sorts by end, ranks, counts, steps, end records)
// and runs the wave kernel over them.  GKEY holds the sorted HSPs' keys; d_fen = one Fenwick node per HSP (the caller's candidates)
int chain_wave_groups(Group *d_groups, uint32_t ngroups, const uint32_t *d_list, uint32_t nlist, mimeo_hsp *d_sorted, uint64_t nhsps,
                      long long *d_best, unsigned long long *d_fen, int *d_pred, uint32_t big_min, bool stats);

}  // namespace mimeo
