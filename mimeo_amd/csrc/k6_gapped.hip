// K6 — lastz `--gapped` (reference call site src/mimeo/wrappers.py:1031):
// every chained HSP becomes an anchor (centre of its best 31-column window); anchors are taken
// by decreasing HSP score, an anchor that lies inside the box of an earlier alignment is
// skipped, every other anchor is extended in both directions by a y-drop affine-gap DP
// (gap open 400 / extend 30, y-drop 9400) and the two halves are joined.
//
// Decomposition:
//   * a half extension is one JOB.  The DP is evaluated row by row; pruning: a cell scoring below
//     (best of the rows above) - ydrop is dead.  Cells carry (score, matches, mismatches), so
//     identity needs no traceback.  Inside a row the only horizontal dependency is the insertion
//     state, a max-plus prefix scan along the row (in-lane over a strip, then one cross-lane scan).
//     Three kernels, each taking the jobs the one before could not hold (dp_round):
//       - k6_dp1, the lean kernel: one wavefront, lane l owns the 14-column strip (j / 14) % 64 == l
//         of an 896-column window that slides with the first live column, all state in registers,
//         counts packed into 16 bits each (65 535 rows at most);
//       - k6_dp_wide, the second chance: the same layout with 32-column strips (2048 columns),
//         unpacked counts and no row limit;
//       - k6_dp_any, the last resort: one workgroup, the rows in global memory, bands up to 2^16
//         columns, cells rebased when the score nears 2^31.
//   * exact shortcut (identical_suffix): if the two sequences are identical and N-free from the
//     anchor to the end of the shorter one, the diagonal is optimal (every column already scores its
//     maximum) and the DP is skipped — this is what makes the trivial (A,A) self alignment cheap.
//   * jobs of different anchors are independent, only the skip rule is ordered: each round takes
//     the next <= nbatch unskipped anchors of every group (k6_pick), extends them all (dp_round),
//     then replays the skip rule in order over the batch (k6_resolve).
//   * path rule (mimeo_params.anchor_rule = MIMEO_ANCHOR_PATH, opt-in): an anchor is skipped iff it is a diagonal step of
//     the path of an earlier alignment.  After a round's DP kernels k6_trace re-runs the round's halves with a traceback,
//     checks them against the first run and leaves each path as gap-free blocks; k6_pick / k6_resolve<true> test the
//     blocks of the alignments whose box holds the anchor.  The box-rule kernels are unchanged.
//   * bounded extensions (mimeo_params.bound_extensions = 1, opt-in, path rule only; parity unpinned): a DP cell on or beyond the
//     nearest earlier path on either side of the anchor's diagonal is dead (alignment specification v1, rule 7; the specification is
//     tests/bounded_oracle.c).  k6_dp1_bounded / k6_dp_any<true> / k6_trace<true> look the bounds up row range by row range
//     (bounds_at); k6_resolve<true, true> sends an anchor back when an alignment accepted after its DP ran reaches into what it swept.
//   * paths out (mimeo_align_units_paths, under every rule; a call that does not ask launches what it launched before): the blocks of
//     the two halves of every returned alignment, merged at the anchor, in the dense order of k6_dense_copy (k6_path_count, a
//     scan, k6_path_write).  Under the box rule one trace pass after the last round makes the blocks (paths_pass).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include <rocprim/rocprim.hpp>

#include "device_util.h"

namespace mimeo {

constexpr int32_t NEG = -(1 << 30);
constexpr int32_t NEGH = -(1 << 29);
// columns per lane: 14 (896-column window) in the lean kernel k6_dp1, 32 (2048 columns) in the second-chance kernel

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

// WSTRIP query bits for columns jb .. jb+WSTRIP-1 (bit s <-> column jb+s); column j consumes query base
// aq + j - 1 (dir > 0) or aq - j (dir < 0).  Out-of-range columns read padding and are never used.
template <int WSTRIP>
__device__ __forceinline__ void load_qbits(const GStrandView &Q, uint32_t aq, int dir, uint32_t jb, uint32_t lenB,
                                           uint32_t &qlo, uint32_t &qhi, uint32_t &qn) {
    constexpr uint32_t SMASK = WSTRIP == 32 ? 0xFFFFFFFFu : ((1u << (WSTRIP & 31)) - 1u);  // WSTRIP in {14, 32}
    if (jb > lenB) { qlo = qhi = qn = 0; return; }
    if (dir > 0) {
        int32_t p = (int32_t)(aq + jb) - 1;
        const Win32 w = win32(Q, p);
        qlo = w.lo & SMASK; qhi = w.hi & SMASK; qn = w.nm & SMASK;
    } else {
        // bit t <-> position p + t <-> column jb + WSTRIP - 1 - t
        int32_t p = (int32_t)aq - (int32_t)jb - (WSTRIP - 1);
        const Win32 w = win32(Q, p);
        qlo = __brev(w.lo & SMASK) >> (32 - WSTRIP); qhi = __brev(w.hi & SMASK) >> (32 - WSTRIP);
        qn = __brev(w.nm & SMASK) >> (32 - WSTRIP);
    }
}

// Target bases of 32 consecutive DP rows i0 .. i0+31 (bit b <-> row i0 + b): one window load per 32 rows
// instead of a dependent global load in every row; the caller fetches one block ahead.
struct RowBases { uint32_t lo, hi, nm; };
__device__ __forceinline__ RowBases load_row_bases(const GStrandView &T, uint32_t at, int dir, uint32_t i0) {
    if (dir > 0) {
        const Win32 w = win32(T, (int32_t)(at + i0 - 1u));
        return RowBases{w.lo, w.hi, w.nm};
    }
    const Win32 w = win32(T, (int32_t)at - (int32_t)i0 - 31);
    return RowBases{__brev(w.lo), __brev(w.hi), __brev(w.nm)};
}

// The exact shortcut of a half extension, by one wavefront (every lane returns the same): true, and the result in `out`, iff
// the two sequences are identical and N-free from the anchor to the end of the shorter one (n bases); `out` is untouched
// otherwise.  The result is the diagonal: i == j == nm == n, and rows == 0 marks it as a shortcut result whose score is
// 64 bits wide, low word in score, high word in maxcols (half_score; k6_trace's TR_DIAG).
__device__ bool identical_suffix(const GStrandView &T, const GStrandView &Q, uint32_t at, uint32_t aq, int dir, HalfResult &out) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t n = min(dir > 0 ? T.len - at : at, dir > 0 ? Q.len - aq : aq);
    const int32_t st = dir > 0 ? (int32_t)at : (int32_t)(at - n), sq = dir > 0 ? (int32_t)aq : (int32_t)(aq - n);
    bool ok = true;
    uint64_t ncg = 0;
    for (uint32_t k0 = 0; k0 < n; k0 += 64u * 32u) {
        uint32_t k = k0 + lane * 32u;
        if (k < n) {
            const Win32 tw = win32(T, st + (int32_t)k), qw = win32(Q, sq + (int32_t)k);
            uint32_t bad = (tw.lo ^ qw.lo) | (tw.hi ^ qw.hi) | tw.nm | qw.nm;
            uint32_t rem = n - k, mask = rem < 32 ? (1u << rem) - 1u : 0xFFFFFFFFu;
            if (bad & mask) ok = false;
            ncg += __popc((tw.lo ^ tw.hi) & mask);
        }
        if (__ballot(!ok)) break;
    }
    if (__ballot(!ok)) return false;
    for (int o = 32; o > 0; o >>= 1) ncg += __shfl_xor(ncg, o);
    const uint64_t sc = 100ull * ncg + 91ull * ((uint64_t)n - ncg);
    out.score = (int32_t)(uint32_t)sc; out.maxcols = (uint32_t)(sc >> 32); out.i = n; out.j = n; out.nm = n; out.nx = 0;
    return true;
}

// The 2048-column kernel: one-sided y-drop affine extension by one wavefront (all lanes return the same result), 32 columns
// per lane, unpacked counts, no limit on the rows.
__device__ HalfResult wave_half_extend_2048(const GStrandView &T, const GStrandView &Q, uint32_t at, uint32_t aq, int dir,
                                            int32_t O, int32_t E, int32_t Y, int32_t cap) {
    constexpr int WSTRIP = 32, WINDOW = 64 * WSTRIP;  // columns per lane, columns in the sliding window
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lenA = dir > 0 ? T.len - at : at, lenB = dir > 0 ? Q.len - aq : aq;
    HalfResult best{0, 0, 0, 0, 0, 0, 0, 0};
    if (identical_suffix(T, Q, at, aq, dir, best)) return best;
    // ---- general row-by-row DP.  Lane l owns columns wb + 32*l .. wb + 32*l + 31 (rank == lane); when
    // the first live column crosses a strip boundary the whole state moves down by that many lanes.
    int32_t Cs[WSTRIP], Ds[WSTRIP];
    uint32_t Cm[WSTRIP], Cx[WSTRIP], Dm[WSTRIP], Dx[WSTRIP];
    uint32_t wb = 0, jb = lane * WSTRIP;
    uint32_t qlo, qhi, qn;
    load_qbits<WSTRIP>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
    bool over = false;
#pragma unroll
    for (int s = 0; s < WSTRIP; s++) {
        uint32_t j = jb + s;
        int32_t v = j ? -O - (int32_t)j * E : 0;
        bool alive = j <= lenB && (j == 0 || v >= -Y);
        Cs[s] = alive ? v : NEG; Cm[s] = 0; Cx[s] = 0;
        Ds[s] = NEG; Dm[s] = 0; Dx[s] = 0;
        if (alive && j >= WINDOW - WSTRIP) over = true;
    }
    if (__ballot(over)) { best.overflow = 1; return best; }
    RowBases rbase{0, 0, 0}, rnext = load_row_bases(T, at, dir, 1u);
    for (uint32_t i = 1; i <= lenA; i++) {
        const int32_t thr = best.score - Y;
        const uint32_t rbit = (i - 1u) & 31u;
        if (rbit == 0) { rbase = rnext; rnext = load_row_bases(T, at, dir, i + 32u); }
        const uint32_t alo = (rbase.lo >> rbit) & 1u, ahi = (rbase.hi >> rbit) & 1u, an = (rbase.nm >> rbit) & 1u, acg = alo ^ ahi;
        // C of the column left of my strip (previous row): last slot of the previous lane
        const Cell p7 = dpp_cell<0x138, 0xf>(Cell{Cs[WSTRIP - 1], Cm[WSTRIP - 1], Cx[WSTRIP - 1]});
        // pass 1 (slots descending, in place): D(i,j) and H(i,j) = max(diagonal, D) overwrite the
        // previous row's D and C; slot s still sees the old C of slot s-1
#pragma unroll
        for (int s = WSTRIP - 1; s >= 0; s--) {
            const uint32_t j = jb + s;
            const bool exists = j <= lenB;
            Cell dd{NEG, 0, 0}, g{NEG, 0, 0};
            if (Ds[s] > NEGH) { dd.s = Ds[s] - E; dd.nm = Dm[s]; dd.nx = Dx[s]; }
            if (Cs[s] > NEGH && Cs[s] - O - E > dd.s) { dd.s = Cs[s] - O - E; dd.nm = Cm[s]; dd.nx = Cx[s]; }
            Cell pc = s ? Cell{Cs[s ? s - 1 : 0], Cm[s ? s - 1 : 0], Cx[s ? s - 1 : 0]} : p7;
            if (pc.s > NEGH && j >= 1) {
                uint32_t dl = alo ^ ((qlo >> s) & 1u), dh = ahi ^ ((qhi >> s) & 1u), nn = an | ((qn >> s) & 1u);
                bool m = !(dl | dh | nn);
                g.s = pc.s + sub_score(dl, dh, acg, nn);
                g.nm = pc.nm + (m ? 1u : 0u);
                g.nx = pc.nx + (m ? 0u : 1u);
            }
            if (!exists) { dd.s = NEG; g.s = NEG; }
            Ds[s] = dd.s; Dm[s] = dd.nm; Dx[s] = dd.nx;
            Cell hh = g;  // diagonal preferred on ties
            if (dd.s > g.s) hh = dd;
            Cs[s] = hh.s; Cm[s] = hh.nm; Cx[s] = hh.nx;
        }
        // pass 2: insertion state = exclusive max-plus scan of u_k = H_k + (k - wb) * E along the
        // row: lane aggregate, then one cross-lane scan
        Cell run{NEG, 0, 0};
#pragma unroll
        for (int s = 0; s < WSTRIP; s++) {
            Cell u{Cs[s] > NEGH ? Cs[s] + (int32_t)(lane * WSTRIP + s) * E : NEG, Cm[s], Cx[s]};
            run = cmax_left(run, u);
        }
        Cell acc = dpp_cell<0x138, 0xf>(wave_incl_maxscan(run));  // best u of every column left of my strip
        // pass 3: C = max(H, I), prune, row statistics
        uint32_t amask = 0;
        Best4 rb{NEG, 0xFFFFFFFFu, 0, 0};
#pragma unroll
        for (int s = 0; s < WSTRIP; s++) {
            Cell hh{Cs[s], Cm[s], Cx[s]};
            Cell I{NEG, acc.nm, acc.nx};
            if (acc.s > NEGH) I.s = acc.s - O - (int32_t)(lane * WSTRIP + s) * E;
            Cell u{hh.s > NEGH ? hh.s + (int32_t)(lane * WSTRIP + s) * E : NEG, hh.nm, hh.nx};
            acc = cmax_left(acc, u);
            Cell c = hh;  // H preferred over I on ties
            if (I.s > c.s) c = I;
            const bool alive = (jb + s <= lenB) && c.s >= thr && c.s > NEGH;
            Cs[s] = alive ? c.s : NEG; Cm[s] = c.nm; Cx[s] = c.nx;
            if (!alive) Ds[s] = NEG;
            if (alive) {
                amask |= 1u << s;
                if (c.s > rb.s) { rb.s = c.s; rb.j = jb + s; rb.nm = c.nm; rb.nx = c.nx; }
            }
        }
        const uint64_t ball = __ballot(amask != 0);
        if (!ball) break;
        const uint32_t rf = (uint32_t)__builtin_ctzll(ball), rl = 63u - (uint32_t)__builtin_clzll(ball);
        if (rl == 63u) { best.overflow = 1; break; }
        best.maxcols = max(best.maxcols, (rl + 1u) * WSTRIP);
        best.rows = i;
        // best cell of the row (only when some lane beats the best of the rows above)
        if (__ballot(rb.s > best.score)) {
            const Best4 t = wave_best(rb);
            if (t.s > best.score) { best.score = t.s; best.i = i; best.j = t.j; best.nm = t.nm; best.nx = t.nx; }
            // 32-bit cells and no limit on the rows here: a half extension that nears 2^31 (20 Mbp of near-identity without a
            // break) goes on to k6_dp_any, which rebases its cells
            if (best.score > cap) { best.overflow = 1; break; }
        }
        // slide the window so that it starts at the strip holding the first live column
        const uint32_t fmask = (uint32_t)__builtin_amdgcn_readlane((int)amask, (int)rf);
        const uint32_t plo = wb + rf * WSTRIP + (uint32_t)__builtin_ctz(fmask);
        const uint32_t nwb = plo & ~(uint32_t)(WSTRIP - 1);
        if (nwb != wb) {
            const uint32_t shift = (nwb - wb) / WSTRIP;  // == rf
            wb = nwb;
            jb = wb + lane * WSTRIP;
            const int src = (int)((lane + shift) & 63u);
            const bool fresh = lane + shift >= 64u;  // strip re-enters on the right with new columns
#pragma unroll
            for (int s = 0; s < WSTRIP; s++) {
                int32_t cs = __shfl(Cs[s], src), ds = __shfl(Ds[s], src);
                Cm[s] = __shfl(Cm[s], src); Cx[s] = __shfl(Cx[s], src);
                Dm[s] = __shfl(Dm[s], src); Dx[s] = __shfl(Dx[s], src);
                Cs[s] = fresh ? NEG : cs;
                Ds[s] = fresh ? NEG : ds;
            }
            uint32_t a0 = __shfl(qlo, src), a1 = __shfl(qhi, src), a2 = __shfl(qn, src);
            if (fresh) load_qbits<WSTRIP>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
            else { qlo = a0; qhi = a1; qn = a2; }
        }
    }
    return best;
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
            uint32_t lo = 0, hi = n;   // first block that starts above t
            while (lo < hi) {
                const uint32_t mid = (lo + hi) >> 1;
                if ((long long)blk[mid].t <= t) lo = mid + 1; else hi = mid;
            }
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

// ---- lean single-wavefront DP (k6_dp1): the production kernel -----------------------------------------------
// Same recurrences, pruning and tie-breaks as wave_half_extend_2048 (one wavefront, a strip of columns per lane, a window
// that slides by whole strips), written for VALU issue, which is what bounds K6 (profiles/r02_*: that kernel's form spent
// 1700+ issue slots per DP row at 16 columns per lane):
//   * counts packed into one word (PCell), 16 bits each: one select instead of two, a third less to scan and exchange
//     per cell.  They grow by one per row at most, so rows < 65535 cannot overflow them; a longer half extension is redone
//     by the 2048-column kernel (unpacked);
//   * no liveness guards: a dead cell is any value below NEGH, arithmetic on it stays below NEGH for the one row
//     until pruning resets it to NEG, so max / compare need no special cases;
//   * the substitution score of a cell is ONE v_perm_b32: the row's target base is wave-uniform, so the four
//     possible scores (+128, as bytes) sit in a scalar register and the column's query base is a precomputed byte
//     selector (selector 4 = the constant 28 = -100 + 128 of an N column; an N row is the table 0x1C1C1C1C);
//   * the insertion state is carried in the frame of the current column (acc = max(acc, H) - E) instead of
//     u_k = H_k + k E: no per-column constants; lanes are stitched with one max-scan of (aggregate + lane * 14 E);
//   * per cell the row maximum is one v_max; which cell it was (smallest column on ties) is found with scalar
//     reads only in rows that improve the best score; liveness is per strip (row maximum above NEGH), which is
//     all the window slide and the overflow test ever needed;
//   * columns beyond the end of the query only exist when the window touches it: rows of such windows run the
//     EDGE variant (one extra mask test per cell), selected wave-uniformly.
// Measured: ~40 VALU instructions per cell.  Strips of 14 columns (896-column window): the widest live band of a
// default-parameter extension is ~600 + 2 strips (y-drop 9400 / gap extend 30 on either side of the best cell; C4: all
// below 768), and a band that does not fit is redone by the 2048-column kernel.
constexpr int L_WS = 14, L_WINDOW = 64 * L_WS;
struct LeanState {
    int32_t C[L_WS], D[L_WS];
    uint32_t Cc[L_WS], Dc[L_WS], sel[L_WS];
};
// a cell of the lean kernel as it moves between lanes: score and packed counts (matches | diagonal steps << 16)
struct PCell {
    int32_t s;
    uint32_t c;
};
__device__ __forceinline__ PCell pcmax_left(const PCell &l, const PCell &r) { return r.s > l.s ? r : l; }  // ties -> left
template <int CTRL, int RMASK>
__device__ __forceinline__ PCell dpp_pcell(const PCell &c) {
    PCell o;  // lanes without a valid source keep the identity (NEG, 0), as dpp_cell
    o.s = __builtin_amdgcn_update_dpp(NEG, c.s, CTRL, RMASK, 0xf, false);
    o.c = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)c.c, CTRL, RMASK, 0xf, false);
    return o;
}

__device__ __forceinline__ int32_t wave_max_i32(int32_t v) {
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x111, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x112, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x114, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x118, 0xf, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x142, 0xa, 0xf, false));
    v = max(v, __builtin_amdgcn_update_dpp(INT32_MIN, v, 0x143, 0xc, 0xf, false));
    return __builtin_amdgcn_readlane(v, 63);
}

// inclusive max-scan, ties to the lower lane; a lane without a source sees its own value (no identity moves)
template <int CTRL, int RMASK>
__device__ __forceinline__ PCell lean_scan_step(const PCell &v) {
    PCell o;
    o.s = __builtin_amdgcn_update_dpp(v.s, v.s, CTRL, RMASK, 0xf, false);
    o.c = (uint32_t)__builtin_amdgcn_update_dpp((int)v.c, (int)v.c, CTRL, RMASK, 0xf, false);
    return pcmax_left(o, v);
}
__device__ __forceinline__ PCell lean_incl_maxscan(PCell v) {
    v = lean_scan_step<0x111, 0xf>(v);
    v = lean_scan_step<0x112, 0xf>(v);
    v = lean_scan_step<0x114, 0xf>(v);
    v = lean_scan_step<0x118, 0xf>(v);
    v = lean_scan_step<0x142, 0xa>(v);
    v = lean_scan_step<0x143, 0xc>(v);
    return v;
}

// byte selectors of a strip from its query bits: 0..3 = base code (lo | hi << 1), 4 = N; upper bytes select zero
__device__ __forceinline__ void lean_selectors(LeanState &S, uint32_t qlo, uint32_t qhi, uint32_t qn) {
#pragma unroll
    for (int s = 0; s < L_WS; s++) {
        const uint32_t idx = ((qlo >> s) & 1u) | (((qhi >> s) & 1u) << 1);
        S.sel[s] = 0x0C0C0C00u | (((qn >> s) & 1u) ? 4u : idx);
    }
}

// one DP row; returns the lane's row maximum (NEG when none of its cells is live).  BND (bounded extension, with EDGE):
// exmask also clears the slots outside the row's allowed interval, and their H is dead before the insertion pass: the
// forbidden cells are a prefix and a suffix of the row, so H masked after pass 1 and C / D after pass 3 is the rule
template <bool EDGE, bool BND = false>
__device__ __forceinline__ int32_t lean_row(LeanState &S, uint32_t srow, int32_t O, int32_t E, int32_t thr, uint32_t exmask,
                                            int32_t lane_base, int32_t kneg128) {
    const int32_t OE = O + E;
    // C of the column left of my strip (previous row): last slot of the previous lane
    PCell pc = dpp_pcell<0x138, 0xf>(PCell{S.C[L_WS - 1], S.Cc[L_WS - 1]});
    // pass 1 (slots descending, in place): D and H = max(diagonal, D); slot s still sees the old C of slot s - 1
#pragma unroll
    for (int s = L_WS - 1; s >= 0; s--) {
        const int32_t t1 = S.D[s] - E, t2 = S.C[s] - OE;
        const bool open = t2 > t1;
        const int32_t ds = max(t1, t2);
        const uint32_t dc = open ? S.Cc[s] : S.Dc[s];
        const PCell left = s ? PCell{S.C[s ? s - 1 : 0], S.Cc[s ? s - 1 : 0]} : pc;
        const uint32_t scb = __builtin_amdgcn_perm(28u, srow, S.sel[s]);   // score + 128
        const int32_t gs = left.s + (int32_t)scb + kneg128;
        const uint32_t gc = left.c + 0x10000u + ((int32_t)scb > 128 ? 1u : 0u);   // diagonal steps << 16 | matches
        const bool vert = ds > gs;  // diagonal preferred on ties
        S.D[s] = ds; S.Dc[s] = dc;
        S.C[s] = max(gs, ds);
        if (BND) S.C[s] = ((exmask >> s) & 1u) ? S.C[s] : NEG;
        S.Cc[s] = vert ? dc : gc;
    }
    // pass 2: the strip's aggregate of the insertion state as it arrives at the first column of the next strip
    PCell run{NEG, 0};
#pragma unroll
    for (int s = 0; s < L_WS; s++) {
        const bool take = S.C[s] > run.s;  // ties -> left
        run.c = take ? S.Cc[s] : run.c;
        run.s = max(run.s, S.C[s]) - E;
    }
    run.s += lane_base;  // common frame: column 0 of the window
    PCell acc = dpp_pcell<0x138, 0xf>(lean_incl_maxscan(run));  // best of every column left of my strip
    acc.s += L_WS * E - lane_base;                                   // ... as it arrives at my first column
    // pass 3: C = max(H, I), prune, row maximum
    int32_t rowmax = NEG;
#pragma unroll
    for (int s = 0; s < L_WS; s++) {
        const int32_t hs = S.C[s];
        const uint32_t hc = S.Cc[s];
        const int32_t is = acc.s - O;
        const bool ins = is > hs;       // H preferred over I on ties
        const int32_t cs = max(hs, is);
        const uint32_t cc = ins ? acc.c : hc;
        const bool take = hs > acc.s;   // ties -> left
        acc.c = take ? hc : acc.c;
        acc.s = max(acc.s, hs) - E;
        bool alive = cs >= thr;
        if (EDGE) alive = alive && ((exmask >> s) & 1u);
        S.C[s] = alive ? cs : NEG; S.Cc[s] = cc;
        S.D[s] = alive ? S.D[s] : NEG;
        rowmax = max(rowmax, S.C[s]);
    }
    return rowmax;
}

// BOUND: the extension is bounded by the group's nacc accepted alignments (bounds_at); *sw receives what it swept
template <bool BOUND>
__device__ HalfResult wave_half_extend_lean(const GStrandView &T, const GStrandView &Q, uint32_t at, uint32_t aq, int dir,
                                            int32_t O, int32_t E, int32_t Y, const BoundCtx &B, uint64_t b0, uint32_t nacc,
                                            HalfSweep *sw) {
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lenA = dir > 0 ? T.len - at : at, lenB = dir > 0 ? Q.len - aq : aq;
    HalfResult best{0, 0, 0, 0, 0, 0, 0, 0};
    if (BOUND) *sw = HalfSweep{0, 0, nacc, 0};
    // a bounded half may take the exact shortcut only when no earlier alignment reaches into its rows
    if ((!BOUND || bounds_none(B, b0, nacc, at, dir)) && identical_suffix(T, Q, at, aq, dir, best)) return best;
    // biased score bytes of the four query bases for each target base (index lo | hi << 1)
    uint32_t tab[4];
#pragma unroll
    for (uint32_t a = 0; a < 4; a++) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t alo = a & 1u, ahi = a >> 1, dl = alo ^ (b & 1u), dh = ahi ^ (b >> 1);
            w |= (uint32_t)(sub_score(dl, dh, alo ^ ahi, 0u) + 128) << (8u * b);
        }
        tab[a] = w;
    }
    LeanState S;
    uint32_t wb = 0, jb = lane * L_WS;
    {
        uint32_t qlo, qhi, qn;
        load_qbits<L_WS>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
        lean_selectors(S, qlo, qhi, qn);
    }
    bool over = false;
#pragma unroll
    for (int s = 0; s < L_WS; s++) {
        const uint32_t j = jb + s;
        const int32_t v = j ? -O - (int32_t)j * E : 0;
        const bool alive = j <= lenB && (j == 0 || v >= -Y);
        S.C[s] = alive ? v : NEG; S.Cc[s] = 0;
        S.D[s] = NEG; S.Dc[s] = 0;
        if (alive && j >= (uint32_t)(L_WINDOW - L_WS)) over = true;
    }
    if (__ballot(over)) { best.overflow = 1; return best; }
    const int32_t lane_base = (int32_t)(lane * L_WS) * E;
    const int32_t kneg128 = __builtin_amdgcn_readfirstlane(-128);
    uint32_t exmask = (1u << L_WS) - 1u;
    bool edge = wb + (uint32_t)L_WINDOW - 1u > lenB;
    if (edge) {
        exmask = 0;
#pragma unroll
        for (int s = 0; s < L_WS; s++) exmask |= (jb + s <= lenB ? 1u : 0u) << s;
    }
    long long bkmin = -K_INF, bkmax = K_INF;   // BOUND: the allowed interval of k = j - i, and the row where it is looked up again
    uint32_t bnext = 1u;
    int32_t klo = INT32_MAX, khi = INT32_MIN;
    RowBases rbase{0, 0, 0}, rnext = load_row_bases(T, at, dir, 1u);
    for (uint32_t i = 1; i <= lenA; i++) {
        // the packed counts hold 16 bits each: a longer extension is redone by the wide kernel (unpacked counts)
        if (i >= 0xFFFFu) { best.overflow = 1; break; }
        if (BOUND && i == bnext) {
            const RowBound rb = bounds_at(B, b0, nacc, at, aq, dir, i);
            bkmin = rb.kmin; bkmax = rb.kmax; bnext = rb.next;
        }
        const int32_t thr = best.score - Y;
        const uint32_t rbit = (i - 1u) & 31u;
        if (rbit == 0) { rbase = rnext; rnext = load_row_bases(T, at, dir, i + 32u); }
        const uint32_t rlo = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbase.lo), rhi = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbase.hi),
                       rnm = (uint32_t)__builtin_amdgcn_readfirstlane((int)rbase.nm);
        const uint32_t a = ((rlo >> rbit) & 1u) | (((rhi >> rbit) & 1u) << 1);
        uint32_t srow = a & 2u ? (a & 1u ? tab[3] : tab[2]) : (a & 1u ? tab[1] : tab[0]);
        if ((rnm >> rbit) & 1u) srow = 0x1C1C1C1Cu;
        // BOUND: the allowed columns of this row are jlo .. jhi; only rows in which they cut the window run the masked variant
        uint32_t bm = 0;
        bool cut = false;
        if (BOUND) {
            const long long jlo = bkmin + (long long)i + 1, jhi = bkmax + (long long)i - 1;
            if (bkmin > -K_INF || bkmax < K_INF) sw->nbound++;
            cut = jlo > (long long)wb || jhi < (long long)wb + (L_WINDOW - 1);
            const long long r0 = jlo - (long long)jb, r1 = jhi - (long long)jb + 1;
            const uint32_t s0 = (uint32_t)min(max(r0, 0ll), (long long)L_WS), s1 = (uint32_t)min(max(r1, 0ll), (long long)L_WS);
            bm = ((1u << s1) - 1u) & ~((1u << s0) - 1u) & exmask;   // exmask: all slots, or those within the query
        }
        const int32_t rowmax = BOUND && cut ? lean_row<true, true>(S, srow, O, E, thr, bm, lane_base, kneg128)
                               : edge ? lean_row<true>(S, srow, O, E, thr, exmask, lane_base, kneg128)
                                      : lean_row<false>(S, srow, O, E, thr, exmask, lane_base, kneg128);
        const uint64_t ball = __ballot(rowmax > NEGH);
        if (!ball) break;
        const uint32_t rf = (uint32_t)__builtin_ctzll(ball), rl = 63u - (uint32_t)__builtin_clzll(ball);
        if (rl == 63u) { best.overflow = 1; break; }
        best.maxcols = max(best.maxcols, (rl + 1u) * L_WS);
        best.rows = i;
        if (BOUND) {   // the strips with a live cell, as diagonals of this row
            klo = min(klo, (int32_t)((long long)wb + rf * L_WS - (long long)i));
            khi = max(khi, (int32_t)((long long)wb + (rl + 1u) * L_WS - 1 - (long long)i));
        }
        const int32_t wmax = wave_max_i32(rowmax);
        if (wmax > best.score) {
            // the cell: lowest lane holding the maximum, smallest slot in it (smallest column on ties)
            const uint32_t L = (uint32_t)__builtin_ctzll(__ballot(rowmax == wmax));
            uint32_t slot = 0, cnt = 0;
#pragma unroll
            for (int s = L_WS - 1; s >= 0; s--) {
                const int32_t v = __builtin_amdgcn_readlane(S.C[s], (int)L);
                if (v == wmax) { slot = (uint32_t)s; cnt = (uint32_t)__builtin_amdgcn_readlane((int)S.Cc[s], (int)L); }
            }
            best.score = wmax; best.i = i; best.j = wb + L * L_WS + slot; best.nm = cnt & 0xFFFFu; best.nx = (cnt >> 16) - (cnt & 0xFFFFu);
        }
        // slide the window so that it starts at the strip holding the first live column
        if (rf) {
            wb += rf * L_WS;
            jb = wb + lane * L_WS;
            const int src = (int)((lane + rf) & 63u);
            const bool fresh = lane + rf >= 64u;  // strip re-enters on the right with new columns
#pragma unroll
            for (int s = 0; s < L_WS; s++) {
                const int32_t cs = __shfl(S.C[s], src), ds = __shfl(S.D[s], src);
                S.Cc[s] = __shfl(S.Cc[s], src); S.Dc[s] = __shfl(S.Dc[s], src);
                S.sel[s] = __shfl(S.sel[s], src);
                S.C[s] = fresh ? NEG : cs;
                S.D[s] = fresh ? NEG : ds;
            }
            if (fresh) {
                uint32_t qlo, qhi, qn;
                load_qbits<L_WS>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
                lean_selectors(S, qlo, qhi, qn);
            }
            edge = wb + (uint32_t)L_WINDOW - 1u > lenB;
            if (edge) {
                exmask = 0;
#pragma unroll
                for (int s = 0; s < L_WS; s++) exmask |= (jb + s <= lenB ? 1u : 0u) << s;
            } else if (BOUND) exmask = (1u << L_WS) - 1u;
        }
    }
    if (BOUND) { sw->klo = klo; sw->khi = khi; }
    return best;
}

__global__ __launch_bounds__(64) void k6_dp1(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                             HalfResult *__restrict__ res, int32_t O, int32_t E, int32_t Y) {
    const DpJob job = jobs[blockIdx.x];
    const Group &G = groups[job.group];
    HalfResult r = wave_half_extend_lean<false>(G.T, G.Q, job.at, job.aq, job.dir, O, E, Y, BoundCtx{}, 0, 0, nullptr);
    if (threadIdx.x == 0) res[job.slot] = r;
}

// k6_dp1 under mimeo_params.bound_extensions.  A half that does not fit (band, rows) goes on to k6_dp_any<true>
__global__ __launch_bounds__(64) void k6_dp1_bounded(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                     HalfResult *__restrict__ res, HalfSweep *__restrict__ sweep, int32_t O, int32_t E,
                                                     int32_t Y, BoundCtx B, unsigned int *__restrict__ novf,
                                                     unsigned int *__restrict__ ovf_list) {
    const DpJob job = jobs[blockIdx.x];
    const Group &G = groups[job.group];
    HalfSweep sw;
    HalfResult r = wave_half_extend_lean<true>(G.T, G.Q, job.at, job.aq, job.dir, O, E, Y, B, G.hsp_begin, G.nacc, &sw);
    if (threadIdx.x == 0) {
        res[job.slot] = r;
        sweep[job.slot] = sw;
        if (r.overflow) ovf_list[atomicAdd(novf, 1u)] = blockIdx.x;
    }
}

// Anchor = centre of the best 31-column window of the HSP (first maximum).  Windows are cut into
// chunks of ANCHOR_CHUNK starts; a wave scans one chunk (each lane slides over 64 consecutive
// starts) and folds its best (sum, start) into a packed 64-bit word with atomicMax — high half
// = biased sum, low half = ~start, so the maximum is the highest sum at the smallest start.
constexpr uint32_t ANCHOR_W = 31, ANCHOR_CHUNK = 4096;
constexpr int ANCHOR_THREADS = 1024;

__device__ void wave_anchor_chunk(const GStrandView &T, const GStrandView &Q, const mimeo_hsp &h, uint32_t chunk,
                                  unsigned long long *packed) {
    const uint32_t lane = threadIdx.x & 63u, nw = h.length - ANCHOR_W + 1;
    const int32_t d = (int32_t)h.tstart - (int32_t)h.qstart;
    const uint32_t w0 = chunk * ANCHOR_CHUNK + lane * (ANCHOR_CHUNK / 64u), w1 = min(nw, w0 + ANCHOR_CHUNK / 64u);
    int32_t bs = INT32_MIN;
    uint32_t bw = 0xFFFFFFFFu;
    if (w0 < w1) {
        int32_t sum = 0;
        bool m;
        for (uint32_t k = 0; k < ANCHOR_W; k++) {
            int32_t pt = (int32_t)(h.tstart + w0 + k);
            sum += pair_score(T, Q, pt, pt - d, &m);
        }
        bs = sum; bw = w0;
        for (uint32_t w = w0 + 1; w < w1; w++) {
            int32_t add = (int32_t)(h.tstart + w + ANCHOR_W - 1), sub = (int32_t)(h.tstart + w - 1);
            sum += pair_score(T, Q, add, add - d, &m) - pair_score(T, Q, sub, sub - d, &m);
            if (sum > bs) { bs = sum; bw = w; }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        int32_t ob = __shfl_xor(bs, o);
        uint32_t ow = __shfl_xor(bw, o);
        if (ob > bs || (ob == bs && ow < bw)) { bs = ob; bw = ow; }
    }
    if (lane == 0 && bw != 0xFFFFFFFFu)
        atomicMax(packed, ((unsigned long long)(uint32_t)(bs + 8192) << 32) | (unsigned long long)(0xFFFFFFFFu - bw));
}

// packed[b0 + r] = best window of the r-th chained HSP of the group.  ANCHOR_SPLIT workgroups of 16
// wavefronts share the (HSP, chunk) items of a group round-robin (the 5 Mbp self HSP alone has 1220
// chunks); k6_anchor_final turns the packed maxima into anchor points.
constexpr uint32_t ANCHOR_SPLIT = 16;
__global__ __launch_bounds__(ANCHOR_THREADS) void k6_anchor_points(const Group *__restrict__ groups,
                                                                   const mimeo_hsp *__restrict__ hs,
                                                                   const uint32_t *__restrict__ order,
                                                                   unsigned long long *__restrict__ packed) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nw = gridDim.y * (ANCHOR_THREADS / 64), me = blockIdx.y * (ANCHOR_THREADS / 64) + (threadIdx.x >> 6);
    uint32_t item = 0;
    for (uint32_t r = 0; r < G.nchain; r++) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        if (h.length <= ANCHOR_W) continue;
        const uint32_t nch = (h.length - ANCHOR_W + 1 + ANCHOR_CHUNK - 1) / ANCHOR_CHUNK;
        // my chunks of this HSP: c = first, first + nw, ...
        const uint32_t first = (me + nw - item % nw) % nw;
        for (uint32_t c = first; c < nch; c += nw) wave_anchor_chunk(G.T, G.Q, h, c, &packed[b0 + r]);
        item += nch;
    }
}
__global__ __launch_bounds__(256) void k6_anchor_final(const Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs,
                                                       const uint32_t *__restrict__ order,
                                                       const unsigned long long *__restrict__ packed,
                                                       uint2 *__restrict__ anchors) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    for (uint32_t r = threadIdx.x; r < G.nchain; r += blockDim.x) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        uint32_t off = h.length / 2;
        if (h.length > ANCHOR_W) off = (0xFFFFFFFFu - (uint32_t)packed[b0 + r]) + ANCHOR_W / 2;
        anchors[b0 + r] = make_uint2(h.tstart + off, h.qstart + off);
    }
}

__device__ __forceinline__ bool in_boxes(const mimeo_alignment *aln, uint32_t n, uint2 a) {
    // wave-cooperative: is the anchor inside the box of any of the n earlier alignments?
    bool inside = false;
    for (uint32_t e = threadIdx.x & 63u; e < n; e += 64u) {
        const mimeo_alignment &o = aln[e];
        if (a.x >= o.tstart && a.x < o.tend && a.y >= o.qstart && a.y < o.qend) inside = true;
    }
    return __ballot(inside) != 0;
}

// ---- path rule (MIMEO_ANCHOR_PATH) ------------------------------------------------------------------------------
// The path of an alignment = its diagonal (match / mismatch) steps from both halves, kept as gap-free blocks (t, q, len)
// sorted by t.  A half's diagonal steps have distinct t (each consumes one target base) and the left half lies below the
// anchor's t, the right half at or above it, so one binary search per half decides whether (t, q) is on the path.
// (PathBlock / PathView are defined further up, ahead of the bounded DP that reads them.)
__device__ __forceinline__ bool on_half_path(const PathBlock *blk, uint32_t n, uint2 a) {
    uint32_t lo = 0, hi = n;  // first block with t > a.x
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (blk[mid].t <= a.x) lo = mid + 1; else hi = mid;
    }
    if (!lo) return false;
    const PathBlock b = blk[lo - 1];
    return a.x - b.t < b.len && a.y >= b.q && a.y - b.q == a.x - b.t;
}
// is anchor a on the path of the alignment of the anchor of rank `rank` (group hsp_begin b0)?
__device__ __forceinline__ bool on_path(const PathView &P, const uint2 *anchors, uint64_t b0, uint32_t rank, uint2 a) {
    const uint2 an = anchors[b0 + rank];
    const uint2 ix = P.pidx[2u * (b0 + rank) + (a.x >= an.x ? 1u : 0u)];
    if (ix.x == PATH_UNTRACED) return false;
    return on_half_path(P.blk + ix.x, ix.y, a);
}
// the skip test of the rule in force against the n accepted alignments aln[b0 ..]: the box is a prefilter of the path
template <bool PATH>
__device__ __forceinline__ bool skip_test(const mimeo_alignment *aln, uint32_t n, uint2 a, const PathView &P,
                                          const uint2 *anchors, uint64_t b0) {
    if (!PATH) return in_boxes(aln + b0, n, a);
    bool on = false;
    for (uint32_t e = threadIdx.x & 63u; e < n; e += 64u) {
        const mimeo_alignment &o = aln[b0 + e];
        if (a.x >= o.tstart && a.x < o.tend && a.y >= o.qstart && a.y < o.qend && on_path(P, anchors, b0, P.accrank[b0 + e], a))
            on = true;
    }
    return __ballot(on) != 0;
}

// Anchor states.  The skip rule is ordered (an anchor is skipped iff it lies in the box of an ACCEPTED
// anchor of lower rank), so anchors are finalised strictly in rank order by k6_resolve; what k6_pick
// may choose freely is which unfinalised anchors get their DP in this round.  Fragments of one repeat
// copy sit on neighbouring diagonals within a few kb and only the best-ranked one survives, so an
// anchor that is NEAR a lower-ranked anchor whose DP is pending is deferred (twice at most): in the
// next round it is normally inside that anchor's accepted box and never costs a DP.
enum : uint8_t { A_NEW = 0, A_DONE = 1, A_SKIPPED = 2, A_ACCEPTED = 3 };
constexpr uint32_t PICK_SCAN = 512;   // ranks looked at per round, from the first unfinalised one
constexpr uint32_t NEAR_DIAG = 256, NEAR_POS = 8192, MAX_DEFER = 2;

__device__ __forceinline__ bool anchors_near(uint2 a, uint2 b) {
    int32_t da = (int32_t)a.x - (int32_t)a.y, db = (int32_t)b.x - (int32_t)b.y;
    uint32_t dd = (uint32_t)abs(da - db), dp = a.x > b.x ? a.x - b.x : b.x - a.x;
    return dd <= NEAR_DIAG && dp <= NEAR_POS;
}

// one wave per group; PATH: the skip test is the path rule (P is unused otherwise)
template <bool PATH>
__global__ __launch_bounds__(64) void k6_pick(Group *__restrict__ groups, const uint2 *__restrict__ anchors,
                                              const mimeo_alignment *__restrict__ aln, uint32_t bmax,
                                              uint8_t *__restrict__ astate, uint8_t *__restrict__ adefer,
                                              DpJob *__restrict__ jobs, unsigned int *__restrict__ njobs, PathView P) {
    __shared__ uint32_t sb[MAX_BATCH];  // ranks scheduled in this round
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t first = G.next, lane = threadIdx.x;
    uint32_t nb = 0;
    for (uint32_t r = first; r < G.nchain && nb < bmax && r - first < PICK_SCAN; r++) {
        if (astate[b0 + r] != A_NEW) continue;  // wave-uniform; states of earlier rounds only
        const uint2 a = anchors[b0 + r];
        if (skip_test<PATH>(aln, G.nacc, a, P, anchors, b0)) {
            if (lane == 0) astate[b0 + r] = A_SKIPPED;
            continue;
        }
        // near an unfinalised lower-ranked anchor whose DP is done (earlier rounds) or scheduled (this round)?
        bool susp = false;
        for (uint32_t r2 = first + lane; r2 < r; r2 += 64)
            if (astate[b0 + r2] == A_DONE && anchors_near(a, anchors[b0 + r2])) susp = true;
        if (lane < nb && anchors_near(a, anchors[b0 + sb[lane]])) susp = true;
        if (__ballot(susp) && adefer[b0 + r] < MAX_DEFER) {
            if (lane == 0) adefer[b0 + r]++;
            continue;
        }
        if (lane == 0) sb[nb] = r;
        nb++;
        __syncthreads();
    }
    if (lane == 0) {
        G.nbatch = nb;
        unsigned int j0 = nb ? atomicAdd(njobs, 2u * nb) : 0u;
        G.job0 = j0;
        for (uint32_t k = 0; k < nb; k++) {
            const uint32_t r = sb[k];
            astate[b0 + r] = A_DONE;
            const uint2 a = anchors[b0 + r];
            const uint32_t slot = 2u * (uint32_t)(b0 + r);
            jobs[j0 + 2 * k] = DpJob{blockIdx.x, a.x, a.y, -1, slot, 0};
            jobs[j0 + 2 * k + 1] = DpJob{blockIdx.x, a.x, a.y, +1, slot + 1, 0};
        }
    }
}

// second chance for half extensions that outgrew the lean kernel (band beyond its 896-column window, 65 535 rows): 2048
// columns.  every: all jobs of the round, not only the overflowed ones (penalties outside the lean kernel's domain)
__global__ __launch_bounds__(64) void k6_dp_wide(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                 HalfResult *__restrict__ res, int32_t O, int32_t E, int32_t Y,
                                                 unsigned int *__restrict__ novf, unsigned int *__restrict__ ovf_list, int32_t cap,
                                                 int every) {
    const DpJob job = jobs[blockIdx.x];
    if (!every && !res[job.slot].overflow) return;
    const Group &G = groups[job.group];
    HalfResult r = wave_half_extend_2048(G.T, G.Q, job.at, job.aq, job.dir, O, E, Y, cap);
    if (threadIdx.x == 0) {
        res[job.slot] = r;
        if (r.overflow) ovf_list[atomicAdd(novf, 1u)] = blockIdx.x;  // band beyond 2048 columns: k6_dp_any
    }
}

// ---- last resort: a half extension whose band does not fit 2048 columns (tandem arrays: every shift by a
// period scores almost as well, so the live band grows with the array).  One workgroup of 1024 threads, the DP
// rows in global memory as a ring of ANY_COLS columns (two rows: previous / current), three passes per row
// with the same rules and tie-breaks as wave_half_extend_2048.  Slow (a few microseconds per row plus ~1 ns per
// live cell) but exact; only jobs that overflowed the register kernels come here.
constexpr uint32_t ANY_COLS = 1u << 16;   // live band + one row's growth must stay below this
constexpr int ANY_THREADS = 1024;
struct AnyRow {  // one DP row in global memory, indexed by column & (ANY_COLS - 1)
    int32_t *cs, *ds;
    uint32_t *cm, *cx, *dm, *dx;
};
__device__ __forceinline__ AnyRow any_row(uint32_t *base, uint32_t parity) {
    uint32_t *b = base + (size_t)parity * 6u * ANY_COLS;
    return AnyRow{(int32_t *)b, (int32_t *)(b + ANY_COLS), b + 2u * ANY_COLS, b + 3u * ANY_COLS, b + 4u * ANY_COLS, b + 5u * ANY_COLS};
}
constexpr size_t ANY_SLOT_WORDS = 2u * 6u * (size_t)ANY_COLS;  // per job

// BOUND (mimeo_params.bound_extensions): cells outside the row's allowed interval (bounds_at) are dead in all three states
template <bool BOUND>
__global__ __launch_bounds__(ANY_THREADS) void k6_dp_any(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                         const unsigned int *__restrict__ list, uint32_t first,
                                                         HalfResult *__restrict__ res, uint32_t *__restrict__ scratch,
                                                         int32_t O, int32_t E, int32_t Y, int32_t cap, BoundCtx B,
                                                         HalfSweep *__restrict__ sweep) {
    __shared__ Cell s_scan[ANY_THREADS / 64];
    __shared__ Best4 s_best[ANY_THREADS / 64];
    __shared__ uint32_t s_first[ANY_THREADS / 64], s_last[ANY_THREADS / 64];
    const DpJob job = jobs[list[first + blockIdx.x]];
    const Group &G = groups[job.group];
    const GStrandView T = G.T, Q = G.Q;
    const uint32_t at = job.at, aq = job.aq;
    const int dir = job.dir;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t lenA = dir > 0 ? T.len - at : at, lenB = dir > 0 ? Q.len - aq : aq;
    uint32_t *base = scratch + (size_t)blockIdx.x * ANY_SLOT_WORDS;
    const uint32_t M = ANY_COLS - 1u;
    HalfResult best{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    long long sbase = 0;   // the cells are 32 bits wide and stand above this (below)
    // row 0: C(0,j) = -O - j*E while that is within the y-drop
    uint32_t lo = 0, hi = 0;
    if (Y >= O + E) hi = min(lenB, (uint32_t)((Y - O) / E));
    const uint32_t ext = (uint32_t)((Y + 200) / E) + 2u;  // how far an insertion can carry a live cell to the right
    bool overflow = min(lenB, hi + ext) + 2u >= ANY_COLS;   // no row can hold more live columns than the query has left
    {
        AnyRow r0 = any_row(base, 0);
        for (uint32_t j = tid; j <= hi && !overflow; j += ANY_THREADS) {
            r0.cs[j & M] = j ? -O - (int32_t)j * E : 0; r0.cm[j & M] = 0; r0.cx[j & M] = 0;
            r0.ds[j & M] = NEG; r0.dm[j & M] = 0; r0.dx[j & M] = 0;
        }
    }
    __syncthreads();
    uint32_t par = 0;
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nacc = BOUND ? G.nacc : 0u;
    long long bkmin = -K_INF, bkmax = K_INF;
    uint32_t bnext = 1u, nbound = 0;
    int32_t klo = INT32_MAX, khi = INT32_MIN;
    for (uint32_t i = 1; i <= lenA && !overflow; i++, par ^= 1u) {
        const AnyRow P = any_row(base, par), N = any_row(base, par ^ 1u);
        if (BOUND && i == bnext) {
            const RowBound rb = bounds_at(B, b0, nacc, at, aq, dir, i);
            bkmin = rb.kmin; bkmax = rb.kmax; bnext = rb.next;
        }
        if (BOUND && (bkmin > -K_INF || bkmax < K_INF)) nbound++;
        const long long jlo = bkmin + (long long)i + 1, jhi = bkmax + (long long)i - 1;   // the allowed columns
        const int32_t thr = best.score - Y;
        const int32_t pa = dir > 0 ? (int32_t)(at + i - 1) : (int32_t)(at - i);
        const Base1 ab = base_at(T, pa);
        const uint32_t alo = ab.lo, ahi = ab.hi, an = ab.nm, acg = alo ^ ahi;
        const uint32_t hx = min(lenB, hi + 1u + ext);  // last column that can be alive in this row
        const uint32_t ncols = hx - lo + 1u;
        if (ncols + 2u >= ANY_COLS) { overflow = true; break; }
        // every thread owns one contiguous chunk of the row's columns (the insertion scan runs left to right)
        const uint32_t chunk = (ncols + ANY_THREADS - 1) / ANY_THREADS;
        const uint32_t j0 = lo + tid * chunk, j1 = min(hx + 1u, j0 + chunk);  // [j0, j1), possibly empty
        // pass 1: D and H = max(diagonal, D) from the previous row (dead outside [lo, hi])
        Cell run{NEG, 0, 0};
        for (uint32_t j = j0; j < j1; j++) {
            const bool in = j <= hi;  // j >= lo holds
            const int32_t cp = in ? P.cs[j & M] : NEG, dp = in ? P.ds[j & M] : NEG;
            Cell dd{NEG, 0, 0}, g{NEG, 0, 0};
            if (dp > NEGH) { dd.s = dp - E; dd.nm = P.dm[j & M]; dd.nx = P.dx[j & M]; }
            if (cp > NEGH && cp - O - E > dd.s) { dd.s = cp - O - E; dd.nm = P.cm[j & M]; dd.nx = P.cx[j & M]; }
            if (j >= 1 && j - 1 >= lo && j - 1 <= hi) {
                const int32_t pc = P.cs[(j - 1) & M];
                if (pc > NEGH) {
                    const Base1 qb = base_at(Q, dir > 0 ? (int32_t)(aq + j - 1) : (int32_t)(aq - j));
                    const uint32_t dl = alo ^ qb.lo, dh = ahi ^ qb.hi, nn = an | qb.nm;
                    const bool m = !(dl | dh | nn);
                    g.s = pc + sub_score(dl, dh, acg, nn);
                    g.nm = P.cm[(j - 1) & M] + (m ? 1u : 0u);
                    g.nx = P.cx[(j - 1) & M] + (m ? 0u : 1u);
                }
            }
            if (BOUND && ((long long)j < jlo || (long long)j > jhi)) { dd.s = NEG; g.s = NEG; }
            N.ds[j & M] = dd.s; N.dm[j & M] = dd.nm; N.dx[j & M] = dd.nx;
            Cell hh = g;  // diagonal preferred on ties
            if (dd.s > g.s) hh = dd;
            N.cs[j & M] = hh.s; N.cm[j & M] = hh.nm; N.cx[j & M] = hh.nx;
            const Cell u{hh.s > NEGH ? hh.s + (int32_t)(j - lo) * E : NEG, hh.nm, hh.nx};
            run = cmax_left(run, u);
        }
        // pass 2: exclusive max-plus scan of the chunk aggregates over the workgroup (ties to the left)
        const Cell winc = wave_incl_maxscan(run);
        if (lane == 63) s_scan[wave] = winc;
        __syncthreads();
        Cell acc{NEG, 0, 0};
        for (uint32_t w = 0; w < wave; w++) acc = cmax_left(acc, s_scan[w]);
        acc = cmax_left(acc, dpp_cell<0x138, 0xf>(winc));  // best u of every column left of my chunk
        // pass 3: C = max(H, I), prune, row statistics
        Best4 rb{NEG, 0xFFFFFFFFu, 0, 0};
        uint32_t myfirst = 0xFFFFFFFFu, mylast = 0;
        for (uint32_t j = j0; j < j1; j++) {
            const Cell hh{N.cs[j & M], N.cm[j & M], N.cx[j & M]};
            Cell I{NEG, acc.nm, acc.nx};
            if (acc.s > NEGH) I.s = acc.s - O - (int32_t)(j - lo) * E;
            const Cell u{hh.s > NEGH ? hh.s + (int32_t)(j - lo) * E : NEG, hh.nm, hh.nx};
            acc = cmax_left(acc, u);
            Cell c = hh;  // H preferred over I on ties
            if (I.s > c.s) c = I;
            const bool alive = c.s >= thr && c.s > NEGH && (!BOUND || ((long long)j >= jlo && (long long)j <= jhi));
            N.cs[j & M] = alive ? c.s : NEG; N.cm[j & M] = c.nm; N.cx[j & M] = c.nx;
            if (!alive) N.ds[j & M] = NEG;
            if (alive) {
                if (myfirst == 0xFFFFFFFFu) myfirst = j;
                mylast = j;
                if (c.s > rb.s) { rb.s = c.s; rb.j = j; rb.nm = c.nm; rb.nx = c.nx; }
            }
        }
        // workgroup reductions: first / last live column, best cell (smallest column on ties: chunks grow with tid)
        uint32_t wf = myfirst, wl = (myfirst == 0xFFFFFFFFu) ? 0u : mylast + 1u;  // last + 1 so that 0 = none
        for (int o = 32; o > 0; o >>= 1) { wf = min(wf, (uint32_t)__shfl_xor((int)wf, o)); wl = max(wl, (uint32_t)__shfl_xor((int)wl, o)); }
        const Best4 wb4 = wave_best(rb);
        if (lane == 0) { s_first[wave] = wf; s_last[wave] = wl; s_best[wave] = wb4; }
        __syncthreads();
        uint32_t first_alive = 0xFFFFFFFFu, last1 = 0;
        Best4 tb{NEG, 0xFFFFFFFFu, 0, 0};
        for (int w = 0; w < ANY_THREADS / 64; w++) {
            first_alive = min(first_alive, s_first[w]);
            last1 = max(last1, s_last[w]);
            const Best4 o = s_best[w];
            if (o.s > tb.s || (o.s == tb.s && o.j < tb.j)) tb = o;
        }
        __syncthreads();  // the LDS arrays are rewritten in the next row
        if (first_alive == 0xFFFFFFFFu) break;
        lo = first_alive;
        hi = last1 - 1u;
        best.maxcols = max(best.maxcols, hi - lo + 1u);
        best.rows = i;
        if (BOUND) {
            klo = min(klo, (int32_t)((long long)lo - (long long)i));
            khi = max(khi, (int32_t)((long long)hi - (long long)i));
        }
        if (tb.s > best.score) { best.score = tb.s; best.i = i; best.j = tb.j; best.nm = tb.nm; best.nx = tb.nx; }
        // The cells are 32 bits wide (as lastz's own score_t, which wraps there).  Every live cell of a row lies within the
        // y-drop of the best score so far, so when that nears the cap the whole row — and the best score — is moved down by
        // half the cap and `sbase` up: comparisons inside a row and between neighbouring rows never see the difference, and
        // the half's score is sbase + best.score in 64 bits
        if (best.score > cap) {
            const int32_t K = cap / 2;
            for (uint32_t j = lo + tid; j <= hi; j += ANY_THREADS) {
                if (N.cs[j & M] > NEGH) N.cs[j & M] -= K;
                if (N.ds[j & M] > NEGH) N.ds[j & M] -= K;
            }
            best.score -= K;
            sbase += K;
            __syncthreads();
        }
    }
    best.base_lo = (uint32_t)(unsigned long long)sbase;
    best.base_hi = (uint32_t)((unsigned long long)sbase >> 32);
    best.overflow = overflow ? 1u : 0u;
    if (tid == 0) res[job.slot] = best;
    if (BOUND && tid == 0) sweep[job.slot] = HalfSweep{klo, khi, nacc, nbound};
}

// ---- traceback of a half extension (path rule) -------------------------------------------------------------------------
// Re-runs one half's DP over rows 1 .. i* (row r depends only on the rows above it, so they are the rows of the first
// run) with the recurrences, pruning and tie-breaks of k6_dp_any, storing one traceback byte per computed cell, checks the
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

// BOUND: the re-run is bounded as the first run was (the group's nacc has not moved since: same round, before k6_resolve)
template <bool BOUND>
__global__ __launch_bounds__(TR_THREADS) void k6_trace(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                       const TraceJob *__restrict__ tjobs, uint32_t k0,
                                                       const HalfResult *__restrict__ res, uint8_t *__restrict__ pool,
                                                       PathBlock *__restrict__ arena, unsigned long long arena_cap,
                                                       uint2 *__restrict__ pidx, unsigned int *__restrict__ ctr,
                                                       int32_t O, int32_t E, int32_t Y, BoundCtx B) {
    __shared__ int32_t s_ring[4 * TR_LDS_COLS];
    __shared__ Cell s_scan[TR_THREADS / 64];
    __shared__ Best4 s_best[TR_THREADS / 64];
    __shared__ uint32_t s_first[TR_THREADS / 64], s_last[TR_THREADS / 64];
    __shared__ uint32_t s_nb, s_off, s_bad;
    const uint32_t k = k0 + blockIdx.x;
    const DpJob job = jobs[k];
    const TraceJob J = tjobs[k];
    const HalfResult hr = res[job.slot];
    const Group &G = groups[job.group];
    const GStrandView T = G.T, Q = G.Q;
    const uint32_t at = job.at, aq = job.aq;
    const int dir = job.dir;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
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
    const uint32_t lenB = dir > 0 ? Q.len - aq : aq;
    const uint32_t W = J.W, M = J.R - 1u, rows = hr.i;
    const TraceLayout Lay = trace_layout(rows, W, J.R, J.cap);
    uint8_t *tb = pool + J.off;
    uint32_t *rowlo = (uint32_t *)(pool + J.off + Lay.rowlo);
    PathBlock *scratch = (PathBlock *)(pool + J.off + Lay.blk);
    int32_t *ring = J.R <= TR_LDS_COLS ? s_ring : (int32_t *)(pool + J.off + Lay.ring);
    int32_t *cs[2] = {ring, ring + 2u * J.R}, *ds[2] = {ring + J.R, ring + 3u * J.R};
    if (tid == 0) s_bad = 0;
    int32_t best = 0;
    uint32_t bi = 0, bj = 0;
    long long sbase = 0;
    uint32_t lo = 0, hi = 0;
    if (Y >= O + E) hi = min(lenB, (uint32_t)((Y - O) / E));
    const uint32_t ext = (uint32_t)((Y + 200) / E) + 2u;
    for (uint32_t j = tid; j <= hi; j += TR_THREADS) { cs[0][j & M] = j ? -O - (int32_t)j * E : 0; ds[0][j & M] = NEG; }
    __syncthreads();
    bool bad = hi + 2u > M;
    uint32_t par = 0;
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nacc = BOUND ? G.nacc : 0u;
    long long bkmin = -K_INF, bkmax = K_INF;
    uint32_t bnext = 1u;
    for (uint32_t i = 1; i <= rows && !bad; i++, par ^= 1u) {
        int32_t *Pc = cs[par], *Pd = ds[par], *Nc = cs[par ^ 1u], *Nd = ds[par ^ 1u];
        if (BOUND && i == bnext) {
            const RowBound rb = bounds_at(B, b0, nacc, at, aq, dir, i);
            bkmin = rb.kmin; bkmax = rb.kmax; bnext = rb.next;
        }
        const long long jlo = bkmin + (long long)i + 1, jhi = bkmax + (long long)i - 1;   // the allowed columns
        const int32_t thr = best - Y;
        const Base1 ab = base_at(T, dir > 0 ? (int32_t)(at + i - 1) : (int32_t)(at - i));
        const uint32_t hx = min(lenB, hi + 1u + ext);
        const uint32_t ncols = hx - lo + 1u;
        if (ncols > W || ncols + 2u > M) { bad = true; break; }
        uint8_t *trow = tb + (size_t)(i - 1u) * W - lo;  // indexed by column
        if (tid == 0) rowlo[i] = lo;
        const uint32_t chunk = (ncols + TR_THREADS - 1) / TR_THREADS;
        const uint32_t j0 = lo + tid * chunk, j1 = min(hx + 1u, j0 + chunk);
        // pass 1: D and H = max(diagonal, D)
        Cell run{NEG, 0, 0};   // nm carries the column of the maximum
        for (uint32_t j = j0; j < j1; j++) {
            const bool in = j <= hi;
            const int32_t cp = in ? Pc[j & M] : NEG, dp = in ? Pd[j & M] : NEG;
            int32_t dd = NEG, g = NEG;
            uint8_t bits = 0;
            if (dp > NEGH) dd = dp - E;
            if (cp > NEGH && cp - O - E > dd) { dd = cp - O - E; bits |= TB_DOPEN; }
            if (j >= 1 && j - 1 >= lo && j - 1 <= hi) {
                const int32_t pc = Pc[(j - 1) & M];
                if (pc > NEGH) {
                    const Base1 qb = base_at(Q, dir > 0 ? (int32_t)(aq + j - 1) : (int32_t)(aq - j));
                    g = pc + sub_score(ab.lo ^ qb.lo, ab.hi ^ qb.hi, ab.lo ^ ab.hi, ab.nm | qb.nm);
                }
            }
            if (BOUND && ((long long)j < jlo || (long long)j > jhi)) { dd = NEG; g = NEG; }
            Nd[j & M] = dd;
            int32_t hh = g;  // diagonal preferred on ties
            if (dd > g) { hh = dd; bits |= TB_HD; }
            Nc[j & M] = hh;
            trow[j] = bits;
            const int32_t u = hh > NEGH ? hh + (int32_t)(j - lo) * E : NEG;
            if (u > run.s) { run.s = u; run.nm = j; }
        }
        // pass 2: exclusive max-plus scan of the chunk aggregates (ties to the left: the column the insertion opened at)
        const Cell winc = wave_incl_maxscan(run);
        if (lane == 63) s_scan[wave] = winc;
        __syncthreads();
        Cell acc{NEG, 0, 0};
        for (uint32_t w = 0; w < wave; w++) acc = cmax_left(acc, s_scan[w]);
        acc = cmax_left(acc, dpp_cell<0x138, 0xf>(winc));
        // pass 3: C = max(H, I), prune, row statistics
        Best4 rb{NEG, 0xFFFFFFFFu, 0, 0};
        uint32_t myfirst = 0xFFFFFFFFu, mylast = 0;
        for (uint32_t j = j0; j < j1; j++) {
            const int32_t hh = Nc[j & M];
            const bool ilive = acc.s > NEGH;
            const int32_t I = ilive ? acc.s - O - (int32_t)(j - lo) * E : NEG;
            uint8_t bits = (ilive && acc.nm + 1u == j) ? TB_IOPEN : 0;   // I(j) opened from H(j - 1)
            const int32_t u = hh > NEGH ? hh + (int32_t)(j - lo) * E : NEG;
            if (u > acc.s) { acc.s = u; acc.nm = j; }
            int32_t c = hh;  // H preferred over I on ties
            if (I > c) { c = I; bits |= TB_CI; }
            const bool alive = c >= thr && c > NEGH && (!BOUND || ((long long)j >= jlo && (long long)j <= jhi));
            Nc[j & M] = alive ? c : NEG;
            if (!alive) Nd[j & M] = NEG;
            trow[j] |= bits;
            if (alive) {
                if (myfirst == 0xFFFFFFFFu) myfirst = j;
                mylast = j;
                if (c > rb.s) { rb.s = c; rb.j = j; }
            }
        }
        uint32_t wf = myfirst, wl = (myfirst == 0xFFFFFFFFu) ? 0u : mylast + 1u;
        for (int o = 32; o > 0; o >>= 1) { wf = min(wf, (uint32_t)__shfl_xor((int)wf, o)); wl = max(wl, (uint32_t)__shfl_xor((int)wl, o)); }
        const Best4 wb4 = wave_best(rb);
        if (lane == 0) { s_first[wave] = wf; s_last[wave] = wl; s_best[wave] = wb4; }
        __syncthreads();
        uint32_t first_alive = 0xFFFFFFFFu, last1 = 0;
        Best4 tbest{NEG, 0xFFFFFFFFu, 0, 0};
        for (int w = 0; w < TR_THREADS / 64; w++) {
            first_alive = min(first_alive, s_first[w]);
            last1 = max(last1, s_last[w]);
            const Best4 o = s_best[w];
            if (o.s > tbest.s || (o.s == tbest.s && o.j < tbest.j)) tbest = o;
        }
        __syncthreads();
        if (first_alive == 0xFFFFFFFFu) { bad = true; break; }   // the first run went on to row i*
        lo = first_alive;
        hi = last1 - 1u;
        if (tbest.s > best) { best = tbest.s; bi = i; bj = tbest.j; }
        if (best > 2000000000) {   // k6_dp_any's rebase (scores of 64 bits, cells of 32)
            const int32_t K = 1000000000;
            for (uint32_t j = lo + tid; j <= hi; j += TR_THREADS) {
                if (Nc[j & M] > NEGH) Nc[j & M] -= K;
                if (Nd[j & M] > NEGH) Nd[j & M] -= K;
            }
            best -= K;
            sbase += K;
            __syncthreads();
        }
    }
    if (tid == 0 && (bad || bi != hr.i || bj != hr.j || sbase + best != half_score(hr))) { ctr[1] = TRERR_DP; ctr[2] = job.slot; s_bad = 1; }
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

// one wave per group: finalise anchors in rank order as far as DP results exist
constexpr uint32_t RESOLVE_NEW = 256;  // boxes accepted per invocation that fit the LDS list

// bounded extensions: does the alignment of the anchor of rank `rank` (box o: tstart, tend, qstart, qend) put a bound
// into the cells that the halves L / R of anchor a looked at?  Yes iff one of its blocks covers an evaluated row of a half
// and its diagonal lies within the k that half swept.  Wave-cooperative (lanes over the blocks).
__device__ __forceinline__ bool bounds_touch(const PathView &P, const uint2 *anchors, uint64_t b0, uint32_t rank, uint4 o, uint2 a,
                                             const HalfResult &L, const HalfResult &R, const HalfSweep &sL, const HalfSweep &sR) {
    const uint32_t rowsL = L.rows ? L.rows : L.i, rowsR = R.rows ? R.rows : R.i;   // rows == 0, i > 0: the shortcut's diagonal
    const long long tlo = (long long)a.x - rowsL, thi = (long long)a.x + rowsR;    // target bases the two halves consumed
    if ((long long)o.y <= tlo || (long long)o.x >= thi) return false;
    const long long d0 = (long long)a.y - (long long)a.x;
    bool hit = false;
    for (uint32_t side = 0; side < 2; side++) {
        const uint2 ix = P.pidx[2u * (b0 + rank) + side];
        if (ix.x == PATH_UNTRACED) continue;
        for (uint32_t k = threadIdx.x & 63u; k < ix.y; k += 64u) {
            const PathBlock b = P.blk[ix.x + k];
            const long long t0 = b.t, t1 = (long long)b.t + b.len, d = (long long)b.q - (long long)b.t;
            if (t0 < thi && t1 > (long long)a.x && d - d0 >= sR.klo && d - d0 <= sR.khi) hit = true;
            if (t0 < (long long)a.x && t1 > tlo && d0 - d >= sL.klo && d0 - d <= sL.khi) hit = true;
        }
    }
    return __ballot(hit) != 0;
}

// BOUND (mimeo_params.bound_extensions, with PATH): the rule is sequential — rank r is bounded by everything accepted
// below r — but a round's DPs ran against the alignments accepted when the round began (HalfSweep.nacc).  Before rank r
// is accepted, every alignment accepted since is tested against what r's halves swept (bounds_touch); if one touches,
// the result is stale: the anchor goes back to A_NEW and the group's resolve stops there, so the next round runs it
// again as the group's lowest unfinalised anchor, which is always bounded by exactly the alignments below it.
// RANK (box rule, paths asked for): the rank of every accepted anchor is recorded as under the path rule (k6_kept_jobs).
template <bool PATH, bool BOUND = false, bool RANK = false>
__global__ __launch_bounds__(64) void k6_resolve(Group *__restrict__ groups, const uint2 *__restrict__ anchors,
                                                 const HalfResult *__restrict__ res, mimeo_alignment *__restrict__ aln,
                                                 uint8_t *__restrict__ astate, unsigned int *__restrict__ remaining, PathView P,
                                                 const HalfSweep *__restrict__ sweep) {
    __shared__ uint4 sbox[RESOLVE_NEW];  // boxes accepted in this invocation (tstart, tend, qstart, qend)
    __shared__ uint32_t srank[PATH ? RESOLVE_NEW : 1];  // ... and the ranks of their anchors (path rule)
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t nacc0 = G.nacc;
    uint32_t nnew = 0, overflow = 0, r = G.next;
    for (; r < G.nchain; r++) {
        const uint8_t st = astate[b0 + r];
        if (st == A_SKIPPED || st == A_ACCEPTED) continue;
        if (nnew == RESOLVE_NEW) break;
        const uint2 a = anchors[b0 + r];
        bool inside = skip_test<PATH>(aln, nacc0, a, P, anchors, b0);  // alignments of earlier invocations (global memory)
        if (!inside) {
            bool in2 = false;
            for (uint32_t e = threadIdx.x; e < nnew; e += 64) {
                uint4 o = sbox[e];
                if (a.x >= o.x && a.x < o.y && a.y >= o.z && a.y < o.w && (!PATH || on_path(P, anchors, b0, srank[PATH ? e : 0], a)))
                    in2 = true;
            }
            inside = __ballot(in2) != 0;
        }
        if (inside) {  // also for an anchor without DP result: a deferred anchor swallowed by now never needs one
            if (threadIdx.x == 0) astate[b0 + r] = A_SKIPPED;
            continue;
        }
        if (st == A_NEW) break;  // not swallowed and no DP result yet: it is scheduled in the next round
        const uint32_t slot = 2u * (uint32_t)(b0 + r);
        HalfResult L = res[slot], R = res[slot + 1];
        if (BOUND && !(L.overflow | R.overflow)) {
            const HalfSweep sL = sweep[slot], sR = sweep[slot + 1];
            bool stale = false;
            for (uint32_t e = sL.nacc; e < nacc0 && !stale; e++) {
                const mimeo_alignment &o = aln[b0 + e];
                stale = bounds_touch(P, anchors, b0, P.accrank[b0 + e], make_uint4(o.tstart, o.tend, o.qstart, o.qend), a, L, R, sL, sR);
            }
            for (uint32_t e = 0; e < nnew && !stale; e++)
                stale = bounds_touch(P, anchors, b0, srank[PATH ? e : 0], sbox[e], a, L, R, sL, sR);
            if (stale) {
                if (threadIdx.x == 0) { astate[b0 + r] = A_NEW; atomicAdd(remaining + 2, 1u); }
                break;
            }
        }
        overflow |= L.overflow | R.overflow;
        // path rule: a half without a traceback (larger than the trace pool) fails the group like a band beyond the limit
        if (PATH && (P.pidx[slot].x == PATH_UNTRACED || P.pidx[slot + 1].x == PATH_UNTRACED)) overflow = 1;
        if (threadIdx.x == 0) {
            mimeo_alignment m;
            m.tid = G.tid; m.qid = G.qid; m.qstrand = G.minus; m.reserved = 0;
            m.tstart = a.x - L.i; m.tend = a.x + R.i; m.qstart = a.y - L.j; m.qend = a.y + R.j;
            m.score = half_score(L) + half_score(R);
            m.id_n = L.nm + R.nm;
            m.id_d = L.nm + R.nm + L.nx + R.nx;
            aln[b0 + nacc0 + nnew] = m;
            sbox[nnew] = make_uint4(m.tstart, m.tend, m.qstart, m.qend);
            if (PATH) srank[PATH ? nnew : 0] = r;
            if (PATH || RANK) P.accrank[b0 + nacc0 + nnew] = r;
            astate[b0 + r] = A_ACCEPTED;
        }
        nnew++;
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        G.next = r;
        G.nacc = nacc0 + nnew;
        G.nbatch = 0;
        if (overflow) G.overflow = 1;
        if (r < G.nchain) atomicAdd(remaining, 1u);
    }
}

// gap-free mode (--gapped off): every chained HSP is reported as is; identity by popcount
__global__ __launch_bounds__(256) void k6_ungapped(Group *__restrict__ groups, const mimeo_hsp *__restrict__ hs,
                                                   const uint32_t *__restrict__ order, mimeo_alignment *__restrict__ aln) {
    Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t r = threadIdx.x >> 6; r < G.nchain; r += 4) {
        const mimeo_hsp h = hs[b0 + order[b0 + r]];
        const int32_t d = (int32_t)h.tstart - (int32_t)h.qstart;
        uint32_t nmatch = 0;
        for (uint32_t w0 = lane * 32u; w0 < h.length; w0 += 64u * 32u) {
            int32_t pt = (int32_t)(h.tstart + w0), pq = pt - d;
            const Win32 tw = win32(G.T, pt), qw = win32(G.Q, pq);
            uint32_t mm = ~((tw.lo ^ qw.lo) | (tw.hi ^ qw.hi)) & ~(tw.nm | qw.nm);
            uint32_t rem = h.length - w0;
            if (rem < 32) mm &= (1u << rem) - 1u;
            nmatch += __popc(mm);
        }
        for (int o = 32; o > 0; o >>= 1) nmatch += __shfl_xor(nmatch, o);
        if (lane == 0) {
            mimeo_alignment m;
            m.tid = G.tid; m.qid = G.qid; m.qstrand = G.minus; m.reserved = 0;
            m.tstart = h.tstart; m.tend = h.tstart + h.length; m.qstart = h.qstart; m.qend = h.qstart + h.length;
            m.score = h.score; m.id_n = nmatch; m.id_d = h.length;
            aln[b0 + r] = m;
        }
    }
    if (threadIdx.x == 0) G.nacc = G.nchain;
}

// threshold, minus-strand coordinates -> query plus strand (start2+/end2+), compaction
__global__ void k6_finish(Group *__restrict__ groups, uint32_t ngroups, mimeo_alignment *__restrict__ aln,
                          int32_t thresh) {
    uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    Group &G = groups[g];
    const uint64_t b0 = G.hsp_begin;
    uint32_t k = 0;
    for (uint32_t e = 0; e < G.nacc; e++) {
        mimeo_alignment a = aln[b0 + e];
        if (a.score < thresh) continue;
        if (G.minus) { uint32_t s = G.Q.len - a.qend, t2 = G.Q.len - a.qstart; a.qstart = s; a.qend = t2; }
        aln[b0 + k++] = a;
    }
    G.naln = k;
}

// The alignments of group g sit at d_aln[hsp_begin .. hsp_begin + naln): a few thousand records scattered over an array of
// one slot per HSP (70 MB on a C4 row).  Packed densely before the read-back: job0 = the group's first dense slot.
__global__ __launch_bounds__(1024) void k6_dense_offsets(Group *__restrict__ groups, uint32_t ngroups) {
    __shared__ uint32_t part[1024];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    for (uint32_t g0 = 0; g0 < ngroups; g0 += 1024) {
        const uint32_t g = g0 + threadIdx.x, n = g < ngroups ? groups[g].naln : 0u;
        part[threadIdx.x] = n;
        __syncthreads();
        for (uint32_t o = 1; o < 1024; o <<= 1) {
            const uint32_t v = threadIdx.x >= o ? part[threadIdx.x - o] : 0u;
            __syncthreads();
            part[threadIdx.x] += v;
            __syncthreads();
        }
        if (g < ngroups) groups[g].job0 = carry + part[threadIdx.x] - n;
        __syncthreads();
        if (threadIdx.x == 1023) carry += part[1023];
        __syncthreads();
    }
}
__global__ __launch_bounds__(64) void k6_dense_copy(const Group *__restrict__ groups, const mimeo_alignment *__restrict__ aln,
                                                    mimeo_alignment *__restrict__ dense) {
    const Group &G = groups[blockIdx.x];
    for (uint32_t k = threadIdx.x; k < G.naln; k += 64) dense[G.job0 + k] = aln[G.hsp_begin + k];
}
void dense_alignments_device(Group *d_groups, uint32_t ngroups, const mimeo_alignment *d_aln, mimeo_alignment *d_dense) {
    hipLaunchKernelGGL(k6_dense_offsets, dim3(1), dim3(1024), 0, stream(), d_groups, ngroups);
    hipLaunchKernelGGL(k6_dense_copy, dim3(ngroups), dim3(64), 0, stream(), (const Group *)d_groups, d_aln, d_dense);
}

static DeviceBuf g_anchors, g_packed, g_jobs, g_res, g_cnt, g_astate, g_ovf_list, g_any;
// path rule: per half slot (first block, count), per alignment slot the anchor's rank, the block arena, the trace pool
static DeviceBuf g_pidx, g_accrank, g_arena, g_pool, g_tjobs, g_tres, g_tctr;
static DeviceBuf g_kjobs, g_pcnt, g_pslot, g_ptmp;   // paths out: jobs of the box rule's trace pass; block counts, half slots, scan scratch
static DeviceBuf g_sweep;   // bounded extensions: per half slot what its DP swept (HalfSweep)

// bounded extensions with penalties outside the lean kernel's domain: every job of the round goes to k6_dp_any<true>
__global__ void k6_list_all(uint32_t n, unsigned int *__restrict__ novf, unsigned int *__restrict__ ovf_list) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) ovf_list[k] = k;
    if (k == 0) *novf = n;
}

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

// before k6_finish: accrank[hsp_begin + k] = anchor rank of the k-th alignment that k6_finish keeps; a kept alignment with a
// half whose traceback did not fit the trace pool fails its group (what k6_resolve<true> does under the path rule)
__global__ void k6_kept_ranks(Group *__restrict__ groups, uint32_t ngroups, const mimeo_alignment *__restrict__ aln,
                              uint32_t *__restrict__ accrank, const uint2 *__restrict__ pidx, int32_t thresh) {
    const uint32_t g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= ngroups) return;
    Group &G = groups[g];
    const uint64_t b0 = G.hsp_begin;
    uint32_t k = 0;
    for (uint32_t e = 0; e < G.nacc; e++) {
        if (aln[b0 + e].score < thresh) continue;
        const uint32_t rank = accrank[b0 + e];
        const uint32_t slot = 2u * (uint32_t)(b0 + rank);
        if (pidx[slot].x == PATH_UNTRACED || pidx[slot + 1].x == PATH_UNTRACED) G.overflow = 1;
        accrank[b0 + k++] = rank;   // k <= e
    }
}

// gap-free mode, after k6_ungapped: alignment r of a group is one block, kept as the left half of "anchor" r
__global__ __launch_bounds__(256) void k6_ungapped_paths(const Group *__restrict__ groups, const mimeo_alignment *__restrict__ aln,
                                                         PathBlock *__restrict__ arena, uint2 *__restrict__ pidx,
                                                         uint32_t *__restrict__ accrank) {
    const Group &G = groups[blockIdx.x];
    const uint64_t b0 = G.hsp_begin;
    for (uint32_t r = threadIdx.x; r < G.nacc; r += 256) {
        const mimeo_alignment a = aln[b0 + r];
        arena[b0 + r] = PathBlock{a.tstart, a.qstart, a.tend - a.tstart};
        pidx[2u * (b0 + r)] = make_uint2((uint32_t)(b0 + r), 1u);
        pidx[2u * (b0 + r) + 1u] = make_uint2(0u, 0u);
        accrank[b0 + r] = r;
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

// bytes of traceback the path rule may hold at once: a share of the free device memory (like the queue arenas of K4);
// MIMEO_K6_TRACE_POOL_MB sets it (tests: force slices, or a pool too small for one half)
static int trace_pool_budget(uint64_t *budget) {
    size_t free_b = 0, total_b = 0;
    HIP_TRY(hipMemGetInfo(&free_b, &total_b));
    *budget = std::min<uint64_t>(((uint64_t)free_b + g_pool.cap) / 4, 16ull << 30);
    if (getenv("MIMEO_K6_TRACE_POOL_MB")) *budget = (uint64_t)atol(getenv("MIMEO_K6_TRACE_POOL_MB")) << 20;
    return 0;
}

// the block arena grows with its contents (block offsets stay valid)
static int arena_reserve(uint64_t blocks, uint64_t used) {
    const size_t bytes = (size_t)blocks * sizeof(PathBlock);
    if (bytes <= g_arena.cap) return 0;
    DeviceBuf nb;
    int rc = nb.reserve(std::max(bytes, 2 * g_arena.cap));
    if (rc) return rc;
    if (used) HIP_TRY(hipMemcpyAsync(nb.p, g_arena.p, (size_t)used * sizeof(PathBlock), hipMemcpyDeviceToDevice, stream()));
    HIP_TRY(hipStreamSynchronize(stream()));
    g_arena.release();
    g_arena = nb;
    return 0;
}

// path rule, after the DP kernels of a round: the traceback of every half of the h0 jobs in d_jobs (the round's; under the box
// rule with paths asked for, the halves of the alignments that are returned: paths_pass), in slices of jobs whose
// tracebacks fit the pool together.  A half whose traceback alone exceeds the pool gets no path (PATH_UNTRACED): k6_resolve
// fails its group if the anchor is accepted, as for a band beyond the DP limit.
static int trace_round(Group *d_groups, const DpJob *d_jobs, uint32_t h0, const mimeo_params *p, uint64_t budget, uint64_t *arena_used, float *ms,
                       uint32_t *slices, uint64_t *largest, bool bounded, BoundCtx bc) {
    hipStream_t st = stream();
    int rc;
    if ((rc = g_tres.reserve((size_t)h0 * sizeof(HalfResult)))) return rc;
    hipLaunchKernelGGL(k6_trace_gather, dim3((h0 + 255) / 256), dim3(256), 0, st, d_jobs, h0, (const HalfResult *)g_res.p,
                       (HalfResult *)g_tres.p);
    std::vector<HalfResult> hr(h0);
    HIP_TRY(hipMemcpyAsync(hr.data(), g_tres.p, (size_t)h0 * sizeof(HalfResult), hipMemcpyDeviceToHost, st));
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
                *largest = std::max(*largest, need);
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
    if ((rc = g_tjobs.reserve((size_t)h0 * sizeof(TraceJob)))) return rc;
    HIP_TRY(hipMemcpyAsync(g_tjobs.p, tj.data(), (size_t)h0 * sizeof(TraceJob), hipMemcpyHostToDevice, st));
    if (need_max && (rc = g_pool.reserve(need_max))) return rc;
    if ((rc = arena_reserve(*arena_used + blocks + 1, *arena_used))) return rc;
    static hipEvent_t e0 = nullptr, e1 = nullptr;
    if (!e0) { HIP_TRY(hipEventCreate(&e0)); HIP_TRY(hipEventCreate(&e1)); }
    HIP_TRY(hipEventRecord(e0, st));
    bc.P.blk = (const PathBlock *)g_arena.p;   // the arena may just have grown
    const auto trace = bounded ? k6_trace<true> : k6_trace<false>;
    for (size_t c = 0; c + 1 < cut.size(); c++)
        if (cut[c + 1] > cut[c] && ++*slices)
            hipLaunchKernelGGL(trace, dim3(cut[c + 1] - cut[c]), dim3(TR_THREADS), 0, st, (const Group *)d_groups,
                               d_jobs, (const TraceJob *)g_tjobs.p, cut[c], (const HalfResult *)g_res.p,
                               (uint8_t *)g_pool.p, (PathBlock *)g_arena.p, (unsigned long long)(g_arena.cap / sizeof(PathBlock)),
                               (uint2 *)g_pidx.p, (unsigned int *)g_tctr.p, O, E, Y, bc);
    HIP_TRY(hipEventRecord(e1, st));
    unsigned int c3[3] = {0, 0, 0};
    HIP_TRY(hipMemcpyAsync(c3, g_tctr.p, 12, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    float t = 0;
    HIP_TRY(hipEventElapsedTime(&t, e0, e1));
    *ms += t;
    if (c3[1]) {
        char msg[200];
        snprintf(msg, sizeof msg, "internal: K6 traceback of half slot %u %s", c3[2],
                 c3[1] == TRERR_DP ? "disagrees with its DP result (score or end cell)"
                 : c3[1] == TRERR_WALK ? "disagrees with its DP result (matches / mismatches along the path)" : "outgrew the block arena");
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    *arena_used = c3[0];
    return 0;
}

// The DP kernels of a round over its n jobs, each taking the jobs that the one before could not hold: the lean kernel, the
// 2048-column kernel (not in bounded mode: it knows no bounds), the global-memory kernel.  The lean kernel's dead-cell
// arithmetic needs the penalties to stay far below 2^29 / 1024; beyond that every job starts at the second kernel of its mode.
static int dp_round(Group *d_groups, uint32_t n, const mimeo_params *p, int32_t cap, bool bounded, const BoundCtx &bc,
                    unsigned int *novf) {
    hipStream_t st = stream();
    int rc;
    const Group *groups = d_groups;
    const DpJob *jobs = (const DpJob *)g_jobs.p;
    HalfResult *res = (HalfResult *)g_res.p;
    HalfSweep *sweep = bounded ? (HalfSweep *)g_sweep.p : nullptr;
    unsigned int *list = (unsigned int *)g_ovf_list.p;
    const int32_t O = p->gap_open, E = p->gap_extend, Y = p->ydrop;
    const bool lean_ok = E <= (1 << 16) && O <= (1 << 24) && Y <= (1 << 28);
    if (bounded) {
        if (lean_ok) hipLaunchKernelGGL(k6_dp1_bounded, dim3(n), dim3(64), 0, st, groups, jobs, res, sweep, O, E, Y, bc, novf, list);
        else hipLaunchKernelGGL(k6_list_all, dim3((n + 255) / 256), dim3(256), 0, st, n, novf, list);
    } else {
        if (lean_ok) hipLaunchKernelGGL(k6_dp1, dim3(n), dim3(64), 0, st, groups, jobs, res, O, E, Y);
        hipLaunchKernelGGL(k6_dp_wide, dim3(n), dim3(64), 0, st, groups, jobs, res, O, E, Y, novf, list, cap, lean_ok ? 0 : 1);
    }
    // bands beyond 2048 columns (tandem arrays): the global-memory kernel, a few jobs at a time
    unsigned int nov = 0;
    HIP_TRY(hipMemcpyAsync(&nov, novf, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!nov) return 0;
    const unsigned int slots = std::min<unsigned int>(nov, 32u);
    if ((rc = g_any.reserve((size_t)slots * ANY_SLOT_WORDS * 4))) return rc;
    const auto any = bounded ? k6_dp_any<true> : k6_dp_any<false>;
    for (unsigned int f = 0; f < nov; f += slots)
        hipLaunchKernelGGL(any, dim3(std::min(slots, nov - f)), dim3(ANY_THREADS), 0, st, groups, jobs, (const unsigned int *)list, f, res,
                           (uint32_t *)g_any.p, O, E, Y, cap, bc, sweep);
    return 0;
}

// MIMEO_K6_STATS: what the DP kernels made of the round's n jobs, on stderr; bounded mode: *bound_jobs counts those that met a bound
static int round_stats(uint32_t n, uint64_t nhsps, bool bounded, unsigned long long *bound_jobs) {
    std::vector<DpJob> hj(n);
    std::vector<HalfResult> hall((size_t)nhsps * 2), hr(n);
    HIP_TRY(hipStreamSynchronize(stream()));
    HIP_TRY(hipMemcpy(hj.data(), g_jobs.p, (size_t)n * sizeof(DpJob), hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hall.data(), g_res.p, hall.size() * sizeof(HalfResult), hipMemcpyDeviceToHost));
    for (size_t k = 0; k < hr.size(); k++) hr[k] = hall[hj[k].slot];
    unsigned long long hist[9] = {0}, rows = 0, maxr = 0, shortcut = 0;
    for (auto &r : hr) {
        if (!r.rows) { shortcut++; continue; }
        hist[std::min<uint32_t>(8, r.maxcols / 128)]++; rows += r.rows; maxr = std::max<unsigned long long>(maxr, r.rows);
    }
    unsigned long long rebased = 0;
    for (auto &r : hr) if (r.base_lo | r.base_hi) rebased++;
    fprintf(stderr, "[k6] jobs %u shortcut %llu (rebased in k6_dp_any: %llu) rows total %llu max %llu band<128..>=1024:", n, shortcut, rebased, rows, maxr);
    for (int b = 0; b < 9; b++) fprintf(stderr, " %llu", hist[b]);
    fprintf(stderr, "\n");
    {
        unsigned long long fine[34] = {0};
        for (auto &r : hr) if (r.rows) fine[std::min<uint32_t>(33, r.maxcols / 32)]++;
        fprintf(stderr, "[k6] widest band, buckets of 32 columns from 448:");
        for (int b = 14; b < 34; b++) fprintf(stderr, " %llu", fine[b]);
        fprintf(stderr, "\n");
    }
    int shown = 0;
    for (auto &r : hr)
        if (!r.rows && shown < 8) { fprintf(stderr, "  [k6] zero-row job: score %d i %u j %u nm %u nx %u ovf %u\n", r.score, r.i, r.j, r.nm, r.nx, r.overflow); shown++; }
    if (bounded) {
        std::vector<HalfSweep> hs((size_t)nhsps * 2);
        HIP_TRY(hipMemcpy(hs.data(), g_sweep.p, hs.size() * sizeof(HalfSweep), hipMemcpyDeviceToHost));
        for (auto &j : hj) *bound_jobs += hs[j.slot].nbound ? 1u : 0u;
    }
    return 0;
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
    if ((rc = g_pcnt.reserve((size_t)(ndense + 1) * 4)) || (rc = g_pslot.reserve((size_t)ndense * 4))) return rc;
    HIP_TRY(hipMemsetAsync(g_pcnt.p, 0, (size_t)(ndense + 1) * 4, st));
    const uint32_t nd = (uint32_t)ndense;
    const dim3 grid((nd + PATH_WAVES - 1) / PATH_WAVES), block(64 * PATH_WAVES);
    hipLaunchKernelGGL(k6_path_slots, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint32_t *)g_accrank.p, (uint32_t *)g_pslot.p);
    hipLaunchKernelGGL(k6_path_count, grid, block, 0, st, (const uint32_t *)g_pslot.p, (const uint2 *)g_pidx.p, (const PathBlock *)g_arena.p, nd,
                       (uint32_t *)g_pcnt.p);
    size_t tb = 0;
    HIP_TRY(rocprim::exclusive_scan(nullptr, tb, (uint32_t *)g_pcnt.p, (unsigned long long *)first.p, 0ull, (size_t)ndense + 1,
                                    rocprim::plus<unsigned long long>(), st));
    if ((rc = g_ptmp.reserve(tb ? tb : 1))) return rc;
    HIP_TRY(rocprim::exclusive_scan(g_ptmp.p, tb, (uint32_t *)g_pcnt.p, (unsigned long long *)first.p, 0ull, (size_t)ndense + 1,
                                    rocprim::plus<unsigned long long>(), st));
    unsigned long long total = 0;
    HIP_TRY(hipMemcpyAsync(&total, (const unsigned long long *)first.p + ndense, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *nblocks = total;
    if (!total) return 0;
    if ((rc = blocks.reserve((size_t)total * sizeof(PathBlock)))) return rc;
    hipLaunchKernelGGL(k6_path_write, grid, block, 0, st, (const uint32_t *)g_pslot.p, (const uint2 *)g_pidx.p, (const PathBlock *)g_arena.p, nd,
                       (const unsigned long long *)first.p, (PathBlock *)blocks.p);
    HIP_TRY(hipGetLastError());
    return 0;
}

// paths out under the box rule, after the last round: one trace pass over the two halves of every accepted alignment with
// score >= hspthresh (k6_kept_jobs), through the slices of trace_round; k6_trace<false>'s agreement check stays an error
static int paths_pass(Group *d_groups, uint32_t ngroups, const mimeo_params *p, const mimeo_alignment *d_aln, uint64_t budget,
                      bool k6_stats) {
    hipStream_t st = stream();
    int rc;
    unsigned int *ctr = (unsigned int *)g_cnt.p;
    HIP_TRY(hipMemsetAsync(g_cnt.p, 0, 16, st));
    const dim3 grid((ngroups + 63) / 64), block(64);
    hipLaunchKernelGGL(k6_kept_jobs, grid, block, 0, st, (const Group *)d_groups, ngroups, d_aln, (const uint2 *)g_anchors.p,
                       (const uint32_t *)g_accrank.p, p->hspthresh, (DpJob *)nullptr, ctr);
    unsigned int njobs = 0;
    HIP_TRY(hipMemcpyAsync(&njobs, ctr, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!njobs) return 0;
    if ((rc = g_kjobs.reserve((size_t)njobs * sizeof(DpJob)))) return rc;
    hipLaunchKernelGGL(k6_kept_jobs, grid, block, 0, st, (const Group *)d_groups, ngroups, d_aln, (const uint2 *)g_anchors.p,
                       (const uint32_t *)g_accrank.p, p->hspthresh, (DpJob *)g_kjobs.p, ctr);
    uint64_t arena_used = 0, largest = 0;
    float ms = 0;
    uint32_t slices = 0;
    if ((rc = trace_round(d_groups, (const DpJob *)g_kjobs.p, njobs, p, budget, &arena_used, &ms, &slices, &largest, false, BoundCtx{}))) return rc;
    if (k6_stats)
        fprintf(stderr, "[k6] paths out: traceback of %u halves %.3f ms, slices %u, %llu path blocks, pool %.1f MB, largest half %.3f MB\n", njobs, ms,
                slices, (unsigned long long)arena_used, g_pool.cap / 1048576.0, largest / 1048576.0);
    return 0;
}

int gapped_device(Group *d_groups, uint32_t ngroups, const mimeo_hsp *d_sorted, const uint32_t *d_order,
                  uint64_t nhsps, const mimeo_params *p, mimeo_alignment *d_aln, bool want_paths) {
    if (!ngroups || !nhsps) return 0;
    hipStream_t st = stream();
    int rc;
    if (want_paths) {   // per half slot its blocks, per alignment slot its anchor's rank (the path rule's tables, under every rule)
        if (nhsps >= (1ull << 31)) { set_error("paths: more than 2^31 HSPs in one batch"); return MIMEO_ERR_LIMIT; }
        if ((rc = g_pidx.reserve((size_t)nhsps * 2 * sizeof(uint2)))) return rc;
        if ((rc = g_accrank.reserve((size_t)nhsps * 4))) return rc;
    }
    if (!p->gapped) {
        hipLaunchKernelGGL(k6_ungapped, dim3(ngroups), dim3(256), 0, st, d_groups, d_sorted, d_order, d_aln);
        if (want_paths) {
            if ((rc = arena_reserve(nhsps, 0))) return rc;
            hipLaunchKernelGGL(k6_ungapped_paths, dim3(ngroups), dim3(256), 0, st, (const Group *)d_groups, (const mimeo_alignment *)d_aln,
                               (PathBlock *)g_arena.p, (uint2 *)g_pidx.p, (uint32_t *)g_accrank.p);
        }
    } else {
        // development switches: read once per call, not per round (MIMEO_K6_TRACE_POOL_MB: trace_pool_budget)
        uint32_t bmax = 8192u / ngroups;  // anchors per group and round (200 units: 32 -> one large round and a short one)
        if (getenv("MIMEO_K6_BMAX")) bmax = (uint32_t)atoi(getenv("MIMEO_K6_BMAX"));
        const bool k6_stats = getenv("MIMEO_K6_STATS") != nullptr;
        // 32-bit DP cells: beyond this score a half extension goes to (or, in k6_dp_any, rebases its cells in) the last kernel;
        // MIMEO_K6_SCORE_CAP lowers it so that tests of ordinary size take that road
        const int32_t cap = getenv("MIMEO_K6_SCORE_CAP") ? std::max(100000, atoi(getenv("MIMEO_K6_SCORE_CAP"))) : 2000000000;
        bmax = bmax < 1 ? 1 : (bmax > MAX_BATCH ? MAX_BATCH : bmax);
        if ((rc = g_anchors.reserve(nhsps * sizeof(uint2)))) return rc;
        if ((rc = g_packed.reserve(nhsps * 8))) return rc;
        HIP_TRY(hipMemsetAsync(g_packed.p, 0, nhsps * 8, st));
        if ((rc = g_jobs.reserve((size_t)ngroups * bmax * 2 * sizeof(DpJob)))) return rc;
        if ((rc = g_res.reserve((size_t)nhsps * 2 * sizeof(HalfResult)))) return rc;
        if ((rc = g_astate.reserve((size_t)nhsps * 2))) return rc;  // state | defer count
        HIP_TRY(hipMemsetAsync(g_astate.p, 0, (size_t)nhsps * 2, st));
        if ((rc = g_cnt.reserve(16))) return rc;
        if ((rc = g_ovf_list.reserve((size_t)ngroups * bmax * 2 * sizeof(unsigned int)))) return rc;
        // many small groups (scaffold pairs of a packed fragmented assembly): one workgroup each will do
        const uint32_t asplit = ngroups > 4096 ? 1u : ANCHOR_SPLIT;
        hipLaunchKernelGGL(k6_anchor_points, dim3(ngroups, asplit), dim3(ANCHOR_THREADS), 0, st, (const Group *)d_groups,
                           d_sorted, d_order, (unsigned long long *)g_packed.p);
        hipLaunchKernelGGL(k6_anchor_final, dim3(ngroups), dim3(256), 0, st, (const Group *)d_groups, d_sorted, d_order,
                           (const unsigned long long *)g_packed.p, (uint2 *)g_anchors.p);
        const bool path = p->anchor_rule == MIMEO_ANCHOR_PATH;
        const bool bounded = path && p->bound_extensions;   // api.hip: bound_extensions needs the path rule
        unsigned long long bound_jobs = 0, rescheduled = 0;  // statistics of the bounded mode
        uint64_t pool_budget = 0, arena_used = 0;
        float ms_trace = 0;
        uint32_t trace_slices = 0, rounds = 0;
        uint64_t largest = 0;   // largest traceback of one half (bytes)
        PathView pv{nullptr, nullptr, nullptr};
        const bool box_paths = want_paths && !path;   // the anchors' ranks are recorded; the halves are traced after the last round
        if (path || box_paths) {
            if ((rc = g_pidx.reserve((size_t)nhsps * 2 * sizeof(uint2)))) return rc;
            if ((rc = g_accrank.reserve((size_t)nhsps * 4))) return rc;
            if ((rc = g_tctr.reserve(16))) return rc;
            if ((rc = arena_reserve(1024, 0))) return rc;
            HIP_TRY(hipMemsetAsync(g_tctr.p, 0, 16, st));
            if ((rc = trace_pool_budget(&pool_budget))) return rc;
            pv = PathView{(const uint2 *)g_pidx.p, nullptr, (uint32_t *)g_accrank.p};
        }
        if (bounded && (rc = g_sweep.reserve((size_t)nhsps * 2 * sizeof(HalfSweep)))) return rc;
        const auto pick = path ? k6_pick<true> : k6_pick<false>;
        const auto resolve = bounded ? k6_resolve<true, true> : path ? k6_resolve<true, false>
                             : box_paths ? k6_resolve<false, false, true> : k6_resolve<false, false>;
        const HalfSweep *sweep = bounded ? (const HalfSweep *)g_sweep.p : nullptr;
        for (;;) {
            HIP_TRY(hipMemsetAsync(g_cnt.p, 0, 16, st));
            unsigned int *njobs = (unsigned int *)g_cnt.p, *remaining = njobs + 1, *novf = njobs + 2;
            pv.blk = (const PathBlock *)g_arena.p;   // the arena may have grown in the last round
            hipLaunchKernelGGL(pick, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint2 *)g_anchors.p, (const mimeo_alignment *)d_aln,
                               bmax, (uint8_t *)g_astate.p, (uint8_t *)g_astate.p + nhsps, (DpJob *)g_jobs.p, njobs, pv);
            unsigned int h0 = 0;   // jobs of the round
            HIP_TRY(hipMemcpyAsync(&h0, njobs, 4, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            if (h0) {
                const BoundCtx bc{(const mimeo_alignment *)d_aln, (const uint2 *)g_anchors.p, pv};
                if ((rc = dp_round(d_groups, h0, p, cap, bounded, bc, novf))) return rc;
                if (k6_stats && (rc = round_stats(h0, nhsps, bounded, &bound_jobs))) return rc;
                if (path) {
                    rounds++;
                    if ((rc = trace_round(d_groups, (const DpJob *)g_jobs.p, h0, p, pool_budget, &arena_used, &ms_trace, &trace_slices, &largest, bounded, bc))) return rc;
                    pv.blk = (const PathBlock *)g_arena.p;
                }
            }
            hipLaunchKernelGGL(resolve, dim3(ngroups), dim3(64), 0, st, d_groups, (const uint2 *)g_anchors.p, (const HalfResult *)g_res.p,
                               d_aln, (uint8_t *)g_astate.p, remaining, pv, sweep);
            unsigned int h4[4] = {0, 0, 0, 0};
            HIP_TRY(hipMemcpyAsync(h4, g_cnt.p, 16, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            rescheduled += h4[3];
            if (!h4[1]) break;
        }
        if (path && k6_stats) {
            fprintf(stderr, "[k6] path rule: traceback %.3f ms, rounds %u slices %u, %llu path blocks, pool %.1f MB, largest half %.3f MB", ms_trace,
                    rounds, trace_slices, (unsigned long long)arena_used, g_pool.cap / 1048576.0, largest / 1048576.0);
            if (bounded) fprintf(stderr, ", bounded jobs %llu, rescheduled %llu", bound_jobs, rescheduled);
            fprintf(stderr, "\n");
        }
        if (box_paths && (rc = paths_pass(d_groups, ngroups, p, d_aln, pool_budget, k6_stats))) return rc;
    }
    if (want_paths)
        hipLaunchKernelGGL(k6_kept_ranks, dim3((ngroups + 63) / 64), dim3(64), 0, st, d_groups, ngroups, (const mimeo_alignment *)d_aln,
                           (uint32_t *)g_accrank.p, (const uint2 *)g_pidx.p, p->hspthresh);
    hipLaunchKernelGGL(k6_finish, dim3((ngroups + 63) / 64), dim3(64), 0, st, d_groups, ngroups, d_aln, p->hspthresh);
    HIP_TRY(hipGetLastError());
    return 0;
}

}  // namespace mimeo
