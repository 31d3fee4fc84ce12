// K6: the band DP of the two workgroup kernels, k6_dp_any (k6_dp.hip) and k6_trace (k6_trace.hip), written once: one workgroup, two
// rows held as a ring of columns, three passes per row with the rules and tie-breaks of wave_half_extend_2048.  band_dp computes the
// scores and the decisions they were made by; what travels beside a score is the caller's payload PL (inline members; M: its ring
// mask, W: the widest row it holds beside the ring): rows() names the two rows' scores, init() writes row 0, h() takes pass 1's
// decisions (D live above, D opened from C, a diagonal step and whether it matches, H took D) and returns what H carries (the nm / nx
// of a Cell), htag() returns that again in pass 3, c() takes "C took the insertion arriving as ia, else H" and returns what C carries.
#pragma once
#include "k6.h"

namespace mimeo {

struct BandRows { int32_t *pc, *pd, *nc, *nd; };   // C and D of the previous and of the current row, indexed by column & M
// Rows 1 .. lastrow of the half `job` of group G by the whole workgroup of THREADS; every thread returns the same: the result as
// k6_dp_any reports it (overflow: a row that the ring or the payload does not hold) and what was swept.  BOUND
// (mimeo_params.bound_extensions): cells outside the row's allowed interval (bounds_at) are dead in all three states
template <int THREADS, bool BOUND, class PL>
__device__ __forceinline__ HalfResult band_dp(PL &pl, const Group &G, const DpJob &job, uint32_t lastrow, int32_t O, int32_t E, int32_t Y, int32_t cap,
                                              const BoundCtx &B, HalfSweep &sw) {
    __shared__ struct { Cell scan[THREADS / 64]; Best4 best[THREADS / 64]; uint32_t first[THREADS / 64], last[THREADS / 64]; } S;
    const GStrandView T = G.T, Q = G.Q;
    const int dir = job.dir;
    const uint32_t at = job.at, aq = job.aq, lenB = dir > 0 ? Q.len - aq : aq, nacc = BOUND ? G.nacc : 0u;
    const uint64_t b0 = G.hsp_begin;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6, M = pl.M;
    HalfResult r{0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    sw = HalfSweep{INT32_MAX, INT32_MIN, nacc, 0};
    long long sbase = 0;   // the cells are 32 bits wide and stand above this (below)
    // row 0: C(0,j) = -O - j*E while that is within the y-drop
    uint32_t lo = 0, hi = 0;
    if (Y >= O + E) hi = min(lenB, (uint32_t)((Y - O) / E));
    const uint32_t ext = (uint32_t)((Y + 200) / E) + 2u;  // how far an insertion can carry a live cell to the right
    if (min(lenB, hi + ext) + 2u > M) { r.overflow = 1; return r; }   // no row can hold more live columns than the query has left
    for (uint32_t j = tid; j <= hi; j += THREADS) pl.init(j, j ? -O - (int32_t)j * E : 0);
    __syncthreads();
    uint32_t par = 0, bnext = 1u;
    long long bkmin = -K_INF, bkmax = K_INF;
    for (uint32_t i = 1; i <= lastrow; i++, par ^= 1u) {
        if (BOUND && i == bnext) {
            const RowBound rb = bounds_at(B, b0, nacc, at, aq, dir, i);
            bkmin = rb.kmin; bkmax = rb.kmax; bnext = rb.next;
        }
        if (BOUND && (bkmin > -K_INF || bkmax < K_INF)) sw.nbound++;
        const long long jlo = bkmin + (long long)i + 1, jhi = bkmax + (long long)i - 1;   // the allowed columns
        const int32_t thr = r.score - Y;
        const Base1 ab = base_at(T, dir > 0 ? (int32_t)(at + i - 1) : (int32_t)(at - i));
        const uint32_t alo = ab.lo, ahi = ab.hi, an = ab.nm, acg = alo ^ ahi;
        const uint32_t hx = min(lenB, hi + 1u + ext);  // last column that can be alive in this row
        const uint32_t ncols = hx - lo + 1u;
        if (ncols + 2u > M || ncols > pl.W) { r.overflow = 1; break; }
        const BandRows R = pl.rows(par, i, lo);
        // every thread owns one contiguous chunk of the row's columns (the insertion scan runs left to right)
        const uint32_t chunk = (ncols + THREADS - 1) / THREADS;
        const uint32_t j0 = lo + tid * chunk, j1 = min(hx + 1u, j0 + chunk);  // [j0, j1), possibly empty
        // pass 1: D and H = max(diagonal, D) from the previous row (dead outside [lo, hi])
        Cell run{NEG, 0, 0};
        for (uint32_t j = j0; j < j1; j++) {
            const bool in = j <= hi;  // j >= lo holds
            const int32_t cp = in ? R.pc[j & M] : NEG, dp = in ? R.pd[j & M] : NEG;
            int32_t dd = NEG, g = NEG;
            const bool dlive = dp > NEGH;
            if (dlive) dd = dp - E;
            const bool dopen = cp > NEGH && cp - O - E > dd;
            if (dopen) dd = cp - O - E;
            bool diag = false, m = false;
            if (j >= 1 && j - 1 >= lo && j - 1 <= hi) {
                const int32_t pc = R.pc[(j - 1) & M];
                if (pc > NEGH) {
                    const Base1 qb = base_at(Q, dir > 0 ? (int32_t)(aq + j - 1) : (int32_t)(aq - j));
                    const uint32_t dl = alo ^ qb.lo, dh = ahi ^ qb.hi, nn = an | qb.nm;
                    diag = true;
                    m = !(dl | dh | nn);
                    g = pc + sub_score(dl, dh, acg, nn);
                }
            }
            if (BOUND && ((long long)j < jlo || (long long)j > jhi)) { dd = NEG; g = NEG; }
            const bool hd = dd > g;  // diagonal preferred on ties
            const int32_t hh = hd ? dd : g;
            const Cell ht = pl.h(j, dlive, dopen, diag, m, hd);
            R.nd[j & M] = dd;
            R.nc[j & M] = hh;
            const Cell u{hh > NEGH ? hh + (int32_t)(j - lo) * E : NEG, ht.nm, ht.nx};
            run = cmax_left(run, u);
        }
        // pass 2: exclusive max-plus scan of the chunk aggregates over the workgroup (ties to the left)
        const Cell winc = wave_incl_maxscan(run);
        if (lane == 63) S.scan[wave] = winc;
        __syncthreads();
        Cell acc{NEG, 0, 0};
        for (uint32_t w = 0; w < wave; w++) acc = cmax_left(acc, S.scan[w]);
        acc = cmax_left(acc, dpp_cell<0x138, 0xf>(winc));  // best u of every column left of my chunk
        // pass 3: C = max(H, I), prune, row statistics
        Best4 rb{NEG, 0xFFFFFFFFu, 0, 0};
        uint32_t myfirst = 0xFFFFFFFFu, mylast = 0;
        for (uint32_t j = j0; j < j1; j++) {
            const int32_t hh = R.nc[j & M];
            const Cell ht = pl.htag(j), ia = acc;
            const int32_t I = ia.s > NEGH ? ia.s - O - (int32_t)(j - lo) * E : NEG;
            const Cell u{hh > NEGH ? hh + (int32_t)(j - lo) * E : NEG, ht.nm, ht.nx};
            acc = cmax_left(acc, u);
            const bool ci = I > hh;  // H preferred over I on ties
            const int32_t c = ci ? I : hh;
            const bool alive = c >= thr && c > NEGH && (!BOUND || ((long long)j >= jlo && (long long)j <= jhi));
            const Cell ct = pl.c(j, ht, ia, ci);
            R.nc[j & M] = alive ? c : NEG;
            if (!alive) R.nd[j & M] = NEG;
            if (alive) {
                if (myfirst == 0xFFFFFFFFu) myfirst = j;
                mylast = j;
                if (c > rb.s) { rb.s = c; rb.j = j; rb.nm = ct.nm; rb.nx = ct.nx; }
            }
        }
        // workgroup reductions: first / last live column, best cell (smallest column on ties: chunks grow with tid)
        uint32_t wf = myfirst, wl = (myfirst == 0xFFFFFFFFu) ? 0u : mylast + 1u;  // last + 1 so that 0 = none
        for (int o = 32; o > 0; o >>= 1) { wf = min(wf, (uint32_t)__shfl_xor((int)wf, o)); wl = max(wl, (uint32_t)__shfl_xor((int)wl, o)); }
        const Best4 wb4 = wave_best(rb);
        if (lane == 0) { S.first[wave] = wf; S.last[wave] = wl; S.best[wave] = wb4; }
        __syncthreads();
        uint32_t first_alive = 0xFFFFFFFFu, last1 = 0;
        Best4 tb{NEG, 0xFFFFFFFFu, 0, 0};
        for (int w = 0; w < THREADS / 64; w++) {
            first_alive = min(first_alive, S.first[w]);
            last1 = max(last1, S.last[w]);
            const Best4 o = S.best[w];
            if (o.s > tb.s || (o.s == tb.s && o.j < tb.j)) tb = o;
        }
        __syncthreads();  // the LDS arrays are rewritten in the next row
        if (first_alive == 0xFFFFFFFFu) break;
        lo = first_alive;
        hi = last1 - 1u;
        r.maxcols = max(r.maxcols, hi - lo + 1u);
        r.rows = i;
        if (BOUND) {
            sw.klo = min(sw.klo, (int32_t)((long long)lo - (long long)i));
            sw.khi = max(sw.khi, (int32_t)((long long)hi - (long long)i));
        }
        if (tb.s > r.score) { r.score = tb.s; r.i = i; r.j = tb.j; r.nm = tb.nm; r.nx = tb.nx; }
        // The cells are 32 bits wide (as lastz's own score_t, which wraps there).  Every live cell of a row lies within the
        // y-drop of the best score so far, so when that nears the cap the whole row — and the best score — is moved down by
        // half the cap and `sbase` up: comparisons inside a row and between neighbouring rows never see the difference, and
        // the half's score is sbase + best.score in 64 bits
        if (r.score > cap) {
            const int32_t K = cap / 2;
            for (uint32_t j = lo + tid; j <= hi; j += THREADS) {
                if (R.nc[j & M] > NEGH) R.nc[j & M] -= K;
                if (R.nd[j & M] > NEGH) R.nd[j & M] -= K;
            }
            r.score -= K;
            sbase += K;
            __syncthreads();
        }
    }
    r.base_lo = (uint32_t)(unsigned long long)sbase;
    r.base_hi = (uint32_t)((unsigned long long)sbase >> 32);
    return r;
}

}  // namespace mimeo
