// K6: the DP kernels of a half extension and the round's cascade over them (dp_round); k6_gapped.hip has the overview.
#include "k6_band.h"

namespace mimeo {

// WSTRIP query bits for columns jb .. jb+WSTRIP-1 (bit s <-> column jb+s); column j consumes query base
// aq + j - 1 (dir > 0) or aq - j (dir < 0).  Out-of-range columns read padding and are never used.
template <int WSTRIP>
__device__ __forceinline__ void load_qbits(const GStrandView &Q, uint32_t aq, int dir, uint32_t jb, uint32_t lenB,
                                           uint32_t &qlo, uint32_t &qhi, uint32_t &qn) {
    constexpr uint32_t SMASK = WSTRIP == 32 ? 0xFFFFFFFFu : ((1u << (WSTRIP & 31)) - 1u);  // WSTRIP in {7, 14, 32}
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
// The strip width WS is a template parameter: a row costs about 36 * WS + 85 VALU instructions whatever part of its
// 64 * WS columns is live, and the widest row of a half comes late: the deletion side of the band stays ~70 columns wide
// while the best score keeps growing and reaches 300 only when the repeat ends.  So k6_dp1 starts a half at L_W1 = L_WS / 2
// columns per lane (lean_dp<L_W1>, a 448-column window).  When a row ends with the last strip but one live, that row is
// still complete: the wavefront lays its state out at L_WS (lean_widen) and goes on with the next row.  When the band
// outgrows the narrow window in row 0, or reaches the last strip from further down in one row, the wavefront runs the half
// again from row 1 at L_WS.  Only a half that outgrows L_WS is reported as an overflow.  Which lane holds a column
// changes no cell, so the result does not depend on the width; and because a strip of L_W1 columns never straddles a
// multiple of L_WS and the handover moves the window base down to one, the windows at L_WS, the overflow test and maxcols
// are those of a pass that ran at L_WS from row 0.
constexpr int L_WS = 14;   // the full width: k6_dp1_bounded, and k6_dp1 from the handover on
constexpr int L_W1 = 7;    // k6_dp1's first rows
static_assert(2 * L_W1 == L_WS, "lean_widen pairs up strips of L_W1 columns, and maxcols is counted in whole strips of L_WS");
constexpr uint32_t LEAN_BAND = 1u, LEAN_ROWS = 2u, LEAN_WIDEN = 3u;   // why lean_dp left: the window (row 0 or a later row), the 16-bit counts, a handover
struct ScoreTab { uint32_t t0, t1, t2, t3; };         // biased score bytes of the four query bases for each target base (index lo | hi << 1)
template <int WS>
struct LeanState {
    int32_t C[WS], D[WS];
    uint32_t Cc[WS], Dc[WS], sel[WS];
};
struct LeanHandover {   // where a pass at half the width stood when its band reached the last strip but one: the rows done, the window base
    HalfResult best;
    uint32_t rows, wb;
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
template <int WS>
__device__ __forceinline__ void lean_selectors(LeanState<WS> &S, uint32_t qlo, uint32_t qhi, uint32_t qn) {
#pragma unroll
    for (int s = 0; s < WS; s++) {
        const uint32_t idx = ((qlo >> s) & 1u) | (((qhi >> s) & 1u) << 1);
        S.sel[s] = 0x0C0C0C00u | (((qn >> s) & 1u) ? 4u : idx);
    }
}

// one DP row; returns the lane's row maximum (NEG when none of its cells is live).  BND (bounded extension, with EDGE):
// exmask also clears the slots outside the row's allowed interval, and their H is dead before the insertion pass: the
// forbidden cells are a prefix and a suffix of the row, so H masked after pass 1 and C / D after pass 3 is the rule
template <int WS, bool EDGE, bool BND = false>
__device__ __forceinline__ int32_t lean_row(LeanState<WS> &S, uint32_t srow, int32_t O, int32_t E, int32_t thr, uint32_t exmask,
                                            int32_t lane_base, int32_t kneg128) {
    const int32_t OE = O + E;
    // C of the column left of my strip (previous row): last slot of the previous lane
    PCell pc = dpp_pcell<0x138, 0xf>(PCell{S.C[WS - 1], S.Cc[WS - 1]});
    // pass 1 (slots descending, in place): D and H = max(diagonal, D); slot s still sees the old C of slot s - 1
#pragma unroll
    for (int s = WS - 1; s >= 0; s--) {
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
    for (int s = 0; s < WS; s++) {
        const bool take = S.C[s] > run.s;  // ties -> left
        run.c = take ? S.Cc[s] : run.c;
        run.s = max(run.s, S.C[s]) - E;
    }
    run.s += lane_base;  // common frame: column 0 of the window
    PCell acc = dpp_pcell<0x138, 0xf>(lean_incl_maxscan(run));  // best of every column left of my strip
    acc.s += WS * E - lane_base;                                   // ... as it arrives at my first column
    // pass 3: C = max(H, I), prune, row maximum
    int32_t rowmax = NEG;
#pragma unroll
    for (int s = 0; s < WS; s++) {
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

// row 0 of a half in a fresh window at column 0: C(0, j) = -O - j E while that stays within the y-drop; false when it does not fit
template <int WS>
__device__ __forceinline__ bool lean_row0(const GStrandView &Q, uint32_t aq, int dir, uint32_t lenB, int32_t O, int32_t E, int32_t Y,
                                          LeanState<WS> &S) {
    const uint32_t jb = (threadIdx.x & 63u) * WS;
    uint32_t qlo, qhi, qn;
    load_qbits<WS>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
    lean_selectors<WS>(S, qlo, qhi, qn);
    bool over = false;
#pragma unroll
    for (int s = 0; s < WS; s++) {
        const uint32_t j = jb + s;
        const int32_t v = j ? -O - (int32_t)j * E : 0;
        const bool alive = j <= lenB && (j == 0 || v >= -Y);
        S.C[s] = alive ? v : NEG; S.Cc[s] = 0;
        S.D[s] = NEG; S.Dc[s] = 0;
        if (alive && j >= (uint32_t)(64 * WS - WS)) over = true;
    }
    return __ballot(over) == 0;
}

// The row loop of the lean kernel at WS columns per lane.  S holds row ho.rows of the half in the window at column ho.wb, ho.best what
// the rows so far came to (row 0: lean_row0 and a zeroed ho).  The result's overflow says why the pass left before the half was
// done (LEAN_BAND, LEAN_ROWS; LEAN_WIDEN: ho then says where it stands), 0 when it is done.  BOUND (WS == L_WS only): the
// extension is bounded by the group's nacc accepted alignments (bounds_at); *sw receives what it swept.
// maxcols is always the figure of the L_WS layout, 14 * (max over rows of hi_i / 14 - lo_{i-1} / 14 + 1) with the first / last live
// column of a row: the window base and the last live strip give those two quotients at either width.
template <int WS, bool BOUND>
__device__ __forceinline__ HalfResult lean_dp(const GStrandView &T, const GStrandView &Q, uint32_t at, uint32_t aq, int dir, int32_t O,
                                              int32_t E, int32_t Y, const ScoreTab tab, const BoundCtx &B, uint64_t b0, uint32_t nacc,
                                              HalfSweep *sw, LeanState<WS> &S, LeanHandover &ho) {
    static_assert(!BOUND || WS == L_WS, "the bounded kernel runs at the full width");
    constexpr int WINDOW = 64 * WS;
    constexpr bool WIDENS = WS == L_W1;   // the pass hands over to L_WS instead of giving up
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t lenA = dir > 0 ? T.len - at : at, lenB = dir > 0 ? Q.len - aq : aq;
    HalfResult best = ho.best;
    best.overflow = 0;
    uint32_t wb = ho.wb, jb = wb + lane * WS;
    const uint32_t i0 = ho.rows + 1u;
    const int32_t lane_base = (int32_t)(lane * WS) * E;
    const int32_t kneg128 = __builtin_amdgcn_readfirstlane(-128);
    uint32_t exmask = (1u << WS) - 1u;
    bool edge = wb + (uint32_t)WINDOW - 1u > lenB;
    if (edge) {
        exmask = 0;
#pragma unroll
        for (int s = 0; s < WS; s++) exmask |= (jb + s <= lenB ? 1u : 0u) << s;
    }
    long long bkmin = -K_INF, bkmax = K_INF;   // BOUND: the allowed interval of k = j - i, and the row where it is looked up again
    uint32_t bnext = 1u;
    int32_t klo = INT32_MAX, khi = INT32_MIN;
    const uint32_t blk = ((i0 - 1u) & ~31u) + 1u;   // first row of the block of 32 target bases that holds row i0
    RowBases rbase{0, 0, 0}, rnext = load_row_bases(T, at, dir, blk);
    if ((i0 - 1u) & 31u) { rbase = rnext; rnext = load_row_bases(T, at, dir, blk + 32u); }
    for (uint32_t i = i0; i <= lenA; i++) {
        // the packed counts hold 16 bits each: a longer extension is redone by the wide kernel (unpacked counts)
        if (i >= 0xFFFFu) { best.overflow = LEAN_ROWS; break; }
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
        uint32_t srow = a & 2u ? (a & 1u ? tab.t3 : tab.t2) : (a & 1u ? tab.t1 : tab.t0);
        if ((rnm >> rbit) & 1u) srow = 0x1C1C1C1Cu;
        // BOUND: the allowed columns of this row are jlo .. jhi; only rows in which they cut the window run the masked variant
        uint32_t bm = 0;
        bool cut = false;
        if (BOUND) {
            const long long jlo = bkmin + (long long)i + 1, jhi = bkmax + (long long)i - 1;
            if (bkmin > -K_INF || bkmax < K_INF) sw->nbound++;
            cut = jlo > (long long)wb || jhi < (long long)wb + (WINDOW - 1);
            const long long r0 = jlo - (long long)jb, r1 = jhi - (long long)jb + 1;
            const uint32_t s0 = (uint32_t)min(max(r0, 0ll), (long long)WS), s1 = (uint32_t)min(max(r1, 0ll), (long long)WS);
            bm = ((1u << s1) - 1u) & ~((1u << s0) - 1u) & exmask;   // exmask: all slots, or those within the query
        }
        const int32_t rowmax = BOUND && cut ? lean_row<WS, true, true>(S, srow, O, E, thr, bm, lane_base, kneg128)
                               : edge ? lean_row<WS, true>(S, srow, O, E, thr, exmask, lane_base, kneg128)
                                      : lean_row<WS, false>(S, srow, O, E, thr, exmask, lane_base, kneg128);
        const uint64_t ball = __ballot(rowmax > NEGH);
        if (!ball) break;
        const uint32_t rf = (uint32_t)__builtin_ctzll(ball), rl = 63u - (uint32_t)__builtin_clzll(ball);
        if (rl == 63u) { best.overflow = LEAN_BAND; break; }
        if constexpr (WS == L_WS) {
            best.maxcols = max(best.maxcols, (rl + 1u) * WS);
        } else {   // no strip straddles a multiple of L_WS
            best.maxcols = max(best.maxcols, ((wb + rl * WS) / L_WS + 1u - wb / L_WS) * L_WS);
        }
        best.rows = i;
        if (BOUND) {   // the strips with a live cell, as diagonals of this row
            klo = min(klo, (int32_t)((long long)wb + rf * WS - (long long)i));
            khi = max(khi, (int32_t)((long long)wb + (rl + 1u) * WS - 1 - (long long)i));
        }
        const int32_t wmax = wave_max_i32(rowmax);
        if (wmax > best.score) {
            // the cell: lowest lane holding the maximum, smallest slot in it (smallest column on ties)
            const uint32_t L = (uint32_t)__builtin_ctzll(__ballot(rowmax == wmax));
            uint32_t slot = 0, cnt = 0;
#pragma unroll
            for (int s = WS - 1; s >= 0; s--) {
                const int32_t v = __builtin_amdgcn_readlane(S.C[s], (int)L);
                if (v == wmax) { slot = (uint32_t)s; cnt = (uint32_t)__builtin_amdgcn_readlane((int)S.Cc[s], (int)L); }
            }
            best.score = wmax; best.i = i; best.j = wb + L * WS + slot; best.nm = cnt & 0xFFFFu; best.nx = (cnt >> 16) - (cnt & 0xFFFFu);
        }
        // slide the window so that it starts at the strip holding the first live column
        if (rf) {
            wb += rf * WS;
            jb = wb + lane * WS;
            const int src = (int)((lane + rf) & 63u);
            const bool fresh = lane + rf >= 64u;  // strip re-enters on the right with new columns
#pragma unroll
            for (int s = 0; s < WS; s++) {
                const int32_t cs = __shfl(S.C[s], src), ds = __shfl(S.D[s], src);
                S.Cc[s] = __shfl(S.Cc[s], src); S.Dc[s] = __shfl(S.Dc[s], src);
                S.sel[s] = __shfl(S.sel[s], src);
                S.C[s] = fresh ? NEG : cs;
                S.D[s] = fresh ? NEG : ds;
            }
            if (fresh) {
                uint32_t qlo, qhi, qn;
                load_qbits<WS>(Q, aq, dir, jb, lenB, qlo, qhi, qn);
                lean_selectors<WS>(S, qlo, qhi, qn);
            }
            edge = wb + (uint32_t)WINDOW - 1u > lenB;
            if (edge) {
                exmask = 0;
#pragma unroll
                for (int s = 0; s < WS; s++) exmask |= (jb + s <= lenB ? 1u : 0u) << s;
            } else if (BOUND) exmask = (1u << WS) - 1u;
        }
        // the last strip but one is live and the last one dead: the row is complete, the next one may not be.  Hand over
        if (WIDENS && rl == 62u) { best.overflow = LEAN_WIDEN; ho.best = best; ho.rows = i; ho.wb = wb; break; }
    }
    if (BOUND) { sw->klo = klo; sw->khi = khi; }
    return best;
}

// the state of a pass at L_W1 = L_WS / 2 columns per lane in the window at wb, laid out at L_WS: the window base moves down to a multiple
// of L_WS (so the pass that goes on has the windows of a pass that started at L_WS), new lane L takes the old lanes 2L - odd and
// 2L + 1 - odd, and what lies outside the old window enters dead, as strips that slide in on the right do
__device__ __forceinline__ void lean_widen(const LeanState<L_W1> &N, LeanState<L_WS> &S, uint32_t &wb, const GStrandView &Q, uint32_t aq,
                                           int dir, uint32_t lenB) {
    const uint32_t lane = threadIdx.x & 63u;
    const int odd = (int)((wb / L_W1) & 1u);
    wb -= (uint32_t)odd * L_W1;
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int src = 2 * (int)lane + h - odd;
        const bool dead = src < 0 || src > 63;
#pragma unroll
        for (int s = 0; s < L_W1; s++) {
            const int32_t cs = __shfl(N.C[s], src & 63), ds = __shfl(N.D[s], src & 63);
            S.Cc[h * L_W1 + s] = __shfl(N.Cc[s], src & 63); S.Dc[h * L_W1 + s] = __shfl(N.Dc[s], src & 63);
            S.C[h * L_W1 + s] = dead ? NEG : cs;
            S.D[h * L_W1 + s] = dead ? NEG : ds;
        }
    }
    uint32_t qlo, qhi, qn;
    load_qbits<L_WS>(Q, aq, dir, wb + lane * L_WS, lenB, qlo, qhi, qn);
    lean_selectors<L_WS>(S, qlo, qhi, qn);
}

// A half extension by one wavefront: the shortcut, else lean_dp.  Unbounded: at L_W1 first; a pass at half the width hands over to
// L_WS when its band reaches the last strip but one (*event = LEAN_WIDEN), and a half whose band outgrew the first window in row 0
// or in one row runs again from row 1 at L_WS (*event = LEAN_BAND).  The result's overflow is 1 when the half needs the next kernel.
template <bool BOUND>
__device__ HalfResult wave_half_extend_lean(const GStrandView &T, const GStrandView &Q, uint32_t at, uint32_t aq, int dir,
                                            int32_t O, int32_t E, int32_t Y, const BoundCtx &B, uint64_t b0, uint32_t nacc,
                                            HalfSweep *sw, uint32_t *event) {
    HalfResult best{0, 0, 0, 0, 0, 0, 0, 0};
    if (BOUND) *sw = HalfSweep{0, 0, nacc, 0};
    // a bounded half may take the exact shortcut only when no earlier alignment reaches into its rows
    if ((!BOUND || bounds_none(B, b0, nacc, at, dir)) && identical_suffix(T, Q, at, aq, dir, best)) return best;
    uint32_t t[4];
#pragma unroll
    for (uint32_t a = 0; a < 4; a++) {
        uint32_t w = 0;
#pragma unroll
        for (uint32_t b = 0; b < 4; b++) {
            const uint32_t alo = a & 1u, ahi = a >> 1, dl = alo ^ (b & 1u), dh = ahi ^ (b >> 1);
            w |= (uint32_t)(sub_score(dl, dh, alo ^ ahi, 0u) + 128) << (8u * b);
        }
        t[a] = w;
    }
    const ScoreTab tab{t[0], t[1], t[2], t[3]};
    const uint32_t lenB = dir > 0 ? Q.len - aq : aq;
    LeanState<L_WS> S;
    LeanHandover ho{best, 0u, 0u};
    bool full0 = true;   // the full-width pass starts at row 0
    if constexpr (!BOUND) {
        LeanState<L_W1> N;
        if (lean_row0<L_W1>(Q, aq, dir, lenB, O, E, Y, N)) {
            best = lean_dp<L_W1, false>(T, Q, at, aq, dir, O, E, Y, tab, B, b0, nacc, sw, N, ho);
            if (best.overflow == 0u || best.overflow == LEAN_ROWS) { best.overflow = best.overflow ? 1u : 0u; return best; }
        } else best.overflow = LEAN_BAND;
        if (best.overflow == LEAN_WIDEN) {
            lean_widen(N, S, ho.wb, Q, aq, dir, lenB);
            full0 = false;
            *event = LEAN_WIDEN;
        } else {
            ho = LeanHandover{HalfResult{0, 0, 0, 0, 0, 0, 0, 0}, 0u, 0u};
            *event = LEAN_BAND;
        }
    }
    if (full0 && !lean_row0<L_WS>(Q, aq, dir, lenB, O, E, Y, S)) { best = HalfResult{0, 0, 0, 0, 0, 0, 0, 0}; best.overflow = 1u; return best; }
    best = lean_dp<L_WS, BOUND>(T, Q, at, aq, dir, O, E, Y, tab, B, b0, nacc, sw, S, ho);
    best.overflow = best.overflow ? 1u : 0u;
    return best;
}

// nrestart[0] counts the halves that ran a second time at the full width, nrestart[1] those that went on at it (MIMEO_K6_STATS)
__global__ __launch_bounds__(64) void k6_dp1(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                             HalfResult *__restrict__ res, int32_t O, int32_t E, int32_t Y,
                                             unsigned int *__restrict__ nrestart) {
    const DpJob job = jobs[blockIdx.x];
    const Group &G = groups[job.group];
    uint32_t event = 0;
    HalfResult r = wave_half_extend_lean<false>(G.T, G.Q, job.at, job.aq, job.dir, O, E, Y, BoundCtx{}, 0, 0, nullptr, &event);
    if (threadIdx.x == 0) {
        res[job.slot] = r;
        if (event) atomicAdd(nrestart + (event == LEAN_WIDEN ? 1 : 0), 1u);
    }
}

// k6_dp1 under mimeo_params.bound_extensions.  A half that does not fit (band, rows) goes on to k6_dp_any<true>
__global__ __launch_bounds__(64) void k6_dp1_bounded(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                     HalfResult *__restrict__ res, HalfSweep *__restrict__ sweep, int32_t O, int32_t E,
                                                     int32_t Y, BoundCtx B, unsigned int *__restrict__ novf,
                                                     unsigned int *__restrict__ ovf_list) {
    const DpJob job = jobs[blockIdx.x];
    const Group &G = groups[job.group];
    HalfSweep sw;
    HalfResult r = wave_half_extend_lean<true>(G.T, G.Q, job.at, job.aq, job.dir, O, E, Y, B, G.hsp_begin, G.nacc, &sw, nullptr);
    if (threadIdx.x == 0) {
        res[job.slot] = r;
        sweep[job.slot] = sw;
        if (r.overflow) ovf_list[atomicAdd(novf, 1u)] = blockIdx.x;
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
// with the same rules and tie-breaks as wave_half_extend_2048 (band_dp, k6_band.h: the row loop it shares with k6_trace).  Slow (a few microseconds per row plus ~1 ns per
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

// band_dp's payload: match / mismatch counts beside every score (identity needs no traceback)
struct CountRows {
    static constexpr uint32_t M = ANY_COLS - 1u, W = ANY_COLS;   // the ring is the only limit of a row
    uint32_t *base;
    AnyRow P, N;
    __device__ __forceinline__ BandRows rows(uint32_t par, uint32_t, uint32_t) {
        P = any_row(base, par); N = any_row(base, par ^ 1u);
        return BandRows{P.cs, P.ds, N.cs, N.ds};
    }
    __device__ __forceinline__ void init(uint32_t j, int32_t c) {
        const AnyRow r0 = any_row(base, 0);
        r0.cs[j & M] = c; r0.cm[j & M] = 0; r0.cx[j & M] = 0;
        r0.ds[j & M] = NEG; r0.dm[j & M] = 0; r0.dx[j & M] = 0;
    }
    __device__ __forceinline__ Cell h(uint32_t j, bool dlive, bool dopen, bool diag, bool m, bool hd) const {
        Cell dd{0, 0, 0}, g{0, 0, 0};
        if (dlive) { dd.nm = P.dm[j & M]; dd.nx = P.dx[j & M]; }
        if (dopen) { dd.nm = P.cm[j & M]; dd.nx = P.cx[j & M]; }
        if (diag) { g.nm = P.cm[(j - 1) & M] + (m ? 1u : 0u); g.nx = P.cx[(j - 1) & M] + (m ? 0u : 1u); }
        N.dm[j & M] = dd.nm; N.dx[j & M] = dd.nx;
        const Cell hh = hd ? dd : g;
        N.cm[j & M] = hh.nm; N.cx[j & M] = hh.nx;
        return hh;
    }
    __device__ __forceinline__ Cell htag(uint32_t j) const { return Cell{0, N.cm[j & M], N.cx[j & M]}; }
    __device__ __forceinline__ Cell c(uint32_t j, const Cell &ht, const Cell &ia, bool ci) const { const Cell ct = ci ? ia : ht; N.cm[j & M] = ct.nm; N.cx[j & M] = ct.nx; return ct; }
};

// BOUND (mimeo_params.bound_extensions): the half is bounded by the group's accepted alignments; sweep receives what it swept
template <bool BOUND>
__global__ __launch_bounds__(ANY_THREADS) void k6_dp_any(const Group *__restrict__ groups, const DpJob *__restrict__ jobs,
                                                         const unsigned int *__restrict__ list, uint32_t first,
                                                         HalfResult *__restrict__ res, uint32_t *__restrict__ scratch,
                                                         int32_t O, int32_t E, int32_t Y, int32_t cap, BoundCtx B,
                                                         HalfSweep *__restrict__ sweep) {
    const DpJob job = jobs[list[first + blockIdx.x]];
    const Group &G = groups[job.group];
    const uint32_t lenA = job.dir > 0 ? G.T.len - job.at : job.at;
    CountRows rows{scratch + (size_t)blockIdx.x * ANY_SLOT_WORDS};
    HalfSweep sw;
    const HalfResult r = band_dp<ANY_THREADS, BOUND>(rows, G, job, lenA, O, E, Y, cap, B, sw);
    if (threadIdx.x == 0) res[job.slot] = r;
    if (BOUND && threadIdx.x == 0) sweep[job.slot] = sw;
}

// bounded extensions with penalties outside the lean kernel's domain: every job of the round goes to k6_dp_any<true>
__global__ void k6_list_all(uint32_t n, unsigned int *__restrict__ novf, unsigned int *__restrict__ ovf_list) {
    const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k < n) ovf_list[k] = k;
    if (k == 0) *novf = n;
}

// The DP kernels of a round over its n jobs, each taking the jobs that the one before could not hold: the lean kernel, the
// 2048-column kernel (not in bounded mode: it knows no bounds), the global-memory kernel.  The lean kernel's dead-cell
// arithmetic needs the penalties to stay far below 2^29 / 1024; beyond that every job starts at the second kernel of its mode.
int dp_round(Group *d_groups, uint32_t n, const mimeo_params *p, int32_t cap, bool bounded, const BoundCtx &bc,
                    unsigned int *novf, unsigned int *nrestart) {
    hipStream_t st = stream();
    int rc;
    const Group *groups = d_groups;
    const DpJob *jobs = (const DpJob *)g_k6.jobs.p;
    HalfResult *res = (HalfResult *)g_k6.res.p;
    HalfSweep *sweep = bounded ? (HalfSweep *)g_k6.sweep.p : nullptr;
    unsigned int *list = (unsigned int *)g_k6.ovf_list.p;
    const int32_t O = p->gap_open, E = p->gap_extend, Y = p->ydrop;
    const bool lean_ok = E <= (1 << 16) && O <= (1 << 24) && Y <= (1 << 28);
    if (bounded) {
        if (lean_ok) hipLaunchKernelGGL(k6_dp1_bounded, dim3(n), dim3(64), 0, st, groups, jobs, res, sweep, O, E, Y, bc, novf, list);
        else hipLaunchKernelGGL(k6_list_all, dim3((n + 255) / 256), dim3(256), 0, st, n, novf, list);
    } else {
        if (lean_ok) hipLaunchKernelGGL(k6_dp1, dim3(n), dim3(64), 0, st, groups, jobs, res, O, E, Y, nrestart);
        hipLaunchKernelGGL(k6_dp_wide, dim3(n), dim3(64), 0, st, groups, jobs, res, O, E, Y, novf, list, cap, lean_ok ? 0 : 1);
    }
    // bands beyond 2048 columns (tandem arrays): the global-memory kernel, a few jobs at a time
    unsigned int nov = 0;
    HIP_TRY(hipMemcpyAsync(&nov, novf, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!nov) return 0;
    const unsigned int slots = std::min<unsigned int>(nov, 32u);
    if ((rc = g_k6.any.reserve((size_t)slots * ANY_SLOT_WORDS * 4))) return rc;
    const auto any = bounded ? k6_dp_any<true> : k6_dp_any<false>;
    for (unsigned int f = 0; f < nov; f += slots)
        hipLaunchKernelGGL(any, dim3(std::min(slots, nov - f)), dim3(ANY_THREADS), 0, st, groups, jobs, (const unsigned int *)list, f, res,
                           (uint32_t *)g_k6.any.p, O, E, Y, cap, bc, sweep);
    return 0;
}

}  // namespace mimeo
