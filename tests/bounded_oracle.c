/*
 * bounded_oracle.c — the SPECIFICATION of mimeo_params.bound_extensions (alignment specification v1, rule 7, last clause).
 *
 * TEST INFRASTRUCTURE ONLY (see the header of oracle/mimeo_oracle.c).  PARITY UNPINNED: this is the project's own rule,
 * modelled on lastz's documented behaviour (a new gapped extension is bounded by the earlier alignments left and right of
 * its anchor), not a statement about what lastz computes.
 *
 * Fixed context: one (pair, strand), anchors in rank order, path rule in force.  P = the diagonal (match / mismatch) steps
 * (t, q) of every earlier EXTENDED alignment of the (pair, strand), above the threshold or not — the set the path rule tests
 * anchors against.  For a target base t: S(t) = { q - t : (t, q) in P }.  For an anchor (at, aq): d0 = aq - at,
 *   dL(t) = max { d in S(t) : d <= d0 }  (none: -inf),   dR(t) = min { d in S(t) : d >= d0 }  (none: +inf).
 * In a half extension row i >= 1 consumes t_i = at + i - 1 (dir +) or at - i (dir -), column j stands at query base
 * q_j = aq + j - 1 (dir +) or aq - j (dir -), also for j = 0.  Cell (i, j), i >= 1, is DEAD in all three states unless
 *   dL(t_i) < q_j - t_i < dR(t_i):
 * its C and D are -inf, its H feeds no insertion, it is never a best cell.  Row 0 is not clipped.  Recurrences,
 * tie-breaks, y-drop pruning against the best of earlier rows, the first-best-cell rule and the walk-back are those of
 * half_extend_tb (oracle/box_vs_path.c), which the function below restates with that one clause added.
 */
#include "../oracle/box_vs_path.c"

/* dL / dR of row t for the anchor diagonal d0 from the sorted keys t << 32 | q */
static void row_bounds(const pathset *all, uint64_t t, int64_t d0, int64_t *dL, int64_t *dR) {
    *dL = INT64_MIN; *dR = INT64_MAX;
    if (!all || !all->n) return;
    uint64_t lo = 0, hi = all->n;   /* first key >= t << 32 */
    const uint64_t k0 = t << 32;
    while (lo < hi) { const uint64_t mid = (lo + hi) >> 1; if (all->key[mid] < k0) lo = mid + 1; else hi = mid; }
    for (; lo < all->n && (all->key[lo] >> 32) == t; lo++) {
        const int64_t d = (int64_t)(all->key[lo] & 0xFFFFFFFFu) - (int64_t)t;
        if (d <= d0 && d > *dL) *dL = d;
        if (d >= d0 && d < *dR) *dR = d;
    }
}

/* half_extend_tb of box_vs_path.c with the clip; `all` == NULL: no clip (then it IS half_extend_tb) */
static half_result half_extend_bounded(const uint8_t *T, uint64_t Lt, const uint8_t *Q, uint64_t Lq, uint64_t at, uint64_t aq,
                                       int dir, const orc_params *p, const pathset *all, pathset *path, uint64_t *clipped) {
    const int64_t O = p->gap_open, E = p->gap_extend, Y = p->ydrop;
    const int64_t d0 = (int64_t)aq - (int64_t)at;
    uint64_t lenA = dir > 0 ? Lt - at : at, lenB = dir > 0 ? Lq - aq : aq;
    half_result best = {0, 0, 0, 0, 0};
    uint64_t cap = 1024;
    cell *C0 = (cell *)malloc(cap * sizeof(cell)), *D0 = (cell *)malloc(cap * sizeof(cell));
    cell *C1 = (cell *)malloc(cap * sizeof(cell)), *D1 = (cell *)malloc(cap * sizeof(cell));
    tbstore S = {0, 0, 0, 0, 0, 0, 0};
    uint64_t lo = 0, hi = 0;
    C0[0].s = 0; C0[0].nm = C0[0].nx = 0; D0[0].s = NEG; D0[0].nm = D0[0].nx = 0;
    tb_row(&S, 0, 0);
    tb_push(&S, 0);
    for (uint64_t j = 1; j <= lenB; j++) {
        int64_t v = -O - (int64_t)j * E;
        if (v < -Y) break;
        if (j >= cap) { cap *= 2; C0 = realloc(C0, cap * sizeof(cell)); D0 = realloc(D0, cap * sizeof(cell));
                        C1 = realloc(C1, cap * sizeof(cell)); D1 = realloc(D1, cap * sizeof(cell)); }
        C0[j].s = v; C0[j].nm = C0[j].nx = 0; D0[j].s = NEG; D0[j].nm = D0[j].nx = 0;
        tb_push(&S, TB_CI);
        hi = j;
    }
    uint64_t plo = lo, phi = hi;
    for (uint64_t i = 1; i <= lenA; i++) {
        int64_t thr = best.score - Y;
        const uint64_t t = dir > 0 ? at + i - 1 : at - i;
        uint8_t a = T[t];
        int64_t dL, dR;
        row_bounds(all, t, d0, &dL, &dR);
        uint64_t jlo = plo, jmax = phi + 1;
        if (jmax > lenB) jmax = lenB;
        cell Icell = {NEG, 0, 0};
        int iopen = 0;
        uint64_t first = UINT64_MAX, last = 0;
        int64_t rowbest = NEG; uint64_t rowbestj = 0; cell rowbestc = {NEG, 0, 0};
        uint64_t j = jlo;
        tb_row(&S, i, jlo);
        for (;; j++) {
            if (j > lenB) break;
            uint64_t idx = j - jlo;
            if (idx + 2 >= cap) { cap *= 2; C0 = realloc(C0, cap * sizeof(cell)); D0 = realloc(D0, cap * sizeof(cell));
                                  C1 = realloc(C1, cap * sizeof(cell)); D1 = realloc(D1, cap * sizeof(cell)); }
            /* the clause: q_j - t_i must lie strictly between dL and dR */
            const int64_t dq = (dir > 0 ? (int64_t)aq + (int64_t)j - 1 : (int64_t)aq - (int64_t)j) - (int64_t)t;
            const int allowed = dq > dL && dq < dR;
            cell d = {NEG, 0, 0}, g = {NEG, 0, 0};
            uint8_t tb = iopen ? TB_IOPEN : 0;
            if (j >= plo && j <= phi) {
                cell pc = C0[j - plo], pd = D0[j - plo];
                if (pd.s > NEG) { d = pd; d.s -= E; }
                if (pc.s > NEG && pc.s - O - E > d.s) { d = pc; d.s = pc.s - O - E; tb |= TB_DOPEN; }
            }
            if (j >= 1 && j - 1 >= plo && j - 1 <= phi && C0[j - 1 - plo].s > NEG) {
                uint8_t b = dir > 0 ? Q[aq + j - 1] : Q[aq - j];
                g = C0[j - 1 - plo];
                g.s += SUB[a][b];
                if (a < 4 && a == b) g.nm++; else g.nx++;
            }
            cell h = g;
            if (d.s > h.s) { h = d; tb |= TB_HD; }
            cell c = h;
            if (Icell.s > c.s) { c = Icell; tb |= TB_CI; }
            if (!allowed) {   /* dead in all three states: C = D = -inf, H feeds no insertion, never a best cell */
                if (c.s >= thr && c.s > NEG / 2) (*clipped)++;   /* a cell the same row would have kept without the clause */
                h.s = NEG;
            }
            if (!allowed || c.s < thr || c.s <= NEG / 2) { c.s = NEG; d.s = NEG; }
            else {
                if (first == UINT64_MAX) first = j;
                last = j;
                if (c.s > rowbest) { rowbest = c.s; rowbestj = j; rowbestc = c; }
            }
            C1[idx] = c; D1[idx] = d;
            tb_push(&S, tb);
            cell ni = {NEG, 0, 0};
            iopen = 0;
            if (Icell.s > NEG) { ni = Icell; ni.s -= E; }
            if (h.s > NEG / 2 && h.s - O - E > ni.s) { ni = h; ni.s = h.s - O - E; iopen = 1; }   /* a dead cell's H is NEG */
            Icell = ni;
            if (j >= jmax && Icell.s < thr) { j++; break; }
        }
        if (first == UINT64_MAX) break;
        if (rowbest > best.score) { best.score = rowbest; best.i = i; best.j = rowbestj; best.nm = rowbestc.nm; best.nx = rowbestc.nx; }
        uint64_t w = last - first + 1;
        memmove(C1, C1 + (first - jlo), w * sizeof(cell));
        memmove(D1, D1 + (first - jlo), w * sizeof(cell));
        cell *tc = C0; C0 = C1; C1 = tc;
        cell *td = D0; D0 = D1; D1 = td;
        plo = first; phi = last;
    }
    {   /* the walk-back of half_extend_tb */
        uint64_t i = best.i, j = best.j;
        int st = 0;
        uint32_t nm = 0, nx = 0;
        while (i || j) {
            if (i == 0) { j--; continue; }
            const uint8_t tb = tb_get(&S, i, j);
            if (st == 0) st = (tb & TB_CI) ? 3 : 1;
            else if (st == 1) {
                if (tb & TB_HD) st = 2;
                else {
                    const uint64_t t = dir > 0 ? at + i - 1 : at - i, q = dir > 0 ? aq + j - 1 : aq - j;
                    if (path->n == path->cap) { path->cap = path->cap ? path->cap * 2 : 4096; path->key = (uint64_t *)realloc(path->key, path->cap * 8); }
                    path->key[path->n++] = (t << 32) | q;
                    if (T[t] < 4 && T[t] == Q[q]) nm++; else nx++;
                    i--; j--; st = 0;
                }
            } else if (st == 2) { st = (tb & TB_DOPEN) ? 0 : 2; i--; }
            else { st = (tb & TB_IOPEN) ? 1 : 3; j--; }
        }
        if (nm != best.nm || nx != best.nx) { fprintf(stderr, "bounded_oracle: traceback disagrees with the carried counts (%u/%u vs %u/%u)\n", nm, nx, best.nm, best.nx); abort(); }
    }
    free(S.tb); free(S.row_off); free(S.row_lo);
    free(C0); free(D0); free(C1); free(D1);
    return best;
}

/* the extended alignments of a run, for the invariant test: path keys (t << 32 | q, strand coordinates) one alignment
 * after the other, and per alignment { minus, at, aq, first key, key count, score } */
typedef struct { uint64_t *key, nkey, capkey; uint64_t *meta, nmeta, capmeta; } pathdump;
static void dump_push(pathdump *d, int minus, uint64_t at, uint64_t aq, int64_t score, const pathset *mine) {
    if (!d) return;
    if (d->nkey + mine->n > d->capkey) { d->capkey = (d->nkey + mine->n) * 2 + 1024; d->key = (uint64_t *)realloc(d->key, d->capkey * 8); }
    if (mine->n) memcpy(d->key + d->nkey, mine->key, mine->n * 8);
    if (d->nmeta + 6 > d->capmeta) { d->capmeta = d->capmeta ? d->capmeta * 2 : 1024; d->meta = (uint64_t *)realloc(d->meta, d->capmeta * 8); }
    uint64_t *m = d->meta + d->nmeta;
    m[0] = (uint64_t)minus; m[1] = at; m[2] = aq; m[3] = d->nkey; m[4] = mine->n; m[5] = (uint64_t)score;
    d->nmeta += 6;
    d->nkey += mine->n;
}

/* the anchor loop of align_pair_strand_rule (path rule), each extension bounded when `bounded`.
 * counts[0] anchors, [1] skipped (on an earlier path), [2] alignments kept, [3] live cells clipped */
static int align_pair_strand_bounded(const uint8_t *T, const uint8_t *Tlow, uint64_t Lt, const uint8_t *Q, uint64_t Lq, int minus,
                                     const orc_params *p, int bounded, alnvec *out, uint64_t *counts, pathdump *dump) {
    hspvec hsps = {0, 0, 0};
    if (scan_pair_strand(T, Tlow, Lt, Q, Lq, p, NULL, &hsps)) return -1;
    if (p->chain) {
        if (chain_hsps(hsps.v, hsps.n)) return -1;
        uint64_t m = 0;
        for (uint64_t i = 0; i < hsps.n; i++) if (hsps.v[i].flags & 1u) hsps.v[m++] = hsps.v[i];
        hsps.n = m;
    }
    if (hsps.n) qsort(hsps.v, hsps.n, sizeof(orc_hsp), cmp_hsp_score_desc);
    const uint64_t first_out = out->n;
    pathset all = {0, 0, 0};   /* P, kept sorted */
    for (uint64_t k = 0; k < hsps.n; k++) {
        orc_hsp *h = &hsps.v[k];
        orc_aln a;
        memset(&a, 0, sizeof a);
        a.qstrand = (uint32_t)minus;
        const uint32_t off = anchor_offset(T, Q, h);
        const uint64_t at = (uint64_t)h->tstart + off, aq = (uint64_t)h->qstart + off;
        counts[0]++;
        if (all.n) { const uint64_t key = (at << 32) | aq; if (bsearch(&key, all.key, all.n, 8, cmp_u64) != NULL) { counts[1]++; continue; } }
        pathset mine = {0, 0, 0};
        half_result L = half_extend_bounded(T, Lt, Q, Lq, at, aq, -1, p, bounded ? &all : NULL, &mine, &counts[3]);
        half_result R = half_extend_bounded(T, Lt, Q, Lq, at, aq, +1, p, bounded ? &all : NULL, &mine, &counts[3]);
        a.tstart = (uint32_t)(at - L.i); a.tend = (uint32_t)(at + R.i);
        a.qstart = (uint32_t)(aq - L.j); a.qend = (uint32_t)(aq + R.j);
        a.score = L.score + R.score;
        a.id_n = L.nm + R.nm;
        a.id_d = L.nm + R.nm + L.nx + R.nx;
        VPUSH(*out, orc_aln, a);
        dump_push(dump, minus, at, aq, a.score, &mine);
        if (mine.n) {
            if (all.n + mine.n > all.cap) { all.cap = (all.n + mine.n) * 2; all.key = (uint64_t *)realloc(all.key, all.cap * 8); }
            memcpy(all.key + all.n, mine.key, mine.n * 8);
            all.n += mine.n;
            qsort(all.key, all.n, 8, cmp_u64);
        }
        free(mine.key);
    }
    uint64_t m = first_out;
    for (uint64_t e = first_out; e < out->n; e++) {
        orc_aln a = out->v[e];
        if (a.score < p->hspthresh) continue;
        if (minus) { uint32_t s = (uint32_t)(Lq - a.qend), t2 = (uint32_t)(Lq - a.qstart); a.qstart = s; a.qend = t2; }
        out->v[m++] = a;
        counts[2]++;
    }
    out->n = m;
    free(all.key);
    free(hsps.v);
    return 0;
}

/* one `lastz T Q` run under the path rule, bounded (1) or not (0: must reproduce orc_align_pair_rule(..., 1)); strands as
 * in p->strand.  keys / meta (either may be NULL): the path dump described at pathdump, released with orc_free. */
int orc_align_pair_bounded(const uint8_t *Ta, uint64_t Lt, const uint8_t *Qa, uint64_t Lq, const orc_params *p, int bounded,
                           orc_aln **out, uint64_t *nout, uint64_t *counts, uint64_t **keys, uint64_t *nkeys, uint64_t **meta,
                           uint64_t *nmeta) {
    alnvec av = {0, 0, 0};
    pathdump dump = {0, 0, 0, 0, 0, 0};
    int rc = 0;
    for (int k = 0; k < 4; k++) counts[k] = 0;
    for (int minus = 0; minus < 2 && !rc; minus++) {
        if (!(p->strand & (minus ? 2 : 1))) continue;
        uint8_t *T, *Tlow, *Q;
        if (prep(Ta, Lt, Qa, Lq, minus, &T, &Tlow, &Q)) return -1;
        rc = align_pair_strand_bounded(T, Tlow, Lt, Q, Lq, minus, p, bounded, &av, counts, keys && meta ? &dump : NULL);
        free(T); free(Tlow); free(Q);
    }
    *out = av.v; *nout = av.n;
    if (keys && meta) { *keys = dump.key; *nkeys = dump.nkey; *meta = dump.meta; *nmeta = dump.nmeta / 6; }
    return rc;
}
