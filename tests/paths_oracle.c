/*
 * paths_oracle.c — the paths of the alignments of one `lastz T Q` run under the box rule (the default) or the path rule:
 * what mimeo_align_units_paths is checked against.
 *
 * TEST INFRASTRUCTURE ONLY (see the header of oracle/mimeo_oracle.c).  PARITY UNPINNED, as everything on top of
 * oracle/box_vs_path.c.
 *
 * This is the anchor loop of align_pair_strand_rule (oracle/box_vs_path.c) with both halves run by half_extend_tb, so that
 * every extended alignment leaves its diagonal (match / mismatch) steps behind.  Nothing else is restated: HSPs, chain,
 * anchor order, the skip tests and the threshold are the calls and the lines of that function.  The records must equal
 * orc_align_pair's under the box rule; under the path rule the dump must equal the one of tests/bounded_oracle.c run
 * unbounded (tests/test_host_paths.py holds it to both).
 */
#include "../oracle/box_vs_path.c"

/* the extended alignments of a run, above the threshold or not: path keys (t << 32 | q, strand coordinates) one alignment
 * after the other, and per alignment { minus, at, aq, first key, key count, score } — the layout of bounded_oracle.c */
typedef struct { uint64_t *key, nkey, capkey; uint64_t *meta, nmeta, capmeta; } pathdump;
static void dump_push(pathdump *d, int minus, uint64_t at, uint64_t aq, int64_t score, const pathset *mine) {
    if (d->nkey + mine->n > d->capkey) { d->capkey = (d->nkey + mine->n) * 2 + 1024; d->key = (uint64_t *)realloc(d->key, d->capkey * 8); }
    if (mine->n) memcpy(d->key + d->nkey, mine->key, mine->n * 8);
    if (d->nmeta + 6 > d->capmeta) { d->capmeta = d->capmeta ? d->capmeta * 2 : 1024; d->meta = (uint64_t *)realloc(d->meta, d->capmeta * 8); }
    uint64_t *m = d->meta + d->nmeta;
    m[0] = (uint64_t)minus; m[1] = at; m[2] = aq; m[3] = d->nkey; m[4] = mine->n; m[5] = (uint64_t)score;
    d->nmeta += 6;
    d->nkey += mine->n;
}

static int align_pair_strand_paths(const uint8_t *T, const uint8_t *Tlow, uint64_t Lt, const uint8_t *Q, uint64_t Lq, int minus,
                                   const orc_params *p, int path_rule, alnvec *out, pathdump *dump) {
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
    pathset all = {0, 0, 0};   /* diagonal steps of every alignment so far, kept sorted (path rule) */
    for (uint64_t k = 0; k < hsps.n; k++) {
        orc_hsp *h = &hsps.v[k];
        orc_aln a;
        memset(&a, 0, sizeof a);
        a.qstrand = (uint32_t)minus;
        const uint32_t off = anchor_offset(T, Q, h);
        const uint64_t at = (uint64_t)h->tstart + off, aq = (uint64_t)h->qstart + off;
        int inbox = 0, onpath = 0;
        for (uint64_t e = first_out; e < out->n && !inbox; e++) {
            orc_aln *o = &out->v[e];
            if (at >= o->tstart && at < o->tend && aq >= o->qstart && aq < o->qend) inbox = 1;
        }
        if (all.n) { const uint64_t key = (at << 32) | aq; onpath = bsearch(&key, all.key, all.n, 8, cmp_u64) != NULL; }
        if (path_rule ? onpath : inbox) continue;
        pathset mine = {0, 0, 0};
        half_result L = half_extend_tb(T, Lt, Q, Lq, at, aq, -1, p, &mine);
        half_result R = half_extend_tb(T, Lt, Q, Lq, at, aq, +1, p, &mine);
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
    }
    out->n = m;
    free(all.key);
    free(hsps.v);
    return 0;
}

/* one `lastz T Q` run under the box rule (path_rule = 0) or the path rule (1), strands as in p->strand: the records, and
 * the dump described at pathdump (keys, meta: released with orc_free) */
int orc_align_pair_paths(const uint8_t *Ta, uint64_t Lt, const uint8_t *Qa, uint64_t Lq, const orc_params *p, int path_rule,
                         orc_aln **out, uint64_t *nout, uint64_t **keys, uint64_t *nkeys, uint64_t **meta, uint64_t *nmeta) {
    alnvec av = {0, 0, 0};
    pathdump dump = {0, 0, 0, 0, 0, 0};
    int rc = 0;
    for (int minus = 0; minus < 2 && !rc; minus++) {
        if (!(p->strand & (minus ? 2 : 1))) continue;
        uint8_t *T, *Tlow, *Q;
        if (prep(Ta, Lt, Qa, Lq, minus, &T, &Tlow, &Q)) return -1;
        rc = align_pair_strand_paths(T, Tlow, Lt, Q, Lq, minus, p, path_rule, &av, &dump);
        free(T); free(Tlow); free(Q);
    }
    *out = av.v; *nout = av.n;
    *keys = dump.key; *nkeys = dump.nkey; *meta = dump.meta; *nmeta = dump.nmeta / 6;
    return rc;
}
