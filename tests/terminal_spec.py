"""Terminal repeats of a feature (mimeo_terminal_repeats, kernel K17): the rules of include/mimeo_hip.h restated twice, with
no device in sight.

  windows(start, end, length, window)   w and the three origins of an item
  gotoh_loops(a, b, P)                  the recurrence cell by cell in three plain loops; the check of the other one (w <= 64)
  gotoh_sweep(a, b, P)                  the same cells anti-diagonal by anti-diagonal: three rolling score vectors and a uint8
                                        direction matrix (16 MiB and about a second at w = 4096)
  terminal_repeats(seqs, intervals, **params)   (records[2n], first[2n + 1], blocks) as engine.terminal_repeats returns them

a and b are arrays of codes: A0 C1 G2 T3, 4 for every other letter.  Both functions return None where nothing is found, else
(score, [(i, j, len), ...] in increasing order, id_n)."""
import numpy as np

from mimeo_amd import _ffi

DEFAULTS = dict(window=1024, match=2, mismatch=3, gap_open=5, gap_extend=2, min_score=40)
NEG = -(1 << 40)

_CODE = np.full(256, 4, dtype=np.uint8)
for _k, _c in enumerate('ACGT'):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _k


def codes(letters):
    """uint8 letters (or bytes) -> codes; lower case counts as upper case, everything but ACGT is 4"""
    if isinstance(letters, (bytes, bytearray)):
        letters = np.frombuffer(bytes(letters), dtype=np.uint8)
    return _CODE[np.asarray(letters, dtype=np.uint8)]


def revcomp_codes(c):
    r = c[::-1].copy()
    r[r < 4] = 3 - r[r < 4]
    return r


def params(**kw):
    P = dict(DEFAULTS)
    for k, v in kw.items():
        if k not in P:
            raise TypeError('unknown terminal-repeat parameter %r' % k)
        P[k] = int(v)
    return P


def windows(start, end, length, window):
    """(w, head origin on fwd, direct tail origin on fwd, inverted tail origin on rc)"""
    w = min(int(window), (int(end) - int(start)) // 2)
    return w, int(start), int(end) - w, int(length) - int(end)


def _score(x, y, P):
    return P['match'] if x < 4 and y < 4 and x == y else -P['mismatch']


def _walk(D, a, b, bi, bj):
    """The traceback from the best cell over the direction nibbles D[i][j]: bits 0-1 the source of H (0 stop, 1 diagonal,
    2 E, 3 F), bit 2 "E extends", bit 3 "F extends".  Blocks in increasing order, and the matching columns."""
    i, j, state = bi, bj, 'H'
    cols = []
    while True:
        if state == 'H':
            if i < 0 or j < 0:
                break
            src = int(D[i][j]) & 3
            if src == 0:
                break
            if src == 1:
                cols.append((i, j))
                i, j = i - 1, j - 1
            else:
                state = 'E' if src == 2 else 'F'
        elif state == 'E':
            if not int(D[i][j]) & 4:
                state = 'H'
            j -= 1
        else:
            if not int(D[i][j]) & 8:
                state = 'H'
            i -= 1
    cols.reverse()
    blocks = []
    for i, j in cols:
        if blocks and blocks[-1][0] + blocks[-1][2] == i and blocks[-1][1] + blocks[-1][2] == j:
            blocks[-1][2] += 1
        else:
            blocks.append([i, j, 1])
    id_n = sum(1 for i, j in cols if a[i] < 4 and a[i] == b[j])
    return [tuple(x) for x in blocks], id_n


def gotoh_loops(a, b, P):
    w = len(a)
    assert len(b) == w
    go, ge = P['gap_open'], P['gap_extend']
    H = [[0] * w for _ in range(w)]
    E = [[NEG] * w for _ in range(w)]
    F = [[NEG] * w for _ in range(w)]
    D = [[0] * w for _ in range(w)]
    best = (0, 0, 0)
    for i in range(w):
        for j in range(w):
            hl, el = (H[i][j - 1], E[i][j - 1]) if j else (0, NEG)
            hu, fu = (H[i - 1][j], F[i - 1][j]) if i else (0, NEG)
            hd = H[i - 1][j - 1] if i and j else 0
            E[i][j] = max(hl - go - ge, el - ge)
            F[i][j] = max(hu - go - ge, fu - ge)
            d = hd + _score(a[i], b[j], P)
            v = H[i][j] = max(0, d, E[i][j], F[i][j])
            src = 0 if v == 0 else 1 if v == d else 2 if v == E[i][j] else 3
            D[i][j] = src | (4 if E[i][j] != hl - go - ge else 0) | (8 if F[i][j] != hu - go - ge else 0)
            if v > best[0]:   # row-major order: the smallest i, then the smallest j, of the equal ones
                best = (v, i, j)
    if best[0] < P['min_score']:
        return None
    blocks, id_n = _walk(D, a, b, best[1], best[2])
    return best[0], blocks, id_n


def gotoh_sweep(a, b, P):
    w = len(a)
    assert len(b) == w
    if w == 0:
        return None
    a = np.asarray(a, dtype=np.int64)
    b = np.asarray(b, dtype=np.int64)
    go, ge, goe = P['gap_open'], P['gap_extend'], P['gap_open'] + P['gap_extend']
    match, mism = P['match'], -P['mismatch']
    D = np.zeros((w, w), dtype=np.uint8)
    ar = np.arange(w)
    # vectors over i + 1 (entry 0: the row above the matrix); every anti-diagonal starts from the values outside the matrix
    H1 = np.zeros(w + 1, dtype=np.int64)
    H2 = np.zeros(w + 1, dtype=np.int64)
    E1 = np.full(w + 1, NEG, dtype=np.int64)
    F1 = np.full(w + 1, NEG, dtype=np.int64)
    best = (0, 0, 0)
    for d in range(2 * w - 1):
        lo, hi = max(0, d - w + 1), min(d, w - 1)   # rows of the anti-diagonal, j = d - i
        ii = ar[lo:hi + 1]
        jj = d - ii
        x, y = a[ii], b[jj]
        s = np.where((x < 4) & (y < 4) & (x == y), match, mism)
        hl, el = H1[lo + 1:hi + 2], E1[lo + 1:hi + 2]   # (i, j - 1) lies on anti-diagonal d - 1 at row i
        hu, fu = H1[lo:hi + 1], F1[lo:hi + 1]           # (i - 1, j) on d - 1 at row i - 1
        dg = H2[lo:hi + 1] + s                          # (i - 1, j - 1) on d - 2 at row i - 1
        e = np.maximum(hl - goe, el - ge)
        f = np.maximum(hu - goe, fu - ge)
        h = np.maximum(np.maximum(dg, 0), np.maximum(e, f))
        src = np.where(h == 0, 0, np.where(h == dg, 1, np.where(h == e, 2, 3)))
        D[ii, jj] = src | np.where(e != hl - goe, 4, 0) | np.where(f != hu - goe, 8, 0)
        m = int(h.max())
        if m >= best[0] and m > 0:
            k = int(np.argmax(h))   # the first of the equal ones: the smallest i of this anti-diagonal
            if m > best[0] or (lo + k, d - lo - k) < (best[1], best[2]):
                best = (m, lo + k, d - lo - k)
        H0 = np.zeros(w + 1, dtype=np.int64)
        E0 = np.full(w + 1, NEG, dtype=np.int64)
        F0 = np.full(w + 1, NEG, dtype=np.int64)
        H0[lo + 1:hi + 2], E0[lo + 1:hi + 2], F0[lo + 1:hi + 2] = h, e, f
        H2, H1, E1, F1 = H1, H0, E0, F0
    if best[0] < P['min_score']:
        return None
    blocks, id_n = _walk(D, a, b, best[1], best[2])
    return best[0], blocks, id_n


def path_score(a, b, blocks, P):
    """the score of a path recomputed from its blocks alone"""
    s = 0
    for k, (i, j, ln) in enumerate(blocks):
        s += sum(_score(a[i + c], b[j + c], P) for c in range(ln))
        if k:
            pi, pj, pl = blocks[k - 1]
            for gap in (i - pi - pl, j - pj - pl):
                if gap:
                    s -= P['gap_open'] + gap * P['gap_extend']
    return s


def terminal_repeats(seqs, intervals, gotoh=gotoh_sweep, **kw):
    """seqs: the scaffolds as uint8 letters (or bytes); intervals: rows of (chrom, start, end)"""
    P = params(**kw)
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
    fwd, rc = {}, {}
    recs = np.zeros(2 * len(iv), dtype=_ffi.ALIGNMENT)
    first = np.zeros(2 * len(iv) + 1, dtype=np.uint64)
    out = []
    for k, (chrom, start, end) in enumerate(iv.tolist()):
        if chrom not in fwd:
            fwd[chrom] = codes(seqs[chrom])
            rc[chrom] = revcomp_codes(fwd[chrom])
        L = len(fwd[chrom])
        assert 0 <= start <= end <= L
        w, ha, db, ib = windows(start, end, L, P['window'])
        a = fwd[chrom][ha:ha + w]
        for o, (strand, org) in enumerate(((fwd, db), (rc, ib))):
            r = recs[2 * k + o]
            r['tid'] = r['qid'] = chrom
            r['qstrand'] = o
            got = gotoh(a, strand[chrom][org:org + w], P) if w else None
            if got is not None:
                score, blocks, id_n = got
                blk = [(ha + i, org + j, ln) for i, j, ln in blocks]
                out += blk
                r['tstart'], r['tend'] = blk[0][0], blk[-1][0] + blk[-1][2]
                q0, q1 = blk[0][1], blk[-1][1] + blk[-1][2]
                r['qstart'], r['qend'] = (L - q1, L - q0) if o else (q0, q1)
                r['score'], r['id_n'], r['id_d'] = score, id_n, sum(b[2] for b in blk)
            first[2 * k + o + 1] = len(out)
    blocks = np.zeros(len(out), dtype=_ffi.PATH_BLOCK)
    if out:
        arr = np.asarray(out, dtype=np.uint32)
        blocks['t'], blocks['q'], blocks['len'] = arr[:, 0], arr[:, 1], arr[:, 2]
    return recs, first, blocks


def column_stats(seqs, recs, first, blocks):
    """what mimeo_path_stats (K9) counts for these paths, restated: _ffi.COLUMN_STATS rows"""
    out = np.zeros(len(recs), dtype=_ffi.COLUMN_STATS)
    for k, r in enumerate(recs):
        T = codes(seqs[int(r['tid'])])
        Q = revcomp_codes(codes(seqs[int(r['qid'])])) if r['qstrand'] else codes(seqs[int(r['qid'])])
        b = blocks[int(first[k]):int(first[k + 1])].tolist()
        for n, (t, q, ln) in enumerate(b):
            x, y = T[t:t + ln], Q[q:q + ln]
            amb = (x > 3) | (y > 3)
            out[k]['ambiguous'] += int(amb.sum())
            out[k]['matches'] += int((~amb & (x == y)).sum())
            out[k]['transitions'] += int((~amb & ((x ^ y) == 2)).sum())
            out[k]['transversions'] += int((~amb & (x != y) & ((x ^ y) != 2)).sum())
            if n:
                pt, pq, pl = b[n - 1]
                if t - pt - pl:
                    out[k]['del_runs'] += 1
                    out[k]['del_bases'] += t - pt - pl
                if q - pq - pl:
                    out[k]['ins_runs'] += 1
                    out[k]['ins_bases'] += q - pq - pl
    return out
