"""Element structure (mimeo_flank_repeats, kernel K18; mimeo_open_frames, kernel K19): the rules of include/mimeo_hip.h
restated twice each, with no device in sight, and the pipeline of `mimeo self --elements` restated over them.

  flank_loops(c, start, end, P)    every candidate (dl, dr, k) in three plain loops, columns compared one by one
  flank_numpy(c, start, end, P)    all candidates at once: one (candidates, max_len) table of column comparisons
  frames_loops(c, rc, start, end)  codon by codon
  frames_numpy(c, rc, start, end)  one closed-codon vector per frame, runs from its differences
  flank_repeats(seqs, intervals, impl, **params), open_frames(seqs, intervals, impl)   as the engine returns them
  element_rows(seqs, iv, ...)      steps 1 - 5 of workflow.elements_block with tests/terminal_spec.py for K17 and K9

c and rc are arrays of codes (tests/terminal_spec.py: A0 C1 G2 T3, 4 for every other letter) of a scaffold's forward strand and
of its reverse complement."""
import numpy as np

from mimeo_amd import _ffi
from tests import terminal_spec as T

FLANK_DEFAULTS = dict(min_len=4, max_len=20, slack=2, max_mismatch=0)
STOPS = ((3, 0, 0), (3, 0, 2), (3, 2, 0))   # TAA TAG TGA


def flank_params(**kw):
    P = dict(FLANK_DEFAULTS)
    for k, v in kw.items():
        if k not in P:
            raise TypeError('unknown flank-repeat parameter %r' % k)
        P[k] = int(v)
    return P


def flank_loops(c, start, end, P):
    """(left_start, right_start, len, mismatches, dl, dr) or None"""
    L, best = len(c), None
    for dl in range(-P['slack'], P['slack'] + 1):
        for dr in range(-P['slack'], P['slack'] + 1):
            for k in range(P['min_len'], P['max_len'] + 1):
                p, r = start + dl - k, end + dr
                if p < 0 or r + k > L or start + dl > end + dr:
                    continue
                bad = [not (c[p + x] < 4 and c[p + x] == c[r + x]) for x in range(k)]
                m = sum(bad)
                if m > P['max_mismatch'] or bad[0] or bad[-1] or k - 3 * m < P['min_len']:
                    continue
                order = (-(k - 3 * m), abs(dl) + abs(dr), m, dl, dr)
                if best is None or order < best[0]:
                    best = (order, (p, r, k, m, dl, dr))
    return None if best is None else best[1]


def flank_numpy(c, start, end, P):
    s, lo, hi = P['slack'], P['min_len'], P['max_len']
    pad = hi + s + 1
    x = np.concatenate([np.full(pad, 5, np.int64), np.asarray(c, dtype=np.int64), np.full(pad, 6, np.int64)])   # no pad letter equals another
    d = np.arange(-s, s + 1)
    dl, dr, k = [a.ravel() for a in np.meshgrid(d, d, np.arange(lo, hi + 1), indexing='ij')]
    p, r = start + dl - k, end + dr
    col = np.arange(hi)[None, :]
    inside = col < k[:, None]
    at = lambda q: x[np.clip(q[:, None] + col, -pad, len(c) + pad - 1) + pad]
    a, b = at(p), at(r)
    bad = ~((a < 4) & (a == b)) & inside
    m = bad.sum(axis=1)
    last = bad[np.arange(k.size), k - 1]
    v = k - 3 * m
    ok = (p >= 0) & (r + k <= len(c)) & (start + dl <= end + dr) & (m <= P['max_mismatch']) & ~bad[:, 0] & ~last & (v >= lo)
    if not ok.any():
        return None
    rows = np.flatnonzero(ok)
    best = rows[np.lexsort((dr[rows], dl[rows], m[rows], np.abs(dl[rows]) + np.abs(dr[rows]), -v[rows]))[0]]
    return int(p[best]), int(r[best]), int(k[best]), int(m[best]), int(dl[best]), int(dr[best])


def _scaffolds(seqs):
    fwd = [T.codes(s) for s in seqs]
    return fwd, [T.revcomp_codes(c) for c in fwd]


def flank_repeats(seqs, intervals, impl=flank_numpy, **kw):
    P = flank_params(**kw)
    fwd, _ = _scaffolds(seqs)
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
    out = np.zeros(len(iv), dtype=_ffi.FLANK_REPEAT)
    for i, (chrom, start, end) in enumerate(iv.tolist()):
        assert 0 <= start <= end <= len(fwd[chrom])
        got = impl(fwd[chrom], start, end, P)
        if got is not None:
            out[i] = got + (0,)
    return out


def _closed(x, y, z):
    return x > 3 or y > 3 or z > 3 or (x, y, z) in STOPS


def frames_loops(c, rc, start, end):
    """six (start, end, codons, met)"""
    L, m, out = len(c), end - start, []
    for sigma in (0, 1):
        s = c[start:end] if sigma == 0 else rc[L - end:L - start]
        for phi in range(3):
            n = max(0, (m - phi) // 3)
            best, t, run0 = (0, 0), 0, None
            for t in range(n + 1):
                closed = t == n or _closed(int(s[phi + 3 * t]), int(s[phi + 3 * t + 1]), int(s[phi + 3 * t + 2]))
                if not closed and run0 is None:
                    run0 = t
                if closed and run0 is not None:
                    if t - run0 > best[0]:
                        best = (t - run0, run0)
                    run0 = None
            cod, t0 = best
            if not cod:
                out.append((0, 0, 0, 0))
                continue
            met = cod
            for u in range(cod):
                if tuple(int(v) for v in s[phi + 3 * (t0 + u):phi + 3 * (t0 + u) + 3]) == (0, 3, 2):
                    met = u
                    break
            a, b = phi + 3 * t0, phi + 3 * (t0 + cod)
            out.append((start + a, start + b, cod, met) if sigma == 0 else (end - b, end - a, cod, met))
    return out


def frames_numpy(c, rc, start, end):
    L, m, out = len(c), end - start, []
    for sigma in (0, 1):
        s = np.asarray(c[start:end] if sigma == 0 else rc[L - end:L - start], dtype=np.int64)
        for phi in range(3):
            n = max(0, (m - phi) // 3)
            cod = s[phi:phi + 3 * n].reshape(n, 3)
            x, y, z = cod[:, 0], cod[:, 1], cod[:, 2]
            stop = (x == 3) & (((y == 0) & ((z == 0) | (z == 2))) | ((y == 2) & (z == 0)))
            opened = ~(stop | (cod > 3).any(axis=1))
            edge = np.diff(np.concatenate([[0], opened.astype(np.int8), [0]]))
            t0s, t1s = np.flatnonzero(edge == 1), np.flatnonzero(edge == -1)
            if t0s.size == 0:
                out.append((0, 0, 0, 0))
                continue
            i = int(np.argmax(t1s - t0s))   # the first of the longest
            t0, t1 = int(t0s[i]), int(t1s[i])
            atg = np.flatnonzero((x[t0:t1] == 0) & (y[t0:t1] == 3) & (z[t0:t1] == 2))
            met = int(atg[0]) if atg.size else t1 - t0
            a, b = phi + 3 * t0, phi + 3 * t1
            out.append((start + a, start + b, t1 - t0, met) if sigma == 0 else (end - b, end - a, t1 - t0, met))
    return out


def open_frames(seqs, intervals, impl=frames_numpy):
    fwd, rc = _scaffolds(seqs)
    iv = np.asarray(intervals, dtype=np.int64).reshape(-1, 3)
    out = np.zeros((len(iv), 6), dtype=_ffi.OPEN_FRAME)
    for i, (chrom, start, end) in enumerate(iv.tolist()):
        assert 0 <= start <= end <= len(fwd[chrom])
        for f, rec in enumerate(impl(fwd[chrom], rc[chrom], start, end)):
            out[i, f] = rec
    return out


# ---- the pipeline of --elements ---------------------------------------------------------------------------------------------------

def letters_of(seqs, chrom, a, b):
    """A C G T N of the plus strand, as the device keeps it"""
    return ''.join('ACGTN'[k] for k in T.codes(seqs[chrom][a:b]))


def element_rows(seqs, iv, window=1024, min_score=40, **flank_kw):
    """Steps 1 - 5 for the intervals (chrom, start, end) of the scaffolds `seqs`: per feature a dict with the values that a line
    of the file shows, as formats.element_lines takes them."""
    iv = [tuple(int(v) for v in r) for r in iv]
    recs, first, blocks = T.terminal_repeats(seqs, iv, window=window, min_score=min_score)
    stats = T.column_stats(seqs, recs, first, blocks)
    rows = []
    for k, (chrom, start, end) in enumerate(iv):
        cands = []
        for o in (0, 1):
            a = recs[2 * k + o]
            if int(a['id_d']) == 0:
                continue
            span = (int(a['tstart']), int(a['qend']))
            fl = flank_repeats(seqs, [(chrom,) + span], **flank_kw)[0]
            cands.append((o, span, fl, int(a['score'])))
        with_tsd = [x for x in cands if int(x[2]['len'])]
        pool = with_tsd if len(with_tsd) == 1 else cands   # both or neither: the higher score, then LTR
        pick = min(pool, key=lambda x: (-x[3], x[0])) if pool else None
        row = dict(kind=None, tsd=None)
        if pick is None:
            el = (start, end)
        else:
            o, span, fl, _ = pick
            a, s = recs[2 * k + o], stats[2 * k + o]
            el = (span[0] + int(fl['dl']), span[1] + int(fl['dr']))
            row.update(kind=('LTR', 'TIR')[o], left_len=int(a['tend']) - int(a['tstart']), right_len=int(a['qend']) - int(a['qstart']), score=int(a['score']),
                       stats=s)
            if int(fl['len']):
                p = int(fl['left_start'])
                row['tsd'] = (int(fl['len']), letters_of(seqs, chrom, p, p + int(fl['len'])), int(fl['mismatches']), int(fl['dl']), int(fl['dr']))
        row['el'] = el
        row['ends'] = letters_of(seqs, chrom, el[0], min(el[0] + 2, el[1])) + '..' + letters_of(seqs, chrom, max(el[1] - 2, el[0]), el[1]) if el[1] > el[0] else None
        fr = open_frames(seqs, [(chrom,) + el])[0]
        f = min(range(6), key=lambda j: (-int(fr[j]['codons']), j))
        row['orf'] = (f // 3, f % 3, int(fr[f]['start']), int(fr[f]['end']), int(fr[f]['codons']), int(fr[f]['met'])) if int(fr[f]['codons']) else None
        rows.append(row)
    return rows
