"""Designed pairs for the two strip widths of k6_dp1 (mimeo_amd/csrc/k6_dp.hip) and a prediction of what the kernel makes of a half.

TEST INFRASTRUCTURE, beside tests/k6_cases.py, whose Case, walk and pair builders it uses.  k6_dp1 starts a half extension at W1 = 7
columns per lane (a 448-column window).  When a row ends with the last strip but one live, the wavefront lays its state out at 14
columns per lane (896 columns) and goes on with the next row; when the band outgrows the narrow window in row 0, or in one row from
further down, the wavefront runs the half again from row 1 at 14.  Only a half that outgrows 896 columns goes on to the 2048-column
kernel.  Which half does what, and in which row, is a condition on the inputs, so every case here is ONE pair whose two halves are
known and that says which event it was built for: tests/test_host_k6_strips.py proves that the cases reach their events,
tests/test_gpu_k6_strips.py holds the engine to the oracle and to `predict` on them.

`strip_pass` restates the row loop of lean_dp for a strip width ws, from the kernel's text: the window of row i starts at the strip
(of ws columns) that holds the first live column of row i - 1; the pass gives up in row 0 iff hi_0 >= 63 ws, in row i iff
hi_i // ws - lo_{i-1} // ws >= 63, and on entering row 65 535; at 2 ws = 14 it hands over after the first row with
hi_i // ws - lo_{i-1} // ws == 62.  The window that the state moves to starts at a multiple of 14, so from there on the pass is the
pass at 14 that k6_cases.route describes, and so is its answer: `predict` is route plus what happened on the way.  A half reports
the band of the 14-column layout whichever width computed its rows: maxcols = 14 (max_i (hi_i // 14 - lo_{i-1} // 14) + 1).

The y-drops, gap extensions and distances below were found with k6_cases.walk_c on grids of those values (steps of 50 in the y-drop at
gap extension 30, of 5 at gap extension 5)."""
import numpy as np

from tests import k6_cases as K

W1, FULL = 7, 14          # L_W1, L_WS of k6_dp.hip
RESTARTS = ('row0', 'band')


def _rows(w, ws, first, last):
    """of rows first .. last in windows of 64 strips of ws columns: rows whose window reaches / does not reach beyond the query's
    end, and whether a strip that came in on the right held a live cell"""
    if last < first:
        return dict(edge=0, plain=0, fresh=False)
    touches = ws * (w.lo[first - 1:last] // ws) + 64 * ws - 1 > w.lenB
    return dict(edge=int(touches.sum()), plain=int((~touches).sum()), fresh=bool(w.hi[first:last + 1].max() >= 64 * ws))


def strip_pass(w, ws, row_limit=K.ROW_LIMIT):
    """the row loop of the lean kernel at ws columns per lane on the walk w, from row 0.  dict: event = None when the pass finishes the
    half, else (reason, row) with reason 'row0' / 'band' / 'rows' / 'widen'; before, at: the last live strip of the row before the
    event and of its row; slid: the row before a 'widen' moved the window; widest: the largest last live strip of a finished pass
    (the window holds strips 0 .. 63, and strip 63 must stay dead); maxcols: the 14-column figure of a finished pass; edge, plain,
    fresh (_rows) of the rows the pass computed"""
    lo, hi, R = w.lo, w.hi, w.rows
    out = dict(event=None, before=None, at=None, slid=False, widest=0, maxcols=0, edge=0, plain=0, fresh=False)
    if hi[0] >= 63 * ws:
        out.update(event=('row0', 0), at=int(hi[0]) // ws)
        return out
    rl = hi[1:] // ws - lo[:-1] // ws
    events = []                                                 # (row, order within the row, reason)
    if row_limit and R >= row_limit - 1 and w.lenA >= row_limit:
        events.append((row_limit, 0, 'rows'))                   # tested before the row is computed
    over = np.flatnonzero(rl >= 63)
    if over.size:
        events.append((int(over[0]) + 1, 1, 'band'))
    last = np.flatnonzero(rl == 62) if 2 * ws == FULL else over[:0]
    if last.size:
        events.append((int(last[0]) + 1, 2, 'widen'))            # after the row, which is complete
    if events:
        row, _, why = min(events)
        out.update(event=(why, row))
        if why != 'rows':
            out.update(before=int(rl[row - 2]) if row > 1 else None, at=int(rl[row - 1]))
        if why == 'widen':
            out.update(slid=bool(row > 1 and lo[row - 1] // ws != lo[row - 2] // ws), **_rows(w, ws, 1, row))
        return out
    if R:
        out.update(widest=int(rl.max()), maxcols=int(FULL * ((hi[1:] // FULL - lo[:-1] // FULL).max() + 1)), **_rows(w, ws, 1, R))
    return out


def predict(w, O=400, E=30, Y=9400, cap=K.CAP, shortcut=False, w1=W1):
    """k6_cases.route(w, ...) and, for a half that reaches k6_dp1: first = strip_pass(w, w1); restarted = the wavefront ran the half
    again at 14 columns per lane; widened = it went on at 14 (after row first['event'][1]).  w1 = 14: one pass, neither happens"""
    r = K.route(w, O, E, Y, cap, shortcut=shortcut)
    r.update(first=None, restarted=False, widened=False)
    lean_ok = E <= (1 << 16) and O <= (1 << 24) and Y <= (1 << 28)
    if shortcut or not lean_ok or w1 == FULL:
        return r
    r['first'] = first = strip_pass(w, w1)
    if first['event'] is None:
        # what fits 64 strips of w1 < 14 columns fits 64 strips of 14: the pass at 14 would have finished it with the same figures
        assert r['kernel'] == 'lean' and r['maxcols'] == first['maxcols'], (r, first)
    else:
        r['restarted'] = first['event'][0] in RESTARTS
        r['widened'] = first['event'][0] == 'widen'
    return r


class StripCase:
    """case: a k6_cases.Case; want: per half (left, right) None or a dict of what the half was built for — event: 'fit' / 'widen' /
    'jump' / 'row0' ('jump': the last strip reached from the last but two or below in one row, or in row 1), widest: the last live strip of a
    pass that fits, slid: the widening follows a slide, kernel: the kernel that finishes the half; edge / plain / fresh: True when
    the rows at W1 must hold such rows, edge2 / plain2 / fresh2: the rows at 14 (after a widening or a restart)"""

    def __init__(self, case, left=None, right=None):
        self.case, self.want = case, (left, right)
        self.name = case.name

    def analyse(self):
        """((walk, prediction), (walk, prediction)) of the left and the right half"""
        _, hs = self.case.analyse()
        O, E, Y = self.case.oey
        return [(w, predict(w, O, E, Y, self.case.cap or K.CAP, shortcut=r['kernel'] == 'shortcut')) for w, r in hs]

    def check(self):
        """asserts that both halves reach what they were built for"""
        for side, (want, (w, p)) in enumerate(zip(self.want, self.analyse())):
            if want is None:
                continue
            tag = (self.name, 'lr'[side])
            first = p['first']
            assert first is not None, tag
            ev = first['event']
            rows2 = None
            if want['event'] == 'fit':
                assert ev is None and first['widest'] == want['widest'] and not p['restarted'] and not p['widened'], (tag, first)
            elif want['event'] == 'widen':
                assert p['widened'] and first['at'] == 62 and (first['before'] is None or first['before'] <= 61), (tag, first)
                assert first['slid'] == bool(want.get('slid')), (tag, first)
                rows2 = _rows(w, FULL, ev[1] + 1, w.rows) if p['kernel'] == 'lean' else None
            else:
                assert p['restarted'], (tag, first)
                if want['event'] == 'row0':
                    assert ev[0] == 'row0' and 63 * W1 <= w.hi[0] < 63 * FULL, (tag, first, int(w.hi[0]))
                else:
                    assert ev[0] == 'band' and (first['before'] is None or first['before'] <= 61) and first['at'] >= 63, (tag, first)
                rows2 = _rows(w, FULL, 1, w.rows) if p['kernel'] == 'lean' else None
            assert p['kernel'] == want['kernel'], (tag, p)
            for k in ('edge', 'plain', 'fresh'):
                if want.get(k):
                    assert first[k], (tag, k, first)
                if want.get(k + '2'):
                    assert rows2 is not None and rows2[k], (tag, k + '2', rows2)


def fit(widest, **kw):
    return dict(event='fit', widest=widest, kernel='lean', **kw)


def leaves(event, kernel='lean', **kw):
    return dict(event=event, kernel=kernel, **kw)


def jump_pair(seed, n, side):
    """150 columns behind the anchor's site the query holds n bases that the target lacks, then both go on alike.  At a small gap
    extension the diagonal behind the insertion gains 100 a row while the best score stands still, and the last live column, the end
    of the column gap that leaves that diagonal, moves 100 / E columns a row: more than two strips of W1 columns at E = 5"""
    rng = np.random.default_rng(seed)
    before, after = K.rand(rng, 150), K.rand(rng, 600)
    return K._site_pair(rng, 500, np.concatenate([before, after]), np.concatenate([before, K.rand(rng, n), after]), side)


def cases():
    """the designed halves of the shipped W1.  Family W (k6_cases.w_pair: 7 kbp, both halves run into the query's end, so their
    windows slide, take in strips on the right and end in EDGE rows) over the y-drops at which its halves fill the narrow window to
    the last strip but three and but two, reach the last but one late, early and in row 1, and outgrow the window in row 0; J: the
    band jumps over the last strip but one; T: row 0 alone is beyond the narrow window, in a half that the pass at 14 holds or loses
    to the 2048-column kernel, and the other half ends 40 rows on with the query's end in the last strip but one; Q: the query
    ends inside the narrow window, or inside the window at 14 after the widening"""
    T, Q = K.w_pair()
    out = [
        StripCase(K.Case('W-y8100', T, Q, ydrop=8100), fit(59, edge=True, plain=True, fresh=True), fit(51, edge=True, plain=True, fresh=True)),
        StripCase(K.Case('W-y8250', T, Q, ydrop=8250), fit(60), fit(51)),
        StripCase(K.Case('W-y8350', T, Q, ydrop=8350), fit(61), fit(51)),
        StripCase(K.Case('W-y8400', T, Q, ydrop=8400), leaves('widen', plain=True, fresh=True, edge2=True, plain2=True, fresh2=True), fit(51)),
        StripCase(K.Case('W-y9400', T, Q), leaves('widen', plain=True, fresh=True, edge2=True, plain2=True, fresh2=True), fit(56)),
        StripCase(K.Case('W-y10000-minus', T, Q, minus=1, ydrop=10000), leaves('widen'), fit(59)),
        StripCase(K.Case('W-y11000', T, Q, ydrop=11000), leaves('widen', plain=True), leaves('widen', plain=True, edge2=True, plain2=True, fresh2=True)),
        StripCase(K.Case('W-y13600', T, Q, ydrop=13600), leaves('jump', plain2=True), leaves('jump', edge2=True)),
        StripCase(K.Case('W-y13700', T, Q, ydrop=13700), leaves('row0', edge2=True, plain2=True, fresh2=True), leaves('row0')),
        StripCase(K.Case('W-y18400', T, Q, ydrop=18400), leaves('row0', kernel='wide'), leaves('row0')),
    ]
    for side in 'rl':
        Tj, Qj = jump_pair(7000, 120, side)
        one = (lambda want: (None, want) if side == 'r' else (want, None))
        out.append(StripCase(K.Case('J-%s120-e5-y1850' % side, Tj, Qj, gap_extend=5, ydrop=1850), *one(leaves('jump', edge2=True, plain2=True, fresh2=True))))
        if side == 'r':   # two strips in the row after a slide, and no further
            out.append(StripCase(K.Case('J-r120-e8-y2872', Tj, Qj, gap_extend=8, ydrop=2872), *one(leaves('widen', slid=True))))
    for k, side in enumerate('rl'):
        # the target ends 40 bases from the anchor on one side, with 440 query bases left: row 1 fills the last strip but one.  The
        # other half has 500 bases of homology and 951 query bases left, and its row 0 is 446 or 700 columns wide
        Tt, Qt = K.end_pair(8200 + 100 * k + 40, 40, side, 't', far=500)
        two = (lambda far, near: (far, near) if side == 'r' else (near, far))
        near = leaves('widen', edge=True, edge2=True)
        out.append(StripCase(K.Case('T-%s40-e15-y7100' % side, Tt, Qt, gap_extend=15, ydrop=7100), *two(leaves('row0', plain2=True), near)))
        out.append(StripCase(K.Case('T-%s40-y21400' % side, Tt, Qt, ydrop=21400), *two(leaves('row0', kernel='wide'), near)))
    for k, (side, rem) in enumerate((('r', 430), ('l', 430), ('r', 700), ('l', 700))):
        Tq, Qq = K.end_pair(8000 + (100 if side == 'l' else 0) + rem, rem, side, 'q')
        want = fit(55 if rem == 430 else 56, edge=True, plain=rem == 700)
        out.append(StripCase(K.Case('Q-%s%d' % (side, rem), Tq, Qq, minus=1 if k == 2 else 0), *((None, want) if side == 'r' else (want, None))))
    return out
