"""The designed diagonals of tests/gapfree_cases.py, on the CPU: the checker is checked on them, and what they cover is ASSERTED.

tests/test_gpu_gapfree_edges.py holds the engine to the C oracle on these families.  That says something only if (a) the oracle is
right on them — so it is held to the plain-Python restatement tests/spec_v1.py on every family and parameter set, on every
SPEC_EVERY-th case of each family (the restatement takes 0.7 s per 45 kbp; whole families would take minutes) — and (b) the families
really reach the edges they were designed for: the stop steps, best-prefix lengths, x-drop boundaries, threshold boundaries and reach
offsets below are conditions on the inputs, proven with a walk that shares no code with the oracle or the engine.  A family that
misses a condition is to be changed; the condition is not."""
import numpy as np
import pytest

from oracle import oracle as O
from tests import gapfree_cases as G
from tests import spec_v1 as S

SPEC_EVERY = 61
COLS = ['tstart', 'qstart', 'length', 'score', 'raw_score']
_cache = {}


def suites():
    if 'full' not in _cache:
        _cache['full'] = G.suites()
    return _cache['full']


def oracle_hsps(name, pair, run):
    key = (name, tuple(sorted(run.items())))
    if key not in _cache:
        q, strand = G.query(pair, run)
        _cache[key] = O.ungapped_hsps(pair.T, q, strand, O.default_params(chain=0, **G.engine_kw(run)))
    return _cache[key]


def by_case(pair, hsps):
    """the HSPs of every designed diagonal, as sorted tuples"""
    out = [[] for _ in pair.cases]
    d = hsps['qstart'].astype(np.int64) - hsps['tstart'].astype(np.int64)
    for h, dd in zip(hsps, d):
        k, r = divmod(int(dd) - 11, 7)
        if r == 0 and 0 <= k < len(pair.cases) and pair.cases[k][0] - 100 <= int(h['tstart']) <= pair.cases[k][0] + pair.cases[k][2]:
            out[k].append(tuple(int(h[c]) for c in COLS))
    return [sorted(o) for o in out]


def spans(hs, lo, hi):
    """one HSP, on target columns lo .. hi - 1 and no more than chance matches of the random flanks beyond"""
    return len(hs) == 1 and lo - 40 <= hs[0][0] <= lo and hi <= hs[0][0] + hs[0][2] <= hi + 40


# ------------------------------------------------------------------------------------------------ the checker is checked
@pytest.mark.parametrize('name', ['A', 'AX', 'B6', 'B6N', 'B6M', 'B78', 'C', 'D', 'E'])
def test_oracle_equals_the_second_restatement_on_every_family_and_parameter_set(name):
    if 'spec' not in _cache:
        _cache['spec'] = G.suites(every=SPEC_EVERY)        # (families D and E are small: every third case, every case)
    pair, runs = _cache['spec'][name]
    if runs is None:
        runs = G.c_runs(O.ungapped_hsps(pair.T, pair.Q, 0, O.default_params(chain=0, hspthresh=1500)), n=2)[2]
    total = 0
    for run in runs:
        q, strand = G.query(pair, run)
        got = O.ungapped_hsps(pair.T, q, strand, O.default_params(chain=0, **G.engine_kw(run)))
        exp = S.ungapped_hsps(pair.T.decode(), S.revcomp(q.decode()) if strand else q.decode(), run.get('hspthresh', 3000),
                              run.get('xdrop', 910), bool(run.get('transitions', 1)), bool(run.get('entropy', 1)))
        assert sorted(tuple(int(h[c]) for c in COLS) for h in got) == sorted(exp), (name, run)
        total += len(exp)
    assert total > 0, name


E_RECIPES = [G.family_e(n, r) for n in G.E_STEPS for r in ('seeded', 'seedless')]      # as gapfree_cases.suites builds family E


# ------------------------------------------------------------------------------------------------ coverage
def _heads(name, xdrop=910):
    """the plain walk on the head (first extended hit) of every designed diagonal of a pair, or (name 'cut') of the cut-out
    scaffolds that the GPU test's batched call runs"""
    key = ('heads', name, xdrop)
    if key not in _cache:
        if name == 'cut':
            ex = [G.extended_hits(t.tobytes(), q.tobytes(), (0, 0, t.size), xdrop) for t, q in G.batched_cutouts(suites())[0]]
        else:
            pair = suites()[name][0]
            ex = [G.extended_hits(pair.T, pair.Q, c, xdrop) for c in pair.cases]
        assert all(ex), name                                 # every designed diagonal has a head
        _cache[key] = [e[0] for e in ex]
    return _cache[key]


def _missing(wanted, have):
    return [v for v in wanted if v not in have]


def test_family_a_stop_steps_and_best_prefix_lengths():
    """Every stop step and best-prefix length the families were designed for occurs among the heads of families A / AX — in the 620 kbp pairs or
    in the cut-out scaffolds of the batched call, where a walk also ends by running out of sequence.  By x-drop alone (the pairs, x-drop 910) the
    left walk, which crosses the 19 seed columns first, cannot stop before step 27 and the right walk not before step 8 —
    a column costs at most 125 — so steps 20..26 and 1..7 exist only at a scaffold's end."""
    pairs = _heads('A') + _heads('AX')
    cuts = _heads('cut')
    # of the cut-outs the batched call gives those in `checked` to the oracle: the steps only a sequence end supplies are among them
    checked = [cuts[i] for i in G.batched_cutouts(suites())[1]]
    assert _missing(range(20, 27), {h['left_stop'] for h in checked}) == [] and _missing(range(1, 8), {h['right_stop'] for h in checked}) == []
    left = {h['left_stop'] for h in pairs + cuts}
    right = {h['right_stop'] for h in pairs + cuts}
    assert _missing(list(range(20, 111)) + list(range(250, 263)), left) == []
    assert _missing(list(range(1, 81)) + list(range(250, 263)), right) == []
    # the part an x-drop can produce is produced by an x-drop, inside a long pair
    assert _missing(list(range(27, 111)) + list(range(250, 263)), {h['left_stop'] for h in pairs}) == []
    assert _missing(list(range(8, 81)) + list(range(250, 263)), {h['right_stop'] for h in pairs}) == []
    # the window hand-overs: 32 / 64 / 80 / 96 steps of the frame walks and the filter's left blocks, 256 of the per-lane walk
    both = (31, 32, 33, 63, 64, 65, 79, 80, 81, 255, 256, 257)
    assert _missing(both + (95, 96, 97), {h['left_best'] for h in pairs}) == []
    assert _missing(both, {h['right_best'] for h in pairs}) == []
    assert max(h['left_best'] for h in pairs) > 400 and max(h['right_best'] for h in pairs) > 400
    # all diagonals of family A carry an HSP at the default parameters
    assert sum(1 for c in by_case(suites()['A'][0], oracle_hsps('A', *suites()['A'][:1], {})) if c) == len(suites()['A'][0].cases)


def test_pre_filter_block_edges_have_a_stop_on_either_side():
    """pair_needs_walk's checkpoints: left steps 24 / 48 / 72 / 96, right steps 24 / 48 / 64.  For each, a head's walk stops in the
    block that ends there and another's in the block behind it (behind the last block: outside the frame).  And the filter's own
    proof — its cheap bounds, restated in gapfree_cases.k34_proven_block — comes at every checkpoint where a proof can
    come at all (none can after the left walk's first block: the seed's twelve care columns lie in it)."""
    pairs = _heads('A') + _heads('AX')
    cuts = _heads('cut')
    for side, edges in (('left_stop', (24, 48, 72, 96)), ('right_stop', (24, 48, 64))):
        stops = np.array([h[side] for h in pairs + cuts])
        for j, e in enumerate(edges):
            lo = edges[j - 1] if j else 0
            hi = edges[j + 1] if j + 1 < len(edges) else e + 24
            assert ((stops > lo) & (stops <= e)).any() and ((stops > e) & (stops <= hi)).any(), (side, e)
            assert (stops == e).any() and (stops == e + 1).any(), (side, e)
    proofs = {'l': set(), 'r': set()}
    for name in ('A', 'AX'):
        pair = suites()[name][0]
        for case, h in zip(pair.cases, _heads(name)):
            a, b, _ = G.columns(pair.T, pair.Q, case[1] - case[0], h['et'] - 96, h['et'] + 64)
            proofs['l'].add(G.k34_proven_block(a[:96][::-1], b[:96][::-1], 910, G.K34_LEFT)[0])
            proofs['r'].add(G.k34_proven_block(a[96:], b[96:], 910, G.K34_RIGHT)[0])
    assert proofs['l'] == {1, 2, 3, None} and proofs['r'] == {0, 1, 2, None}, proofs


def test_family_e_sits_on_the_pre_filters_strict_comparison():
    """bound_block2's `up + xdrop < lomax`: on the seedless-rescue cases the bound equals the running score, which is exactly -xdrop at
    the checkpoint; the strict comparison proves nothing there, `<=` would prove a stop — and the walk goes on into the
    rescue, to an HSP above the threshold that a filter with `<=` drops (nothing else on the diagonal could bring it back)."""
    pair, runs = suites()['E']
    recipes = E_RECIPES
    for n, blocks in ((24, 0), (48, 1), (64, 2)):
        run = next(r for r in runs if r['xdrop'] == G.e_xdrop(n))
        for k, r in enumerate(recipes):
            if r != G.family_e(n, 'seedless') and r != G.family_e(n, 'seeded'):
                continue
            t0, q0, ln = pair.cases[k]
            ex = G.extended_hits(pair.T, pair.Q, pair.cases[k], run['xdrop'])
            head = ex[0]
            assert head['t'] == t0 + 24 and head['right_best'] >= ln - 46 and head['raw'] >= 6000, (n, k, head)
            a, b, _ = G.columns(pair.T, pair.Q, q0 - t0, head['et'], head['et'] + 64)
            assert G.k34_proven_block(a, b, run['xdrop'], G.K34_RIGHT, strict=True) == (None, True), (n, k)
            assert G.k34_proven_block(a, b, run['xdrop'], G.K34_RIGHT, strict=False)[0] == blocks, (n, k)
            # the whole filter, restated: nothing else keeps the hit, so `<=` alone would dismiss it
            assert G.k34_needs_walk(pair.T, pair.Q, head['t'], q0 - t0, run['xdrop'], run['hspthresh'])
            assert not G.k34_needs_walk(pair.T, pair.Q, head['t'], q0 - t0, run['xdrop'], run['hspthresh'], strict=False)
            if r == G.family_e(n, 'seedless'):
                assert head['hits'] == [head['t']], (n, k, head['hits'])          # the only seed hit of the diagonal
            hs = by_case(pair, oracle_hsps('E', pair, run))[k]
            assert spans(hs, t0 + 24, t0 + ln - 3), (n, k, hs)


def test_family_e_sits_on_the_walk_queue_filters_strict_comparison():
    """bound_window's `U + xdrop < lomax` (hit_needs_walk: the filter of the walk-queue kernel behind K34 and of MIMEO_HEAVY=v1,
    checkpoints every 16 steps): at steps 16, 32, 48 and 64 its bound U is the running score, exactly -xdrop, with nothing
    better than the empty prefix before; `<` proves nothing, `<=` would prove a stop.  Only the bound is restated here, not the
    rest of that filter (its seed veto, its left side); what `<=` does to the results was measured once on the device
    (profiles/r11_gapfree_edges_durations.txt)."""
    pair, runs = suites()['E']
    for n in (16, 32, 48, 64):
        run = next(r for r in runs if r['xdrop'] == G.e_xdrop(n))
        for k, r in enumerate(E_RECIPES):
            if r not in (G.family_e(n, 'seedless'), G.family_e(n, 'seeded')):
                continue
            t0, q0, ln = pair.cases[k]
            head = G.extended_hits(pair.T, pair.Q, pair.cases[k], run['xdrop'])[0]
            assert head['t'] == t0 + 24 and head['right_best'] >= ln - 46 and head['raw'] >= 6000, (n, k, head)
            a, b, _ = G.columns(pair.T, pair.Q, q0 - t0, head['et'], head['et'] + 64)
            assert G.k4_proven_block(a, b, run['xdrop']) == (None, True), (n, k)
            assert G.k4_proven_block(a, b, run['xdrop'], strict=False)[0] == n // 16 - 1, (n, k)


# ------------------------------------------------------------------------------------------------ family B
def _b_layout(pair):
    """(side, seeded) of every case: family_b emits right / left for the seeded rescue, then for the seedless one"""
    return [(('right', 'left')[k % 2], k // 2 % 2 == 0) for k in range(len(pair.cases))]


@pytest.mark.parametrize('name,c,need', [('B6', 738, 40), ('B6N', 600, 10)])
def test_family_b_changes_exactly_at_the_dips_cost(name, c, need):
    """between x-drop c - 1 and c (c = what the dip costs) a seeded diagonal goes from two HSPs to one; between c and c + 1 no designed
    diagonal changes at all"""
    pair = suites()[name][0]
    lo, at, hi = (by_case(pair, oracle_hsps(name, pair, {'xdrop': x})) for x in (c - 1, c, c + 1))
    changed = {'right': 0, 'left': 0}
    for k, (side, seeded) in enumerate(_b_layout(pair)):
        if seeded and len(lo[k]) == 2 and len(at[k]) == 1:
            changed[side] += 1
            t0, q0, n = pair.cases[k]
            assert spans(at[k], t0, t0 + n), (k, at[k])              # the one HSP is the whole copy
        if not seeded:
            assert len(lo[k]) == len(at[k]) == 1                     # a seedless rescue is reached from the core or not at all
    assert changed['right'] >= need and changed['left'] >= need, changed
    assert at == hi
    assert sum(1 for a, b in zip(lo, at) if a != b) >= 3 * need      # the seedless rescues change too: one HSP grows


def test_family_b_at_the_default_x_drop():
    """910: seven dip columns (861) are crossed, eight (984) are not"""
    pair = suites()['B78'][0]
    hs = by_case(pair, oracle_hsps('B78', pair, {}))
    half = len(pair.cases) // 2                                      # family_b: all of m = 7, then all of m = 8
    crossed = {7: 0, 8: 0}
    for k, (side, seeded) in enumerate(_b_layout(pair)):
        if seeded:
            crossed[7 if k < half else 8] += len(hs[k]) == 1
            assert k < half or len(hs[k]) == 2, (k, hs[k])
    assert crossed[7] >= 30 and crossed[8] == 0, crossed


def test_soft_masked_core_has_no_head():
    """B6M: the target's core in lower case carries no seed word; the diagonal's first hit lies in the rescue or (seedless
    rescue) nowhere"""
    pair = suites()['B6M'][0]
    hs = by_case(pair, oracle_hsps('B6M', pair, {'xdrop': 738}))
    for k, (side, seeded) in enumerate(_b_layout(pair)):
        ex = G.extended_hits(pair.T, pair.Q, pair.cases[k], 738)
        t0, _, n = pair.cases[k]
        core = (t0, t0 + 40) if side == 'right' else (t0 + n - 40, t0 + n)
        assert all(not (core[0] - 18 <= t < core[1]) for t in (ex[0]['hits'] if ex else [])), k
        assert len(hs[k]) == (1 if seeded else 0), (k, hs[k])


# ------------------------------------------------------------------------------------------------ family C
def test_family_c_every_chosen_threshold_keeps_an_hsp_that_the_next_one_loses():
    pair = suites()['C'][0]
    base = oracle_hsps('C', pair, {'hspthresh': 1500})
    raw, adj, runs = G.c_runs(base)
    assert len(raw) == 6 and len(adj) == 6
    assert (base['score'] < base['raw_score']).sum() > 50             # the entropy factor bites
    assert base['raw_score'].min() < 2000 and base['raw_score'].max() > 4000
    for scores, col, entropy in ((raw, 'raw_score', 0), (adj, 'score', 1)):
        for s in scores:
            keep = oracle_hsps('C', pair, {'hspthresh': s, 'entropy': entropy})
            lose = oracle_hsps('C', pair, {'hspthresh': s + 1, 'entropy': entropy})
            assert keep.size > lose.size and (keep[col] == s).any() and not (lose[col] == s).any(), (col, s)


# ------------------------------------------------------------------------------------------------ family D
def test_family_d_reach_offsets():
    """Y's seed ends at the head's reach - 1, at it and one behind it: skipped, skipped, extended — the head itself scoring below the
    threshold, so that only its reach is left of it"""
    pair, runs = suites()['D']
    hs = by_case(pair, oracle_hsps('D', pair, runs[0]))
    seen = {-1: 0, 0: 0, 1: 0}
    for k, (case, delta) in enumerate(zip(pair.cases, pair.meta)):
        t0, q0, n = case
        ex = G.extended_hits(pair.T, pair.Q, case, 500)
        head = ex[0]
        assert t0 - 18 <= head['t'] <= t0 and head['reach'] == t0 + 46 and head['raw'] < 6000, (k, head)
        y = head['reach'] + delta - 19
        assert y in head['hits'], (k, delta)
        seen[delta] += 1
        extended = [e['t'] for e in ex]
        if delta == 1:
            assert extended[1] == y and ex[1]['start'] <= t0 and ex[1]['reach'] >= t0 + n and ex[1]['raw'] >= 6000, (k, ex[1])
            assert spans(hs[k], t0, t0 + n), (k, hs[k])
        else:
            assert y not in extended and head['reach'] + 1 - 19 not in head['hits'], (k, extended)
            assert spans(hs[k], t0 + 51, t0 + n) and hs[k][0][0] == t0 + 51, (k, hs[k])
    assert min(seen.values()) >= 5, seen
