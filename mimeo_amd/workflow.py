"""The three mimeo workflows with the shell pipeline replaced by engine calls.

Mirrors the reference's command builders + executor:
  self_repeats  <- wrappers.py:899-1271 self_LZ_cmds   + utils.py:213-254 run_cmd
  x_repeats     <- wrappers.py:683-896  xspecies_LZ_cmds
  map_hits      <- wrappers.py:525-680  map_LZ_cmds, :33-117 import_Align, :443-522 writeGFFlines
Same argument names and meaning as those functions where they still apply; `lzpath` /
`bdtlsPath` are gone because no external tool is run.
"""
import logging
import os

import numpy as np

from . import engine, formats
from .dist import Dist, deal_units, shard_pairs_by_target


def all_pairs(n_a, n_b=None):
    """utils.py:65-106 get_all_pairs: full ordered Cartesian product; self mode includes (A,A)
    and both orders.  The reference inherits the order of glob(); here it is FASTA order."""
    if n_b is None:
        return [(a, b) for a in range(n_a) for b in range(n_a)]
    return [(a, b) for a in range(n_a) for b in range(n_b)]


def anchor_rule_code(rule):
    """'box' / 'path' (CLI --anchorRule) or the number itself -> mimeo_params.anchor_rule"""
    if isinstance(rule, str):
        if rule not in engine._ffi.ANCHOR_RULES:
            raise ValueError('anchor rule must be one of %s, not %r' % (sorted(engine._ffi.ANCHOR_RULES), rule))
        return engine._ffi.ANCHOR_RULES[rule]
    return int(rule)


def gapped_params(hspthresh, anchor_rule, bound_extensions):
    """engine parameters of a workflow: --hspthresh, --anchorRule, --boundExtensions (only with the path rule)"""
    rule = anchor_rule_code(anchor_rule)
    if bound_extensions and rule != engine._ffi.ANCHOR_PATH:
        raise ValueError('bound_extensions needs the path anchor rule (anchor_rule=%r)' % (anchor_rule,))
    return engine.default_params(hspthresh=hspthresh, anchor_rule=rule, bound_extensions=1 if bound_extensions else 0)


PACK_MEMBER_BP = 6 << 20   # the engine packs scaffolds of up to this size into super-scaffolds when there are at least ...
PACK_MIN = 8               # ... this many of them (mimeo_hip.h, mimeo_align_pairs)


def align_blocks(A, B, pairs, params, min_len, min_idt, dist=None, paths=False, divergence=False, paf_rows=True):
    """Align every pair (sharded over ranks when dist.world > 1) and return {(t, q): [TAB lines]} on every rank, the raw
    record count and the (n, 4) array of (tid, qid, start1, end1) of the rows kept — what the BED projection of the TAB reads
    back (wrappers.py:1120-1128).

    Sharding (by target scaffold, no data-path collective).  A self job over the full pair matrix of large
    scaffolds deals UNITS (dist.deal_units): a rank gets its target rows' minus-strand units and the plus-strand units of the
    unordered pairs dealt to those rows, in both orders, so that the engine computes each plus-strand pair once.  Fragmented
    assemblies (the engine packs them into super-scaffolds when it is handed a full cross product) and two-genome jobs are
    sharded by target with whole pairs, as before.

    paths=True (--paf): the engine also returns every alignment's path, the block counts and the blocks travel through the
    same all-gatherv as the records, and a fourth value comes back: {(t, q): [PAF lines]}, the rows of the TAB blocks in
    their order.  divergence=True (--divergence, with paths): rank 0, which writes the file, also asks the engine for the column
    statistics of the rows that are written (engine.path_stats on the kept rows only: every rank holds the genomes and the
    gathered paths, so no collective is added) and its PAF lines carry the tags of formats.divergence_tags.  With paths a fifth
    value follows: (records, first, blocks) of the rows kept, in the order of `kept` — what --regionStats joins with the regions
    and what --maf and --cs ask the engine's text for (write_maf, write_paf).
    paf_rows=False: the paths are wanted for that alone, no PAF line is made and the fourth value is empty."""
    dist = dist or Dist()
    none = (np.zeros(0, dtype=engine._ffi.ALIGNMENT), np.zeros(1, dtype=np.uint64), np.zeros(0, dtype=engine._ffi.PATH_BLOCK))
    first = blk = None

    def run(fn, work):
        if not work:
            return none if paths else none[0]
        return fn(A, B, work, params, paths=True) if paths else fn(A, B, work, params)
    QG = B if B is not None else A
    n = len(A.names)
    failed = []
    if dist.world > 1:
        small = sum(1 for ln in A.lengths if ln <= PACK_MEMBER_BP)
        full_self = B is None and len(pairs) == n * n and len(set(pairs)) == n * n
        if full_self and small < PACK_MIN:
            cost = {t: A.lengths[t] * sum(A.lengths) for t in range(n)}
            units = deal_units(n, cost, dist.world, dist.rank)
            alns = run(engine.align_units, units)
            failed = [(units[i][0], units[i][1]) for i, _ in engine.failed_pairs()] if units else []
        else:
            qsum = {}
            for t, q in pairs:
                qsum[t] = qsum.get(t, 0) + QG.lengths[q]
            cost = {t: A.lengths[t] * s for t, s in qsum.items()}
            mine = shard_pairs_by_target(pairs, cost, dist.world, dist.rank)
            alns = run(engine.align_pairs, mine)
            failed = [mine[i] for i, _ in engine.failed_pairs()] if mine else []
    else:
        mine = list(pairs)
        alns = run(engine.align_pairs, mine)
        failed = [mine[i] for i, _ in engine.failed_pairs()] if mine else []
    if paths:
        alns, first, blk = alns
        first, blk = dist.allgather_paths(first, blk)
    alns = dist.allgather_records(alns)
    alns, first, blk, left_out = drop_failed_pairs(dist, alns, first, blk, failed)
    for t, q in (left_out if dist.rank == 0 else ()):   # the reference's script loses a failing lastz run's rows and goes on (utils.py:125-128)
        logging.warning('Alignment of %s onto %s hit an engine limit and was left out (a DP band wider than 65536 columns, or a '
                        'traceback larger than the trace pool)', QG.names[q], A.names[t])
    if not paths:
        blocks, kept = formats.tab_blocks(alns, A.names, QG.names, min_len, min_idt)
        return blocks, int(alns.size), kept
    rows = []
    blocks, kept = formats.tab_blocks(alns, A.names, QG.names, min_len, min_idt, rows=rows)
    f2, b2 = formats.select_paths(first, blk, rows[0])
    if not paf_rows:
        return blocks, int(alns.size), kept, {}, (alns[rows[0]], f2, b2)
    stats = engine.path_stats(A, B, alns[rows[0]], f2, b2) if divergence and dist.rank == 0 else None
    paf = formats.paf_lines(alns[rows[0]], f2, b2, A.names, A.lengths, QG.names, QG.lengths, stats=stats)
    paf_blocks, at = {}, 0
    for pr in sorted(blocks):   # tab_blocks makes its blocks in (tid, qid) order
        paf_blocks[pr] = paf[at:at + len(blocks[pr])]
        at += len(blocks[pr])
    return blocks, int(alns.size), kept, paf_blocks, (alns[rows[0]], f2, b2)


def drop_failed_pairs(dist, alns, first, blk, failed):
    """What is left out of a job is a scaffold pair (mimeo_hip.h, mimeo_get_failed_pairs), on every rank: `failed`, this
    rank's (t, q) that hit an engine limit, are exchanged (one all-gatherv, which every rank joins — a rank without work or
    without failures too), and every record of a pair of the union goes, with its path: the other strand of a pair whose
    strands dist.deal_units dealt to two ranks was computed by a rank that saw nothing fail.  alns (and first / blk, or None
    without paths): the gathered records.  Returns (alns, first, blk, the sorted union); the order of the rest is kept."""
    mine = np.array(sorted(set((int(t), int(q)) for t, q in failed)), dtype=np.uint32).reshape(-1, 2)
    union = sorted(set(map(tuple, dist.allgather_records(mine).reshape(-1, 2).tolist())))
    if union and alns.size:
        key = alns['tid'].astype(np.uint64) << np.uint64(32) | alns['qid'].astype(np.uint64)
        keep = np.flatnonzero(~np.isin(key, np.array([t << 32 | q for t, q in union], dtype=np.uint64)))
        if first is not None:
            first, blk = formats.select_paths(first, blk, keep)
        alns = alns[keep]
    return alns, first, blk, union


TEXT_BUDGET = 1 << 26   # columns of alignment text asked of the engine at once by the writers: two rows of 64 MiB


def file_order(pairs, blocks, splitSelf=False):
    """The kept rows (numbered as align_blocks returns them: pair by pair in sorted (t, q) order, the order of each TAB block)
    in the order the files list them: pair by pair as write_tab / write_paf go through `pairs`, with --strictSelf the
    same-scaffold rows behind the others."""
    at, start = 0, {}
    for pr in sorted(blocks):
        start[pr] = at
        at += len(blocks[pr])
    out = []
    for intra in ((False, True) if splitSelf else (None,)):
        for pr in pairs:
            if intra is not None and (pr[0] == pr[1]) != intra:
                continue
            if pr in start:
                out.append(np.arange(start[pr], start[pr] + len(blocks[pr]), dtype=np.int64))
    return np.concatenate(out) if out else np.zeros(0, dtype=np.int64)


def text_runs(columns, budget):
    """Cut rows 0 .. len(columns) into runs [i0, i1) of consecutive rows whose columns add up to at most `budget`; a single
    longer row goes alone."""
    runs, i0, n = [], 0, len(columns)
    while i0 < n:
        i1, c = i0 + 1, int(columns[i0])
        while i1 < n and c + int(columns[i1]) <= budget:
            c += int(columns[i1])
            i1 += 1
        runs.append((i0, i1))
        i0 = i1
    return runs


def path_text_runs(A, B, kept_paths, order, budget=TEXT_BUDGET):
    """The alignment text of the rows `order` of kept_paths = (records, first, blocks), run by run (text_runs): yields
    (j0, j1, records, first, blocks, row_first, trow, qrow) for order[j0:j1], one engine.path_text call each, so that the host
    never holds more than about `budget` columns of text — a chromosome-long self diagonal is half a gigabyte of rows, and a
    large job's rows do not fit in memory at once.  What is yielded depends on the rows alone, not on the budget."""
    recs, first, blk = kept_paths
    f2, b2 = formats.select_paths(first, blk, order)
    r2 = recs[order]
    for j0, j1 in text_runs(formats.path_columns(f2, b2), budget):
        k0, k1 = int(f2[j0]), int(f2[j1])
        fr, br = f2[j0:j1 + 1] - f2[j0], b2[k0:k1]
        yield (j0, j1, r2[j0:j1], fr, br) + tuple(engine.path_text(A, B, r2[j0:j1], fr, br))


def write_paf(path, pairs, paf_blocks, splitSelf=False, cs=None):
    """--paf: the PAF row of every row of the TAB, in the TAB's order (write_tab); with --strictSelf the rows of the
    same-scaffold TAB follow those of the main one.  No header: PAF has none.  cs (--cs): (A, B, kept_paths, blocks, budget)
    — every row also ends in cs:Z: (formats.cs_tag), made from the engine's alignment text run by run (path_text_runs)."""
    lines = []
    for intra in ((False, True) if splitSelf else (None,)):
        for pr in pairs:
            if intra is not None and (pr[0] == pr[1]) != intra:
                continue
            lines.extend(paf_blocks.get(pr, ()))
    with open(path, 'w') as f:
        if cs is None:
            for line in lines:
                f.write(line + '\n')
            return
        A, B, kept_paths, blocks, budget = cs
        order = file_order(pairs, blocks, splitSelf)
        assert order.size == len(lines)
        for j0, j1, _, _, _, row_first, trow, qrow in path_text_runs(A, B, kept_paths, order, budget):
            for line, tag in zip(lines[j0:j1], formats.cs_tags(row_first, trow, qrow)):
                f.write(line + '\tcs:Z:' + tag + '\n')


def write_maf(path, A, B, pairs, blocks, kept_paths, splitSelf=False, budget=TEXT_BUDGET):
    """--maf: one MAF block (formats.maf_lines) per row of the TAB, in the TAB's order; with --strictSelf the rows of the
    same-scaffold TAB follow those of the main one, as in write_paf.  blocks: the TAB blocks of align_blocks; kept_paths: its
    (records, first, blocks) of the rows kept.  The text comes from the engine (engine.path_text, kernel K11) in runs of at most
    `budget` columns; the bytes written do not depend on the budget."""
    QG = B if B is not None else A
    with open(path, 'w') as f:
        f.write(formats.MAF_HEADER + '\n')
        for _, _, recs, first, blk, row_first, trow, qrow in path_text_runs(A, B, kept_paths, file_order(pairs, blocks, splitSelf), budget):
            for block in formats.maf_lines(recs, row_first, trow, qrow, first, blk, A.names, A.lengths, QG.names, QG.lengths):
                f.write(block + '\n')


def write_tab(path, pairs, blocks, select=None):
    """Header + one sorted block per pair, appended in pair order (wrappers.py:996, :1056)."""
    with open(path, 'w') as f:
        f.write(formats.TAB_HEADER + '\n')
        for pr in pairs:
            if select is not None and not select(pr):
                continue
            for line in blocks.get(pr, ()):  # a pair without surviving rows adds nothing
                f.write(line + '\n')


def collapse_to_gff(tab_path, names, lengths, min_cov, min_len, source, label, prefix, kept=None, regions_out=None):
    """wrappers.py:1116-1177: TAB -> BED -> depth >= minCov -> merge -> minLen -> GFF rows.  `kept`: the (tid, start1, end1)
    of the rows this process has just written to `tab_path` (tid = index into `names`) — the same numbers the BED projection
    would read back from the file, without parsing 6e5 lines again; None: read the file (--recycle, imported TABs).
    regions_out (a list, optional) receives the regions behind the lines, as engine.coverage_collapse returned them
    (chrom = index into the sorted names)."""
    names_sorted = sorted(names, key=lambda s: s.encode())
    cid = {n: i for i, n in enumerate(names_sorted)}
    length_of = dict(zip(names, lengths))
    if kept is not None:
        rank = np.array([cid[n] for n in names], dtype=np.uint32)
        iv = np.stack([rank[kept[:, 0]], kept[:, 1].astype(np.uint32), kept[:, 2].astype(np.uint32)], axis=1) if kept.shape[0] else np.zeros((0, 3), np.uint32)
    else:
        iv = formats.bed_intervals(formats.parse_tab(tab_path), cid)
    if iv.shape[0] == 0:
        return []
    regions = engine.coverage_collapse(iv, [length_of[n] for n in names_sorted], min_cov, min_len)
    if regions_out is not None:
        regions_out.append(regions)
    return formats.gff_repeat_lines(regions, names_sorted, source, label, prefix)


def region_stat_block(A, B, kept_paths, select, regions, prefix, header):
    """--regionStats for one block of GFF3 rows: the rows `select` (a mask) of the kept rows' (records, first, blocks) joined
    with `regions` (formats.region_items), one engine.window_stats call, the lines of formats.region_stat_lines."""
    recs, first, blk = kept_paths
    rows = np.flatnonzero(select)
    f2, b2 = formats.select_paths(first, blk, rows)
    names_sorted = sorted(A.names, key=lambda s: s.encode())
    cid = {n: i for i, n in enumerate(names_sorted)}
    items, per_region = formats.region_items(recs[rows], regions, [cid[n] for n in A.names], first=f2, blocks=b2, self_job=B is None)
    stats = engine.window_stats(A, B, recs[rows], f2, b2, items, len(regions))
    return formats.region_stat_lines(regions, names_sorted, prefix, stats, per_region, header=header)


def terminal_calls(A, regions, window, min_score):
    """What --terminalRepeats and --elements share for one block of GFF3 rows: the regions as intervals of their scaffolds, one
    engine.terminal_repeats call (kernel K17: each region's head against its tail, direct and inverted) and one
    engine.path_stats call (K9) over the returned records.  Returns (names_sorted, intervals, records, stats)."""
    names_sorted = sorted(A.names, key=lambda s: s.encode())
    tid = {n: i for i, n in enumerate(A.names)}
    iv = np.zeros(len(regions), dtype=engine._ffi.INTERVAL)
    if len(regions):
        iv['chrom'] = [tid[names_sorted[int(c)]] for c in regions['chrom']]
        iv['start'], iv['end'] = regions['start'], regions['end']
    recs, first, blk = engine.terminal_repeats(A, iv, window=int(window), min_score=int(min_score))
    return names_sorted, iv, recs, engine.path_stats(A, None, recs, first, blk)


def terminal_block(A, regions, prefix, window, min_score, header, calls=None):
    """--terminalRepeats for one block of GFF3 rows: terminal_calls (or what it returned, `calls`, where --elements made the
    calls already) and the lines of formats.terminal_repeat_lines.  Needs no alignment of the job: only the regions."""
    names_sorted, _, recs, stats = calls if calls is not None else terminal_calls(A, regions, window, min_score)
    return formats.terminal_repeat_lines(regions, names_sorted, prefix, window, recs, stats, header=header)


def genome_letters(A, spans):
    """The letters (A C G T, N for everything else) of the plus-strand stretches (scaffold id, start, end), end > start, of the
    resident genome: one engine.path_text call (K11) over one-block paths of each stretch against itself."""
    n = len(spans)
    if not n:
        return []
    s = np.asarray(spans, dtype=np.int64).reshape(-1, 3)
    recs = np.zeros(n, dtype=engine._ffi.ALIGNMENT)
    recs['tid'] = recs['qid'] = s[:, 0]
    recs['tstart'] = recs['qstart'] = s[:, 1]
    recs['tend'] = recs['qend'] = s[:, 2]
    recs['id_n'] = recs['id_d'] = s[:, 2] - s[:, 1]
    blk = np.zeros(n, dtype=engine._ffi.PATH_BLOCK)
    blk['t'] = blk['q'] = s[:, 1]
    blk['len'] = s[:, 2] - s[:, 1]
    rf, trow, _ = engine.path_text(A, None, recs, np.arange(n + 1, dtype=np.uint64), blk)
    return [bytes(trow[int(rf[i]):int(rf[i + 1])]).decode() for i in range(n)]


def elements_block(A, regions, prefix, window, min_score, tsd, min_orf, header, calls=None):
    """--elements for one block of GFF3 rows (the lines of formats.element_lines): (1) terminal_calls — K17 over the regions, K9
    over its records; (2) for every orientation found the element is [tstart, qend), and one engine.flank_repeats call (K18,
    parameters `tsd`: min_len, max_len, slack, max_mismatch) covers all of them; (3) per feature the orientation with a
    target-site duplication is chosen — both or neither: the higher K17 score, then LTR; (4) the element is
    [tstart + dl, qend + dr), the feature itself where no orientation was found; (5) one engine.open_frames call (K19) covers
    the n elements; (6) the letters of the duplications and of the elements' ends come from the resident genome
    (genome_letters).  Needs no alignment of the job: only the regions."""
    names_sorted, iv, recs, stats = calls if calls is not None else terminal_calls(A, regions, window, min_score)
    n = len(regions)
    found = [(k, o) for k in range(n) for o in (0, 1) if int(recs[2 * k + o]['id_d']) > 0]
    span = np.zeros(len(found), dtype=engine._ffi.INTERVAL)
    for j, (k, o) in enumerate(found):
        span[j] = (iv[k]['chrom'], recs[2 * k + o]['tstart'], recs[2 * k + o]['qend'])
    fl = engine.flank_repeats(A, span, **tsd)
    cands = [[] for _ in range(n)]
    for j, (k, o) in enumerate(found):
        cands[k].append((o, j))
    rows, el = [], np.zeros(n, dtype=engine._ffi.INTERVAL)
    el[:] = iv
    for k in range(n):
        with_tsd = [c for c in cands[k] if int(fl[c[1]]['len'])]
        pool = with_tsd if len(with_tsd) == 1 else cands[k]
        row = dict(kind=None, tsd=None)
        if pool:
            o, j = min(pool, key=lambda c: (-int(recs[2 * k + c[0]]['score']), c[0]))
            a, f = recs[2 * k + o], fl[j]
            el[k]['start'], el[k]['end'] = int(span[j]['start']) + int(f['dl']), int(span[j]['end']) + int(f['dr'])
            row.update(kind=formats.TERMINAL_KINDS[o], left_len=int(a['tend']) - int(a['tstart']), right_len=int(a['qend']) - int(a['qstart']),
                       score=int(a['score']), stats=stats[2 * k + o])
            if int(f['len']):
                row['tsd'] = [int(f['len']), (int(iv[k]['chrom']), int(f['left_start']), int(f['left_start']) + int(f['len'])), int(f['mismatches']), int(f['dl']),
                              int(f['dr'])]
        row['el'] = (int(el[k]['start']), int(el[k]['end']))
        rows.append(row)
    fr = engine.open_frames(A, el)
    want = []   # (row, what, stretch)
    for k, row in enumerate(rows):
        c, (a, b) = int(iv[k]['chrom']), row['el']
        if row['tsd'] is not None:
            want.append((k, 'tsd', row['tsd'][1]))
        if b > a:
            want += [(k, 'head', (c, a, min(a + 2, b))), (k, 'tail', (c, max(b - 2, a), b))]
        f = min(range(6), key=lambda j: (-int(fr[k, j]['codons']), j))
        row['orf'] = (f // 3, f % 3, int(fr[k, f]['start']), int(fr[k, f]['end']), int(fr[k, f]['codons']), int(fr[k, f]['met'])) if int(fr[k, f]['codons']) else None
        row['ends'] = None
    ends = {}
    for (k, what, _), text in zip(want, genome_letters(A, [w[2] for w in want])):
        if what == 'tsd':
            rows[k]['tsd'][1] = text
        else:
            ends[(k, what)] = text
    for k, row in enumerate(rows):
        if (k, 'head') in ends:
            row['ends'] = ends[(k, 'head')] + '..' + ends[(k, 'tail')]
    return formats.element_lines(regions, names_sorted, prefix, rows, min_orf, header=header)


def family_block(A, kept_paths, select, regions, prefix, cover, suffix, header):
    """--families for one block of GFF3 rows: the rows `select` (a mask) of the kept rows' (records, first, blocks) joined with
    `regions` (formats.region_items, without the trivial self rows), one engine.link_regions call (kernel K12), the lines of
    formats.family_lines."""
    _, names_sorted, _, family, links = linked_regions(A, kept_paths, select, regions, cover)
    return formats.family_lines(regions, names_sorted, prefix, family, links, suffix=suffix, header=header)


def linked_regions(A, kept_paths, select, regions, cover):
    """What --families and --consensus share for one block of GFF3 rows: the rows `select` (a mask) of the kept rows' (records,
    first, blocks) joined with `regions` (formats.region_items, without the trivial self rows) and one engine.link_regions call
    (kernel K12).  Returns ((records, first, blocks) of the rows, the sorted names, the items, family, links)."""
    recs, first, blk = kept_paths
    rows = np.flatnonzero(select)
    f2, b2 = formats.select_paths(first, blk, rows)
    names_sorted = sorted(A.names, key=lambda s: s.encode())
    cid = {n: i for i, n in enumerate(names_sorted)}
    chrom_of_tid = [cid[n] for n in A.names]
    items, _ = formats.region_items(recs[rows], regions, chrom_of_tid, first=f2, blocks=b2, self_job=True)
    family, links = engine.link_regions(A, recs[rows], f2, b2, regions, chrom_of_tid, items, cover)
    return (recs[rows], f2, b2), names_sorted, items, family, links


CONSENSUS_BUDGET = 1 << 22   # columns asked of engine.pileup at once: 128 MiB of counts on the host


def family_piles(A, kept_paths, select, regions, cover):
    """What --consensus and --familyAlignments share for one block of GFF3 rows: the families exactly as family_block computes
    them (linked_regions), of every family the representative region (formats.family_representatives) as a window, and the
    items of those regions (formats.region_items, without the trivial self rows) as the piles, sorted by window.  Returns
    ((records, first, blocks) of the rows, the sorted names, reps, windows, items)."""
    paths, names_sorted, items, family, links = linked_regions(A, kept_paths, select, regions, cover)
    reps = formats.family_representatives(regions, family, links)
    tid_of = {n: i for i, n in enumerate(A.names)}
    rep = np.array([i for i, _ in reps], dtype=np.int64)
    windows = np.zeros(rep.size, dtype=engine._ffi.PILEUP_WINDOW)
    if rep.size:
        windows['tid'] = [tid_of[names_sorted[int(c)]] for c in regions['chrom'][rep]]
        windows['start'], windows['end'] = regions['start'][rep], regions['end'][rep]
    window_of = np.full(len(regions), -1, dtype=np.int64)
    window_of[rep] = np.arange(rep.size)
    its = items[window_of[items['group'].astype(np.int64)] >= 0] if items.size else items
    its = its.copy()
    its['group'] = window_of[its['group'].astype(np.int64)]
    its = its[np.argsort(its['group'], kind='stable')]
    return paths, names_sorted, reps, windows, its


def consensus_block(A, kept_paths, select, regions, prefix, cover, suffix, budget=CONSENSUS_BUDGET, insertions=False):
    """--consensus for one block of GFF3 rows: the families exactly as family_block computes them, of every family the
    representative region (formats.family_representatives) as a window, the items of those regions (formats.region_items,
    without the trivial self rows) as the pile (family_piles), engine.pileup (kernel K13) in runs of windows of at most `budget`
    columns (a longer window goes alone), the lines of formats.consensus_records.  The lines do not depend on the budget.  insertions
    (--consensusInsertions): per run of windows the sites in front of which most of the pile inserts something
    (formats.insertion_sites), one engine.insertions call (kernel K14) over the same windows and items — none for a run without a
    site — and its called bytes spliced into the records; a site where a run was longer than its columns is logged once, with
    its family."""
    (recs, f2, b2), names_sorted, reps, windows, its = family_piles(A, kept_paths, select, regions, cover)
    lines = []
    for g0, g1 in text_runs(windows['end'].astype(np.int64) - windows['start'], budget):
        run = its[np.searchsorted(its['group'], g0, side='left'):np.searchsorted(its['group'], g1, side='left')].copy()
        run['group'] -= g0
        cols, call = engine.pileup(A, None, recs, f2, b2, windows[g0:g1], run)
        ins = None
        if insertions:
            sites = formats.insertion_sites(windows[g0:g1], cols)
            ins = (sites, np.zeros(0, dtype=np.uint8))
            if sites.size:
                res, _, icall = engine.insertions(A, None, recs, f2, b2, windows[g0:g1], run, sites, counts=False)
                ins = (sites, icall)
                for s in np.flatnonzero(res['longer']).tolist():
                    logging.warning('--consensusInsertions: family F%d%s: an inserted run of %d bases in front of base %d of its representative is '
                                    'longer than the %d insertion columns of the site and was truncated',
                                    g0 + int(sites['window'][s]) + 1, suffix, int(res['max_len'][s]), int(sites['x'][s]), int(sites['ncols'][s]))
        lines += formats.consensus_records(regions, names_sorted, prefix, reps[g0:g1], cols, call, suffix=suffix, number=g0 + 1, insertions=ins)
    return lines


STACK_BUDGET = 1 << 26   # row bytes asked of engine.stack at once (one row goes whatever its size)


def pile_calls(A, recs, f2, b2, win, run):
    """What --familyAlignments and --copyDivergence / --landscape share for one run of windows `win` with the items `run` over
    them: engine.pileup (kernel K13) for the counts and the call, and once more without items for the representative's own
    letters; the sites (formats.stack_sites: every column in front of which a row inserts something, with as many columns as its
    longest run, which a first engine.insertions call over the sites reports); engine.insertions (kernel K14) for the call of the
    insertion columns.  Returns (own, call, sites, icall)."""
    cols, call = engine.pileup(A, None, recs, f2, b2, win, run)
    _, own = engine.pileup(A, None, recs, f2, b2, win, run[:0], counts=False)
    sites = formats.stack_sites(win, cols)
    icall = np.zeros(0, dtype=np.uint8)
    if sites.size:
        res, _, _ = engine.insertions(A, None, recs, f2, b2, win, run, sites, counts=False, call=False)
        sites = formats.stack_sites(win, cols, max_len=res['max_len'])
        _, _, icall = engine.insertions(A, None, recs, f2, b2, win, run, sites, results=False, counts=False)
    return own, call, sites, icall


def alignment_block(A, kept_paths, select, regions, prefix, cover, suffix, budget=CONSENSUS_BUDGET, stack_budget=STACK_BUDGET):
    """--familyAlignments for one block of GFF3 rows: the families, representatives, windows and piles of consensus_block
    (family_piles), and per run of windows of at most `budget` columns: engine.pileup (kernel K13) for the counts and the call,
    and once more without items for the representative's own letters; the sites (formats.stack_sites: every column in front of
    which a row inserts something, with as many columns as its longest run, which a first engine.insertions call over the
    sites reports); engine.insertions (kernel K14) for the call of the insertion columns; and engine.stack (kernel K15) for the
    rows, in runs of items of at most stack_budget bytes (one row goes whatever its size).  Returns the lines of
    formats.stockholm_blocks; they depend on neither budget.  A row with hidden bases (a run beyond the 1024 columns of a site)
    is logged once, with its family."""
    (recs, f2, b2), names_sorted, reps, windows, its = family_piles(A, kept_paths, select, regions, cover)
    lines = []
    for g0, g1 in text_runs(windows['end'].astype(np.int64) - windows['start'], budget):
        win = windows[g0:g1]
        run = its[np.searchsorted(its['group'], g0, side='left'):np.searchsorted(its['group'], g1, side='left')].copy()
        run['group'] -= g0
        own, call, sites, icall = pile_calls(A, recs, f2, b2, win, run)
        width = (win['end'].astype(np.int64) - win['start']) + np.bincount(sites['window'], weights=sites['ncols'], minlength=g1 - g0).astype(np.int64)
        rows = []
        for i0, i1 in text_runs(width[run['group'].astype(np.int64)] if run.size else np.zeros(0, dtype=np.int64), stack_budget):
            res, row_first, text = engine.stack(A, None, recs, f2, b2, win, run[i0:i1], sites)
            for k in np.flatnonzero(res['bases']).tolist():
                it, r = run[i0 + k], res[k]
                qid = int(recs['qid'][int(it['aln'])])
                name = formats.stockholm_row_name(A.names[qid], int(A.lengths[qid]), int(recs['qstrand'][int(it['aln'])]), int(r['q_lo']), int(r['q_hi']))
                rows.append((int(it['group']), name, text[int(row_first[k]):int(row_first[k + 1])]))
                if r['hidden']:
                    logging.warning('--familyAlignments: family F%d%s: row %s has %d inserted bases beyond the insertion columns of its sites; they are '
                                    'not shown', g0 + int(it['group']) + 1, suffix, name, int(r['hidden']))
        lines += formats.stockholm_blocks(regions, names_sorted, prefix, reps[g0:g1], sites, own, call, icall, rows, suffix=suffix, number=g0 + 1)
    return lines


def divergence_block(A, kept_paths, select, regions, prefix, cover, suffix, budget=CONSENSUS_BUDGET):
    """--copyDivergence and --landscape for one block of GFF3 rows: the families, representatives, windows and piles of
    consensus_block (family_piles), and per run of windows of at most `budget` columns the consensus exactly as alignment_block
    makes it (pile_calls: the call of every target column and of the insertion columns of every site), then one
    engine.call_stats call (kernel K16) over the run's items: every row of the pile against the consensus.  Returns the members
    of formats.copy_divergence_lines and formats.landscape_lines: per family the representative's own row
    (formats.own_call_stats) and one per item with bases, in the order of the items — the sequence rows of the family's
    Stockholm block.  They do not depend on the budget."""
    (recs, f2, b2), names_sorted, reps, windows, its = family_piles(A, kept_paths, select, regions, cover)
    members = []
    for g0, g1 in text_runs(windows['end'].astype(np.int64) - windows['start'], budget):
        win = windows[g0:g1]
        run = its[np.searchsorted(its['group'], g0, side='left'):np.searchsorted(its['group'], g1, side='left')].copy()
        run['group'] -= g0
        own, call, sites, icall = pile_calls(A, recs, f2, b2, win, run)
        stats = engine.call_stats(A, None, recs, f2, b2, win, run, sites, call, icall)
        mine = formats.own_call_stats(own, call, sites, icall, win)
        at = 0
        for g in range(g1 - g0):
            r = regions[reps[g0 + g][0]]
            family = 'F%d%s' % (g0 + g + 1, suffix)
            members.append((family, 'rep', names_sorted[int(r['chrom'])], int(r['start']), int(r['end']), '+', mine[g]))
            while at < run.size and int(run['group'][at]) == g:   # the items are sorted by window
                s, a = stats[at], int(run['aln'][at])
                at += 1
                if s['q_hi'] > s['q_lo']:
                    qid = int(recs['qid'][a])
                    members.append((family, 'copy', A.names[qid]) + formats.copy_stretch(int(A.lengths[qid]), int(recs['qstrand'][a]), int(s['q_lo']), int(s['q_hi'])) + (s,))
    return members


def self_repeats(A, pairs, outtab, outgff, minIdt=60, minLen=100, hspthresh=3000, minCov=3, intraCov=5,
                 splitSelf=False, reuseTab=False, label='Self_repeats', prefix=None, dist=None, source='mimeo-self',
                 B=None, anchor_rule='box', bound_extensions=False, paf=None, divergence=False, region_stats=None, maf=None, cs=False,
                 text_budget=TEXT_BUDGET, families=None, family_cover=80, consensus=None, consensus_budget=CONSENSUS_BUDGET,
                 consensus_insertions=False, family_alignments=None, stack_budget=STACK_BUDGET, copy_divergence=None, landscape=None,
                 terminal_repeats=None, terminal_window=1024, terminal_min_score=40, elements=None, tsd_min=4, tsd_max=20, tsd_slack=2, tsd_mismatch=0,
                 element_min_orf=300):
    """`mimeo self` (and, with B and source='mimeo', `mimeo x`).  paf: also write the rows of the TAB as PAF with their
    CIGARs to this file (--paf; nothing when the TAB is recycled); divergence: with paf, every PAF row also carries its
    divergence tags (--divergence; formats.divergence_tags).  anchor_rule: the gapped stage's skip rule, 'box' or
    'path' (or its _ffi.ANCHOR_* number; mimeo_hip.h MIMEO_ANCHOR_*).  bound_extensions: bound every gapped extension by
    the earlier alignments of its pair and strand (mimeo_params.bound_extensions); ValueError without the path rule.
    region_stats: also write, to this file, one line per GFF3 row with the column statistics of the alignment rows that overlap
    the region, clipped to it (--regionStats; formats.region_stat_lines, kernel K10).  The alignment call then asks for the
    paths, with or without paf; rank 0 holds the gathered paths and every rank the genomes, so no collective is added.  Nothing
    is written when the TAB is recycled (there are no paths).  maf: also write the rows of the TAB as MAF to this file (--maf;
    write_maf); cs: with paf, every PAF row also carries cs:Z: (--cs).  Both take the alignments' text from the engine (kernel
    K11) on rank 0, in runs of at most text_budget columns; like region_stats they ask the alignment call for the paths and add
    no collective, and nothing is written when the TAB is recycled.  families (`mimeo self` only: ValueError with B): also
    write, to this file, one line per GFF3 row with the repeat family of the region (--families; formats.family_lines, kernel
    K12): two regions are of one family when an alignment row that covers family_cover per cent of the one projects, through
    its path, onto family_cover per cent of the other (include/mimeo_hip.h "family linking v1").  Like region_stats it asks the
    alignment call for the paths, runs on rank 0 and adds no collective; with splitSelf the intra block is linked on its own
    and its families are named F1_intra ...; nothing is written when the TAB is recycled or a pair is listed twice.  consensus
    (`mimeo self` only: ValueError with B): also write, to this file, one FASTA record per repeat family with the family's
    consensus sequence (--consensus; consensus_block, formats.consensus_records, kernel K13): the families are computed exactly
    as for `families` (family_cover applies; `families` itself is not needed), every family's representative region is a window,
    the alignment rows over it are piled up per column in runs of at most consensus_budget columns, and a base is called from
    each column (include/mimeo_hip.h "pileup v1") — a repeat library for `mimeo filter` and `mimeo map`.  It asks the alignment
    call for the paths, runs on rank 0 and adds no collective; with splitSelf the intra block follows with F*_intra names;
    nothing is written when the TAB is recycled or a pair is listed twice.  consensus_insertions (with consensus: ValueError
    without it): where most of the rows over a representative insert something in front of a column, the inserted bases are piled
    up and called too (--consensusInsertions; kernel K14, include/mimeo_hip.h "pileup v2, insertion columns") and go into the
    record, so that a private deletion of the representative does not become the family's; on rank 0, no collective; every other
    output is unchanged.  family_alignments (`mimeo self` only: ValueError with B): also write, to this file, one Stockholm 1.0
    block per repeat family with the copies behind its consensus stacked in the representative's coordinates, the inserted
    columns opened up (--familyAlignments; alignment_block, formats.stockholm_blocks, kernel K15, include/mimeo_hip.h "pileup v3,
    the stack"): the families are those of `families` (family_cover applies; neither `families` nor `consensus` is needed), the
    rows are fetched from the engine in runs of at most stack_budget bytes; on rank 0, no collective; with splitSelf the intra
    block follows with F*_intra names; nothing is written when the TAB is recycled or a pair is listed twice; every other output
    is unchanged.  copy_divergence / landscape (`mimeo self` only: ValueError with B): also write, to these files, one line per
    family member with its column counts, divergence and Kimura distance against the family's consensus (--copyDivergence;
    formats.copy_divergence_lines) and the members binned by that distance and weighted by bases (--landscape;
    formats.landscape_lines): divergence_block, kernel K16, include/mimeo_hip.h "pileup v4, rows against the call".  The families
    are those of `families` (family_cover applies; none of `families`, `consensus`, `family_alignments` is needed); either works
    alone, and both share one computation; on rank 0, no collective; with splitSelf the intra block follows with F*_intra
    names; nothing is written when the TAB is recycled or a pair is listed twice; every other output is unchanged.
    terminal_repeats (`mimeo self` only: ValueError with B): also write, to this file, for every GFF3 row the repeats at its own
    two ends (--terminalRepeats; terminal_block, formats.terminal_repeat_lines, kernel K17, include/mimeo_hip.h "Terminal repeats
    of features"): the first terminal_window bases of the region against its last, direct (kind LTR) and inverted (kind TIR), a
    full affine-gap local alignment each, reported from a score of terminal_min_score on.  It needs the regions alone — none of
    paf, families or consensus, no paths, and it works with a recycled TAB; on rank 0, no collective; with splitSelf the intra
    block's lines follow; every other output is unchanged.  elements (`mimeo self` only: ValueError with B): also write, to this
    file, one structural line per GFF3 row (--elements; elements_block, formats.element_lines): the terminal repeats of K17
    (terminal_window and terminal_min_score apply; terminal_repeats need not be given, and where it is the block's K17 and K9
    calls are shared), the target-site duplication just outside them (kernel K18, include/mimeo_hip.h "Flank repeats": tsd_min ..
    tsd_max bases, either end free to move by tsd_slack bases, at most tsd_mismatch mismatches), which fixes the element's first
    and last base, the longest open reading frame inside the element (kernel K19) and a class, where an element is coding from
    element_min_orf codons on.  Like terminal_repeats it needs the regions alone; on rank 0, no collective; with splitSelf the
    intra block's lines follow; every other output is unchanged."""
    dist = dist or Dist()
    cs = cs and paf is not None
    if families is not None and B is not None:
        raise ValueError('families needs a self job: the regions and the queries must lie in one genome')
    if consensus is not None and B is not None:
        raise ValueError('consensus needs a self job: the regions and the queries must lie in one genome')
    if family_alignments is not None and B is not None:
        raise ValueError('family_alignments needs a self job: the regions and the queries must lie in one genome')
    if copy_divergence is not None and B is not None:
        raise ValueError('copy_divergence needs a self job: the regions and the queries must lie in one genome')
    if landscape is not None and B is not None:
        raise ValueError('landscape needs a self job: the regions and the queries must lie in one genome')
    if terminal_repeats is not None:
        if B is not None:
            raise ValueError('terminal_repeats needs a self job: the regions must lie in the genome that was aligned to itself')
        if not 1 <= int(terminal_window) <= 4096:
            raise ValueError('terminal_window must be in 1..4096, not %r' % (terminal_window,))
        if int(terminal_min_score) < 1:
            raise ValueError('terminal_min_score must be at least 1, not %r' % (terminal_min_score,))
    if elements is not None:
        if B is not None:
            raise ValueError('elements needs a self job: the regions must lie in the genome that was aligned to itself')
        if not 1 <= int(terminal_window) <= 4096:
            raise ValueError('terminal_window must be in 1..4096, not %r' % (terminal_window,))
        if int(terminal_min_score) < 1:
            raise ValueError('terminal_min_score must be at least 1, not %r' % (terminal_min_score,))
        if not 2 <= int(tsd_min) <= 32:
            raise ValueError('tsd_min must be in 2..32, not %r' % (tsd_min,))
        if not int(tsd_min) <= int(tsd_max) <= 32:
            raise ValueError('tsd_max must be in tsd_min..32, not %r' % (tsd_max,))
        if not 0 <= int(tsd_slack) <= 8:
            raise ValueError('tsd_slack must be in 0..8, not %r' % (tsd_slack,))
        if not 0 <= int(tsd_mismatch) <= 2:
            raise ValueError('tsd_mismatch must be in 0..2, not %r' % (tsd_mismatch,))
        if int(element_min_orf) < 1:
            raise ValueError('element_min_orf must be at least 1, not %r' % (element_min_orf,))
    if consensus_insertions and consensus is None:
        raise ValueError('consensus_insertions needs consensus: there is no library to insert into')
    if (families is not None or consensus is not None or family_alignments is not None or copy_divergence is not None or landscape is not None) and \
            not 1 <= int(family_cover) <= 100:
        raise ValueError('family_cover must be in 1..100, not %r' % (family_cover,))
    kept_paths = None
    outtab_intra = outtab + '_intra.tab'
    kept = None
    if not reuseTab or not os.path.isfile(outtab):
        params = gapped_params(hspthresh, anchor_rule, bound_extensions)
        blocks, _, kept, *more = align_blocks(A, B, pairs, params, minLen, minIdt, dist,
                                               paths=paf is not None or region_stats is not None or maf is not None or families is not None or consensus is not None
                                               or family_alignments is not None or copy_divergence is not None or landscape is not None,
                                               divergence=divergence and paf is not None, paf_rows=paf is not None)
        if region_stats is not None or families is not None or consensus is not None or family_alignments is not None or copy_divergence is not None or \
                landscape is not None:
            kept_paths = more[1]
        if paf is not None and dist.rank == 0:
            write_paf(paf, pairs, more[0], splitSelf=splitSelf and B is None, cs=(A, B, more[1], blocks, text_budget) if cs else None)
        if maf is not None and dist.rank == 0:
            write_maf(maf, A, B, pairs, blocks, more[1], splitSelf=splitSelf and B is None, budget=text_budget)
        if len(set(pairs)) != len(pairs):
            kept = None   # a pair listed twice is written twice (the reference would run it twice): read the file back instead
            kept_paths = None
        if dist.rank == 0:
            if splitSelf:
                write_tab(outtab, pairs, blocks, select=lambda pr: pr[0] != pr[1])
                write_tab(outtab_intra, pairs, blocks, select=lambda pr: pr[0] == pr[1])
            else:
                write_tab(outtab, pairs, blocks)
    elif maf is not None and dist.rank == 0:
        logging.warning('--maf needs the alignments\' paths: none with a recycled alignment file; %s is not written', maf)
    if dist.rank != 0:
        return None
    k_main = k_intra = None
    if kept is not None:   # the rows just written, split like the files
        intra = kept[:, 0] == kept[:, 1] if B is None else np.zeros(kept.shape[0], bool)
        k_main = kept[~intra][:, [0, 2, 3]] if splitSelf else kept[:, [0, 2, 3]]
        k_intra = kept[intra][:, [0, 2, 3]]
    reg_main, reg_intra = [], []
    lines = collapse_to_gff(outtab, A.names, A.lengths, minCov, minLen, source, str(label), str(prefix), kept=k_main, regions_out=reg_main)
    if splitSelf:
        if reuseTab and not os.path.isfile(outtab_intra) and os.path.isfile(outtab):
            logging.warning("Warning: Could not find intra-chrom results file: %s \nRe-run in '--strictSelf' "
                            "mode if required." % outtab_intra)
        else:
            # the reference restarts the ID counter with the same prefix (wrappers.py:1259-1264)
            lines += collapse_to_gff(outtab_intra, A.names, A.lengths, intraCov, minLen, source,
                                     str(label) + '_intra', str(prefix), kept=k_intra, regions_out=reg_intra)
    with open(outgff, 'w') as f:
        f.write(formats.GFF_HEADER + '\n')
        for line in lines:
            f.write(line + '\n')
    if region_stats is not None:
        if kept_paths is None:
            logging.warning('--regionStats needs the alignments\' paths: none with a recycled alignment file or a pair listed twice; %s is not written',
                            region_stats)
        else:
            # the regions of a block take their rows from the TAB the block was collapsed from
            none = np.zeros(0, dtype=engine._ffi.INTERVAL)
            split = splitSelf and B is None
            rl = region_stat_block(A, B, kept_paths, ~intra if split else np.ones(kept.shape[0], bool), reg_main[0] if reg_main else none, str(prefix), True)
            if split:   # the intra lines follow, with their restarted IDs, as in the GFF3
                rl += region_stat_block(A, B, kept_paths, intra, reg_intra[0] if reg_intra else none, str(prefix), False)
            with open(region_stats, 'w') as f:
                for line in rl:
                    f.write(line + '\n')
    if families is not None:
        if kept_paths is None:
            logging.warning('--families needs the alignments\' paths: none with a recycled alignment file or a pair listed twice; %s is not written',
                            families)
        else:
            none = np.zeros(0, dtype=engine._ffi.INTERVAL)
            fl = family_block(A, kept_paths, ~intra if splitSelf else np.ones(kept.shape[0], bool), reg_main[0] if reg_main else none, str(prefix),
                              int(family_cover), '', True)
            if splitSelf:   # the intra block is linked on its own; its lines follow, with their restarted IDs, as in the GFF3
                fl += family_block(A, kept_paths, intra, reg_intra[0] if reg_intra else none, str(prefix), int(family_cover), '_intra', False)
            with open(families, 'w') as f:
                for line in fl:
                    f.write(line + '\n')
    if consensus is not None:
        if kept_paths is None:
            logging.warning('--consensus needs the alignments\' paths: none with a recycled alignment file or a pair listed twice; %s is not written',
                            consensus)
        else:
            none = np.zeros(0, dtype=engine._ffi.INTERVAL)
            cl = consensus_block(A, kept_paths, ~intra if splitSelf else np.ones(kept.shape[0], bool), reg_main[0] if reg_main else none, str(prefix),
                                 int(family_cover), '', consensus_budget, bool(consensus_insertions))
            if splitSelf:   # the intra block's families follow, as in --families
                cl += consensus_block(A, kept_paths, intra, reg_intra[0] if reg_intra else none, str(prefix), int(family_cover), '_intra', consensus_budget,
                                      bool(consensus_insertions))
            with open(consensus, 'w') as f:
                for line in cl:
                    f.write(line + '\n')
    if family_alignments is not None:
        if kept_paths is None:
            logging.warning('--familyAlignments needs the alignments\' paths: none with a recycled alignment file or a pair listed twice; %s is not written',
                            family_alignments)
        else:
            none = np.zeros(0, dtype=engine._ffi.INTERVAL)
            al = alignment_block(A, kept_paths, ~intra if splitSelf else np.ones(kept.shape[0], bool), reg_main[0] if reg_main else none, str(prefix),
                                 int(family_cover), '', consensus_budget, stack_budget)
            if splitSelf:   # the intra block's families follow, as in --families
                al += alignment_block(A, kept_paths, intra, reg_intra[0] if reg_intra else none, str(prefix), int(family_cover), '_intra', consensus_budget,
                                      stack_budget)
            with open(family_alignments, 'w') as f:
                for line in al:
                    f.write(line + '\n')
    if copy_divergence is not None or landscape is not None:
        flags = [(copy_divergence, '--copyDivergence', formats.copy_divergence_lines), (landscape, '--landscape', formats.landscape_lines)]
        if kept_paths is None:
            for path, flag, _ in flags:
                if path is not None:
                    logging.warning('%s needs the alignments\' paths: none with a recycled alignment file or a pair listed twice; %s is not written', flag, path)
        else:
            none = np.zeros(0, dtype=engine._ffi.INTERVAL)
            members = divergence_block(A, kept_paths, ~intra if splitSelf else np.ones(kept.shape[0], bool), reg_main[0] if reg_main else none, str(prefix),
                                       int(family_cover), '', consensus_budget)
            if splitSelf:   # the intra block's families follow, as in --families
                members += divergence_block(A, kept_paths, intra, reg_intra[0] if reg_intra else none, str(prefix), int(family_cover), '_intra', consensus_budget)
            for path, _, make in flags:   # one computation for both files
                if path is not None:
                    with open(path, 'w') as f:
                        for line in make(members):
                            f.write(line + '\n')
    if terminal_repeats is not None or elements is not None:
        none = np.zeros(0, dtype=engine._ffi.INTERVAL)
        tsd = dict(min_len=int(tsd_min), max_len=int(tsd_max), slack=int(tsd_slack), max_mismatch=int(tsd_mismatch))
        tl, el = [], []
        # the intra lines follow, with their restarted IDs, as in the GFF3
        for regs, header in ((reg_main, True), (reg_intra, False)) if splitSelf else ((reg_main, True),):
            regs = regs[0] if regs else none
            calls = terminal_calls(A, regs, terminal_window, terminal_min_score) if elements is not None else None   # one K17 and one K9 call for both files
            if terminal_repeats is not None:
                tl += terminal_block(A, regs, str(prefix), terminal_window, terminal_min_score, header, calls=calls)
            if elements is not None:
                el += elements_block(A, regs, str(prefix), terminal_window, terminal_min_score, tsd, int(element_min_orf), header, calls=calls)
        for path, out in ((terminal_repeats, tl), (elements, el)):
            if path is not None:
                with open(path, 'w') as f:
                    for line in out:
                        f.write(line + '\n')
    return lines


def map_hits(A, B, pairs, outtab, minIdt=95, minLen=100, hspthresh=3000, reuseTab=False, dist=None, anchor_rule='box',
             bound_extensions=False, paf=None, divergence=False, maf=None, cs=False, text_budget=TEXT_BUDGET):
    """`mimeo map` alignment stage (wrappers.py:525-680): TAB only, no coverage collapse.  anchor_rule, bound_extensions,
    paf, divergence, maf, cs and text_budget as self_repeats."""
    dist = dist or Dist()
    if not reuseTab or not os.path.isfile(outtab):
        params = gapped_params(hspthresh, anchor_rule, bound_extensions)
        blocks, _, _, *more = align_blocks(A, B, pairs, params, minLen, minIdt, dist, paths=paf is not None or maf is not None,
                                            divergence=divergence and paf is not None, paf_rows=paf is not None)
        if dist.rank == 0:
            write_tab(outtab, pairs, blocks)
            if paf is not None:
                write_paf(paf, pairs, more[0], cs=(A, B, more[1], blocks, text_budget) if cs else None)
            if maf is not None:
                write_maf(maf, A, B, pairs, blocks, more[1], budget=text_budget)
    elif maf is not None and dist.rank == 0:
        logging.warning('--maf needs the alignments\' paths: none with a recycled alignment file; %s is not written', maf)


def trf_filter(rows, A, prefix=None, tmatch=2, tmismatch=7, tminscore=50, tmaxperiod=50, maxtandem=40, tdelta=7):
    """wrappers.py:120-262 trfFilter with the on-GPU tandem scorer (K8) in the place of TRF: the
    slice is seq[int(tStart):int(tEnd)] exactly as the reference cuts it (origin-one start used as
    a 0-based index, wrappers.py:190), a hit stays if masked/len*100 < maxtandem (:237-240), then
    the survivors are re-sorted and renumbered (:243-259).  tmatch / tmismatch / tdelta / tminscore /
    tmaxperiod are TRF's weights and thresholds; its detection statistics tPM / tPI have no counterpart."""
    cid = {n: i for i, n in enumerate(A.names)}
    iv = np.array([(cid[r[0]], int(r[2]), int(r[3])) for r in rows], dtype=np.uint32).reshape(-1, 3)
    masked = engine.tandem_masked(A, iv, tmatch, tmismatch, tminscore, tmaxperiod, tdelta)
    keep = []
    for r, m, (c, s, e) in zip(rows, masked.tolist(), iv.tolist()):
        ln = min(e, A.lengths[c]) - s
        if ln > 0 and m / ln * 100 < float(maxtandem):
            keep.append(r)
    return formats.renumber(keep, prefix)
