"""Host-side text stages of the mimeo hot path: what run_jobs.sh does with sed/awk/sort around the
lastz and bedtools calls.  Every function cites the reference command text it reproduces (paths
relative to /root/reference/src/mimeo); the engine (HIP) supplies the numbers, these functions
supply the bytes.
"""
import bisect
import math
import os
import re

import numpy as np

TAB_HEADER = '#name1\tstrand1\tstart1\tend1\tname2\tstrand2\tstart2+\tend2+\tscore\tidentity'  # wrappers.py:996
GFF_HEADER = '##gff-version 3\n#seqid\tsource\ttype\tstart\tend\tscore\tstrand\tphase\tattributes'  # wrappers.py:1153


def read_fasta(path, headers=None):
    """FASTA -> (ids, [uint8 arrays]).  id = first word of the header, like Biopython's rec.id
    used by the reference (utils.py:307, :549).  `headers` (a list) receives the full header lines
    (Biopython's rec.description: what SeqIO.write puts behind '>')."""
    names, seqs, cur = [], [], None
    with open(path, 'rb') as f:
        data = f.read()
    for block in data.split(b'>')[1:]:
        nl = block.find(b'\n')
        header = block if nl < 0 else block[:nl]
        body = b'' if nl < 0 else block[nl + 1:]
        names.append(header.split()[0].decode() if header.split() else '')
        if headers is not None:
            headers.append(header.rstrip(b'\r').decode())
        seqs.append(np.frombuffer(body.translate(None, b'\n\r \t'), dtype=np.uint8))
    return names, seqs


def read_fasta_dir(dirname):
    """All records of all files in a directory, like chromlens/get_all_pairs glob the split
    directory (utils.py:92-102, :529-531); files are visited in sorted order."""
    names, seqs = [], []
    for fn in sorted(os.listdir(dirname)):
        p = os.path.join(dirname, fn)
        if os.path.isfile(p):
            n, s = read_fasta(p)
            names += n
            seqs += s
    return names, seqs


def check_unique(names):
    """utils.py:300-306 / :472-499: duplicate sequence ids are fatal."""
    seen = set()
    for n in names:
        if n in seen:
            raise SystemExit('Non-unique name in genome: %s. Quitting.' % n)
        seen.add(n)


def chromlens(names, seqs, outfile=None):
    """utils.py:502-557: (id, str(len)) sorted by id; optional `id\\tlen` file (bedtools -g).
    `seqs`: sequences or plain lengths."""
    lens = sorted(((n, str(s if isinstance(s, int) else len(s))) for n, s in zip(names, seqs)), key=lambda x: x[0])
    if outfile:
        with open(outfile, 'w') as f:
            for n, l in lens:
                f.write(n + '\t' + l + '\n')
    return lens


def identity_pct(n, d):
    """lastz prints identity as `n/d` and `%.1f%%`; the reference strips the % (wrappers.py:1040)
    and compares the printed one-decimal value with minIdt (wrappers.py:1052)."""
    return '%.1f' % (100.0 * n / d) if d else '0.0'


def printed_tenths(id_n, id_d):
    """The digits of `'%.1f' % (100 n / d)` as an integer (80.0 -> 800), element-wise: lastz prints identity `%.1f%%`, the
    reference strips the % (wrappers.py:1040) and awk compares the PRINTED one-decimal value with minIdt (wrappers.py:1052):
    format first, compare the formatted number.  '%.1f' rounds the double's exact value half-even: floor(10 v + 1/2) away
    from a tie, Python's own formatting within 1e-6 of one (10 v carries a rounding error of its own there)."""
    idn, idd = np.asarray(id_n, dtype=np.float64), np.asarray(id_d, dtype=np.float64)
    with np.errstate(divide='ignore', invalid='ignore'):
        val = np.where(idd > 0, 100.0 * idn / idd, 0.0)
    x10 = val * 10.0
    fl = np.floor(x10)
    frac = x10 - fl
    tenths = (fl + (frac > 0.5)).astype(np.int64)
    for i in np.flatnonzero(np.abs(frac - 0.5) < 1e-6).tolist():
        tenths[i] = int(('%.1f' % val[i]).replace('.', ''))
    return tenths


def tab_blocks(alns, tnames, qnames, min_len, min_idt, rows=None):
    """Every pair's block of the 10-column TAB at once (wrappers.py:1043-1056, per pair:
    awk '0+$5 >= minLen' | awk '0+$13 >= minIdt {print $1,$2,$3,$4,$6,$7,$8,$9,$11,$13}' | sort -k 1,1 -k 3n,4n).
    `alns`: engine records of any number of (target, query) pairs; start1 and start2+ are origin-one (lastz general
    format), ends inclusive == half-open end.  Returns ({(tid, qid): [lines]}, kept) where `kept` is an (n, 4)
    int64 array of (tid, qid, start1, end1) of the rows written, in block order — what the BED projection of the
    file would read back (wrappers.py:1120-1128).  One pass over numpy columns instead of a Python loop per record:
    a C4 job has 6e5 alignments.  `rows` (a list, optional) receives one int64 array: the index into `alns` of every row
    written, in block order (the PAF writer pairs each TAB row with its path)."""
    if rows is not None:
        rows.append(np.zeros(0, dtype=np.int64))
    if alns.size == 0:
        return {}, np.zeros((0, 4), dtype=np.int64)
    ts, te = alns['tstart'].astype(np.int64), alns['tend'].astype(np.int64)
    tenths = printed_tenths(alns['id_n'], alns['id_d'])
    keep = (te - ts >= min_len) & (tenths >= int(min_idt) * 10 if float(min_idt) == int(min_idt) else tenths / 10.0 >= min_idt)   # length1 = end1 - start1 + 1 = te - ts
    idx = np.flatnonzero(keep)
    if idx.size == 0:
        return {}, np.zeros((0, 4), dtype=np.int64)
    tid, qid = alns['tid'].astype(np.int64)[idx], alns['qid'].astype(np.int64)[idx]
    pair = tid << 32 | qid
    order = np.lexsort((ts[idx], pair))          # name1 is constant inside a block: start1 numeric, then the whole line
    idx, tid, qid, pair = idx[order], tid[order], qid[order], pair[order]
    s1, e1 = ts[idx] + 1, te[idx]
    tn, qn = np.array(list(tnames), dtype=object)[tid].tolist(), np.array(list(qnames), dtype=object)[qid].tolist()
    sign = np.array(['+', '-'], dtype=object)[(alns['qstrand'][idx] != 0).astype(np.int64)].tolist()
    t10 = tenths[idx]
    lines = ['%s\t+\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d.%d' % r
             for r in zip(tn, s1.tolist(), e1.tolist(), qn, sign, (alns['qstart'].astype(np.int64)[idx] + 1).tolist(),
                          alns['qend'][idx].tolist(), alns['score'][idx].tolist(), (t10 // 10).tolist(), (t10 % 10).tolist())]
    # ties on (pair, start1) fall to sort's last-resort comparison of the whole line, byte by byte
    same = np.flatnonzero((pair[1:] == pair[:-1]) & (s1[1:] == s1[:-1]))
    if same.size:
        perm = np.arange(idx.size)
        run_start = same[np.r_[True, np.diff(same) > 1]]
        run_end = same[np.r_[np.diff(same) > 1, True]] + 2
        for a, b in zip(run_start.tolist(), run_end.tolist()):
            o = sorted(range(a, b), key=lambda k: lines[k].encode())
            lines[a:b] = [lines[k] for k in o]
            perm[a:b] = o
        idx, tid, qid, s1 = idx[perm], tid[perm], qid[perm], s1[perm]
    if rows is not None:
        rows[-1] = idx
    cuts = np.flatnonzero(np.diff(pair)) + 1
    blocks = {}
    for a, b in zip(np.r_[0, cuts].tolist(), np.r_[cuts, pair.size].tolist()):
        blocks[(int(tid[a]), int(qid[a]))] = lines[a:b]
    return blocks, np.stack([tid, qid, s1, te[idx]], axis=1)


def cigar(blocks):
    """The gap-free blocks (t, q, len) of ONE alignment (engine.align_units(..., paths=True)) as a CIGAR of M / I / D with the
    target as the reference, the SAM convention: M a block, I query bases absent from the target, D target bases absent from
    the query.  Where both sequences jump between two blocks (an insertion next to a deletion) the I comes first.  No = / X:
    those need the sequence text."""
    ops = []
    for k in range(len(blocks)):
        b = blocks[k]
        if k:
            p = blocks[k - 1]
            dq, dt = int(b['q']) - int(p['q']) - int(p['len']), int(b['t']) - int(p['t']) - int(p['len'])
            if dq:
                ops.append('%dI' % dq)
            if dt:
                ops.append('%dD' % dt)
        ops.append('%dM' % int(b['len']))
    return ''.join(ops)


def divergence_tags(s):
    """The divergence tags of one PAF row from its column statistics `s` (one row of engine.path_stats, or a mapping with the
    fields of _ffi.COLUMN_STATS), tab-separated.  With mism = transitions + transversions + ambiguous:
      NM:i:  mism + inserted + deleted bases (the edit distance of the alignment)
      de:f:  (mism + gap runs) / (matches + mism + gap runs): minimap2's gap-compressed divergence
      ts:i: / tv:i:  transitions and transversions
      kd:f:  Kimura's two-parameter distance -1/2 ln((1 - 2P - Q) sqrt(1 - 2Q)), P = ts / n, Q = tv / n over the
             n = matches + ts + tv unambiguous columns; left out where it is undefined (n == 0 or a factor <= 0: saturated)
    The counts are the engine's exact integers; the floating-point arithmetic is the host's."""
    mism, runs, de, kd = divergence_values(s)
    tags = ['NM:i:%d' % (mism + int(s['ins_bases']) + int(s['del_bases'])), 'de:f:%.4f' % (de if de is not None else 0.0),
            'ts:i:%d' % int(s['transitions']), 'tv:i:%d' % int(s['transversions'])]
    if kd is not None:
        tags.append('kd:f:%.4f' % kd)
    return '\t'.join(tags)


def divergence_values(s):
    """The floating-point arithmetic of divergence_tags and region_stat_lines on one row of column statistics (32- or 64-bit
    fields): (mism, gap runs, de, kd) with mism = transitions + transversions + ambiguous; de = (mism + runs) / (matches + mism +
    runs), None where there is no column and no run; kd = Kimura's two-parameter distance, None where it is undefined (no
    unambiguous column, or a factor <= 0: saturated)."""
    m, ts, tv, amb = int(s['matches']), int(s['transitions']), int(s['transversions']), int(s['ambiguous'])
    runs = int(s['ins_runs']) + int(s['del_runs'])
    mism = ts + tv + amb
    den = m + mism + runs
    de = (mism + runs) / den if den else None
    kd = None
    n = m + ts + tv
    if n:
        a, b = 1.0 - 2.0 * ts / n - tv / n, 1.0 - 2.0 * tv / n
        if a > 0.0 and b > 0.0:
            kd = 0.0 - 0.5 * math.log(a * math.sqrt(b))   # 0.0 - x: no '-0.0000' for identical sequences
    return mism, runs, de, kd


def select_paths(first, blocks, rows):
    """(first, blocks) of the alignments `rows` (indexes), in that order"""
    first = np.asarray(first, dtype=np.int64)
    rows = np.asarray(rows, dtype=np.int64)
    cnt = first[rows + 1] - first[rows] if rows.size else np.zeros(0, np.int64)
    out = np.zeros(rows.size + 1, dtype=np.uint64)
    out[1:] = np.cumsum(cnt)
    take = np.repeat(first[rows] - out[:-1].astype(np.int64), cnt) + np.arange(int(out[-1]), dtype=np.int64) if rows.size else np.zeros(0, np.int64)
    return out, blocks[take]


def path_columns(first, blocks):
    """Columns of every alignment's row (engine.path_text: row_first[i + 1] - row_first[i]) from the paths alone, as int64:
    (t_end - t_first) + (q_end - q_first) - sum of len; 0 without blocks."""
    first = np.asarray(first, dtype=np.int64)
    t, q, ln = blocks['t'].astype(np.int64), blocks['q'].astype(np.int64), blocks['len'].astype(np.int64)
    s = np.concatenate([np.zeros(1, np.int64), np.cumsum(ln)])
    out = np.zeros(first.size - 1, dtype=np.int64)
    some = np.flatnonzero(first[1:] > first[:-1])
    a, z = first[:-1][some], first[1:][some] - 1
    out[some] = (t[z] + ln[z] - t[a]) + (q[z] + ln[z] - q[a]) - (s[z + 1] - s[a])
    return out


MAF_HEADER = '##maf version=1 scoring=mimeo-amd'


def maf_lines(records, row_first, trow, qrow, first, blocks, tnames, tlens, qnames, qlens):
    """One MAF block per record, as one string of three lines (a file writes it and a newline, which is the empty line that
    ends a block):
      a score=<score>
      s <tname> <tstart> <tend - tstart> + <tlen> <trow>
      s <qname> <start> <qend - qstart> <+|-> <qlen> <qrow>
    Row i is trow[row_first[i]:row_first[i + 1]] over the same range of qrow (engine.path_text); the path of record i is
    blocks[first[i]:first[i + 1]].  The query start is on the aligned strand, MAF's own convention for a '-' row: the q of the
    path's first block, which is qlen - qend of the record (without blocks: qstart, or qlen - qend).  The letters are the
    engine's: upper case, N for everything that is not ACGT."""
    out = []
    for i in range(len(records)):
        r = records[i]
        t, q, minus = int(r['tid']), int(r['qid']), int(r['qstrand']) != 0
        a, z = int(row_first[i]), int(row_first[i + 1])
        if int(first[i + 1]) > int(first[i]):
            qs = int(blocks[int(first[i])]['q'])
        else:
            qs = int(qlens[q]) - int(r['qend']) if minus else int(r['qstart'])
        out.append('a score=%d\ns %s %d %d + %d %s\ns %s %d %d %s %d %s\n' % (
            int(r['score']), tnames[t], int(r['tstart']), int(r['tend']) - int(r['tstart']), int(tlens[t]), bytes(trow[a:z]).decode('ascii'),
            qnames[q], qs, int(r['qend']) - int(r['qstart']), '-' if minus else '+', int(qlens[q]), bytes(qrow[a:z]).decode('ascii')))
    return out


_ACGT = np.zeros(256, dtype=bool)
_ACGT[list(b'ACGT')] = True


def cs_tag(trow_i, qrow_i):
    """minimap2's short cs of ONE alignment from its two rows (engine.path_text), the target as the reference:
      :<n>    a maximal run of matches — columns of equal letters, both of ACGT (the matches of engine.path_stats)
      *<x><y> one column of any other aligned pair: target letter, query letter, lower case; 'n' is a letter here, so N over N
              is *nn and never part of a ':' run
      +<seq>  an insertion run (query bases absent from the target), -<seq> a deletion run, lower case
    The ':' lengths sum to id_n, and the tag walks the columns of cg:Z:.  A run-length encoding of four column classes: the work
    per column is numpy's."""
    t, q = np.asarray(trow_i, dtype=np.uint8), np.asarray(qrow_i, dtype=np.uint8)
    if t.size != q.size:
        raise ValueError('rows of %d and %d columns' % (t.size, q.size))
    if t.size == 0:
        return ''
    cls = np.ones(t.size, dtype=np.int8)               # 1: a mismatch, or a column with an N
    cls[(t == q) & _ACGT[t]] = 0                       # 0: match
    cls[t == 0x2D] = 2                                 # 2: insertion
    cls[q == 0x2D] = 3                                 # 3: deletion
    cut = np.flatnonzero(cls[1:] != cls[:-1]) + 1
    starts, ends = np.concatenate([[0], cut]), np.concatenate([cut, [t.size]])
    tl, ql = t | 0x20, q | 0x20                        # letters to lower case ('-' is in no run that prints it from its own row)
    out = []
    for a, z, c in zip(starts.tolist(), ends.tolist(), cls[starts].tolist()):
        if c == 0:
            out.append(':%d' % (z - a))
        elif c == 1:
            sub = np.empty((z - a, 3), dtype=np.uint8)
            sub[:, 0], sub[:, 1], sub[:, 2] = 0x2A, tl[a:z], ql[a:z]
            out.append(sub.tobytes().decode('ascii'))
        elif c == 2:
            out.append('+' + ql[a:z].tobytes().decode('ascii'))
        else:
            out.append('-' + tl[a:z].tobytes().decode('ascii'))
    return ''.join(out)


def cs_tags(row_first, trow, qrow):
    """cs_tag of every row of an engine.path_text result"""
    return [cs_tag(trow[int(row_first[i]):int(row_first[i + 1])], qrow[int(row_first[i]):int(row_first[i + 1])]) for i in range(len(row_first) - 1)]


def paf_lines(records, first, blocks, tnames, tlens, qnames, qlens, stats=None, cs=None):
    """One PAF row per record: query name, length, start, end (0-based half-open, query plus strand), strand, target name,
    length, start, end, residue matches (id_n), alignment length (id_d + gap bases), 255 (no mapping quality), then
    AS:i:<score> and cg:Z:<cigar>.  The path of record i is blocks[first[i]:first[i + 1]] (mimeo_hip.h,
    mimeo_align_units_paths): t on the target plus strand, q on the aligned strand, so the CIGAR of a '-' row runs along the
    target forward and the reverse-complemented query — PAF's own meaning.  stats (one row of engine.path_stats per record;
    --divergence): the tags of divergence_tags between AS:i: and cg:Z:.  cs (one cs_tag per record; --cs): cs:Z:<tag> follows
    cg:Z:, so that a row without it is a prefix of the row with it."""
    lines = []
    for i in range(len(records)):
        r = records[i]
        b = blocks[int(first[i]):int(first[i + 1])]
        gaps = (int(r['tend']) - int(r['tstart']) - int(r['id_d'])) + (int(r['qend']) - int(r['qstart']) - int(r['id_d']))
        t, q = int(r['tid']), int(r['qid'])
        lines.append('%s\t%d\t%d\t%d\t%s\t%s\t%d\t%d\t%d\t%d\t%d\t255\tAS:i:%d\t%scg:Z:%s' % (
            qnames[q], int(qlens[q]), int(r['qstart']), int(r['qend']), '-' if int(r['qstrand']) else '+', tnames[t], int(tlens[t]),
            int(r['tstart']), int(r['tend']), int(r['id_n']), int(r['id_d']) + gaps, int(r['score']),
            divergence_tags(stats[i]) + '\t' if stats is not None else '', cigar(b)) + ('\tcs:Z:' + cs[i] if cs is not None else ''))
    return lines


def tab_block(alns, tname, qname, min_len, min_idt):
    """One pair's block (records of ONE (target, query) pair): see tab_blocks."""
    if alns.size == 0:
        return []
    one = alns.copy()
    one['tid'], one['qid'] = 0, 0
    blocks, _ = tab_blocks(one, [tname], [qname], min_len, min_idt)
    return blocks.get((0, 0), [])


def parse_tab(path):
    """Read a 10-column TAB (ours, or imported from another aligner: README.md:329-347)."""
    rows = []
    with open(path) as f:
        for line in f:
            if not line.strip() or line.startswith('#'):
                continue
            rows.append(line.split())
    return rows


def _awk_num(s):
    m = re.match(r'\s*[-+]?(\d+\.?\d*([eE][-+]?\d+)?|\.\d+([eE][-+]?\d+)?)', s)
    return float(m.group(0)) if m else 0.0


def bed_intervals(tab_rows, chrom_ids):
    """wrappers.py:1120-1128: awk '{print $1,$3,$4}' — BED start is the origin-one start1,
    un-shifted.  Returns an (n,3) uint32 array of (chrom id, start, end);
    rows on unknown chromosomes are dropped (bedtools genomecov would reject them)."""
    out = []
    for f in tab_rows:
        c = chrom_ids.get(f[0])
        if c is None:
            continue
        s = int(f[2]) if f[2].isdigit() else int(_awk_num(f[2]))   # awk's numeric reading of the field; plain digits need no regex
        e = int(f[3]) if f[3].isdigit() else int(_awk_num(f[3]))
        if s < 0 or e < 0:
            continue
        out.append((c, s, e))
    return np.array(out, dtype=np.uint32).reshape(-1, 3)


def gff_repeat_lines(regions, names_sorted, source, label, prefix):
    """wrappers.py:1166-1177 (self, source 'mimeo-self') / :883-894 (x, source 'mimeo'): one
    row per region in (chrom, start) order, ID = prefix_%05d counting from 1."""
    lines = []
    for i, r in enumerate(regions, 1):
        lines.append('\t'.join([names_sorted[int(r['chrom'])], source, label, str(int(r['start'])), str(int(r['end'])),
                                '.', '+', '.', 'ID=%s_%05d' % (prefix, i)]))
    return lines


WINDOW_ITEM = np.dtype([(n, '<u4') for n in ('aln', 'group', 'w0', 'w1')])   # _ffi.WINDOW_ITEM (this module does not load the library)
REGION_STATS_FIELDS = ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_runs', 'ins_bases', 'del_runs', 'del_bases')
REGION_STATS_HEADER = '\t'.join(('#ID', 'seqid', 'start', 'end', 'rows', 'covered', 'columns') + REGION_STATS_FIELDS + ('identity', 'de', 'kd'))


def region_items(records, regions, chrom_of_tid, first=None, blocks=None, self_job=False):
    """The join of alignments and repeat regions for engine.window_stats: for every record and every region of its target
    scaffold with [tstart, tend) and [start, end) overlapping, one item (record number, region number, max(start, tstart),
    min(end, tend)).  records: engine records; regions: the _ffi.INTERVAL rows engine.coverage_collapse returns — sorted by
    (chrom, start) and disjoint; chrom_of_tid[tid]: the region chromosome number of target scaffold tid (the collapse numbers
    the scaffolds in sorted-name order, the engine in FASTA order).

    A region is the half-open interval [start, end) the collapse computed, the numbers printed in its GFF3 row; the record's
    side is its true 0-based tstart — NOT the origin-one start1 that the BED projection feeds to the collapse un-shifted
    (bed_intervals): the statistics are those of the alignment's columns that lie on the region's bases.

    self_job (with first, blocks: the records' paths): the trivial self rows are left out — same scaffold, plus strand, and a
    path of exactly one block with t == q, a sequence against itself.  They are all matches and would only dilute every region.
    Returns (items, rows): WINDOW_ITEM rows ordered by record, then region, and the number of items of every region."""
    nreg = len(regions)
    none = (np.zeros(0, dtype=WINDOW_ITEM), np.zeros(nreg, dtype=np.int64))
    if len(records) == 0 or nreg == 0:
        return none
    rec = np.arange(len(records), dtype=np.int64)
    if self_job:
        if first is None or blocks is None:
            raise ValueError('self_job needs the paths (first, blocks) to tell the trivial self rows')
        first = np.asarray(first, dtype=np.int64)
        one = first[1:] - first[:-1] == 1
        b = blocks[first[:-1][one]]
        on_diagonal = np.zeros(len(records), dtype=bool)
        on_diagonal[one] = b['t'] == b['q']
        trivial = on_diagonal & (records['tid'] == records['qid']) & (records['qstrand'] == 0)
        rec = rec[~trivial]
    chrom = np.asarray(chrom_of_tid, dtype=np.int64)[records['tid'][rec].astype(np.int64)]
    ts, te = records['tstart'][rec].astype(np.int64), records['tend'][rec].astype(np.int64)
    rc, rs, re_ = regions['chrom'].astype(np.int64), regions['start'].astype(np.int64), regions['end'].astype(np.int64)
    # one key orders (chrom, position); the regions are disjoint, so their ends are sorted like their starts
    lo = np.searchsorted(rc << 32 | re_, chrom << 32 | ts, side='right')   # the first region that ends behind tstart
    hi = np.searchsorted(rc << 32 | rs, chrom << 32 | te, side='left')     # one past the last region that starts in front of tend
    cnt = np.maximum(hi - lo, 0)
    total = int(cnt.sum())
    if total == 0:
        return none
    src = np.repeat(np.arange(rec.size), cnt)
    grp = np.repeat(lo - (np.cumsum(cnt) - cnt), cnt) + np.arange(total)
    w0, w1 = np.maximum(rs[grp], ts[src]), np.minimum(re_[grp], te[src])
    keep = w0 < w1   # a record without a base has no overlap
    items = np.zeros(int(keep.sum()), dtype=WINDOW_ITEM)
    items['aln'], items['group'], items['w0'], items['w1'] = rec[src][keep], grp[keep], w0[keep], w1[keep]
    return items, np.bincount(grp[keep], minlength=nreg).astype(np.int64)


def region_stat_lines(regions, names_sorted, prefix, stats, rows, header=True):
    """--regionStats: REGION_STATS_HEADER (header=True), then one tab-separated line per region.  ID, seqid, start and end are
    those of the region's GFF3 row (gff_repeat_lines); rows: the alignments that overlap the region (region_items); stats: its
    row of engine.window_stats; columns = matches + transitions + transversions + ambiguous; covered = columns + del_bases (the
    region's bases under an alignment, each counted once per alignment); identity = matches / columns; de and kd as in
    divergence_tags, over the region's sums.  A quantity that is undefined prints as '.'."""
    lines = [REGION_STATS_HEADER] if header else []
    for i, r in enumerate(regions, 1):
        s = stats[i - 1]
        c = [int(s[f]) for f in REGION_STATS_FIELDS]
        columns = c[0] + c[1] + c[2] + c[3]
        _, _, de, kd = divergence_values(s)
        lines.append('\t'.join([('%s_%05d' % (prefix, i)), names_sorted[int(r['chrom'])], str(int(r['start'])), str(int(r['end'])), str(int(rows[i - 1])),
                                str(columns + c[7]), str(columns)] + [str(v) for v in c] +
                               ['%.4f' % (c[0] / columns) if columns else '.', '%.4f' % de if de is not None else '.', '%.4f' % kd if kd is not None else '.']))
    return lines


TERMINAL_REPEATS_HEADER = '\t'.join(('#feature', 'seqid', 'start', 'end', 'kind', 'window', 'left_start', 'left_end', 'right_start', 'right_end', 'score',
                                     'columns', 'matches', 'ts', 'tv', 'ambiguous', 'gap_runs', 'gap_bases', 'identity', 'kd'))
TERMINAL_KINDS = ('LTR', 'TIR')   # by qstrand: a direct repeat, an inverted repeat


def terminal_repeat_lines(regions, names_sorted, prefix, window, records, stats, header=True):
    """--terminalRepeats: TERMINAL_REPEATS_HEADER (header=True), then one tab-separated line per orientation that was found, so
    0, 1 or 2 lines per region.  ID, seqid, start and end are those of the region's GFF3 row, as in region_stat_lines; records:
    the 2 n records of engine.terminal_repeats for the regions (2 k direct: kind LTR; 2 k + 1 inverted: kind TIR); stats: their
    rows of engine.path_stats.  window: the bases of each end that were examined, min(window, length // 2); left_* / right_*:
    the two repeats on the plus strand, in the region's own convention (tstart / tend and qstart / qend of the record); columns
    = matches + ts + tv + ambiguous; gap_runs / gap_bases: insertions and deletions together; identity = matches / columns and
    kd (Kimura's two-parameter distance between the two repeats, which dates the insertion of an LTR element) as in
    region_stat_lines, '.' where undefined."""
    lines = [TERMINAL_REPEATS_HEADER] if header else []
    for i, r in enumerate(regions, 1):
        w = min(int(window), (int(r['end']) - int(r['start'])) // 2)
        for o in (0, 1):
            a, s = records[2 * (i - 1) + o], stats[2 * (i - 1) + o]
            if int(a['id_d']) == 0:
                continue   # nothing found in this orientation
            c = [int(s[f]) for f in ('matches', 'transitions', 'transversions', 'ambiguous')]
            columns = sum(c)
            _, runs, _, kd = divergence_values(s)
            lines.append('\t'.join(['%s_%05d' % (prefix, i), names_sorted[int(r['chrom'])], str(int(r['start'])), str(int(r['end'])), TERMINAL_KINDS[o], str(w),
                                    str(int(a['tstart'])), str(int(a['tend'])), str(int(a['qstart'])), str(int(a['qend'])), str(int(a['score'])), str(columns)] +
                                   [str(v) for v in c] + [str(runs), str(int(s['ins_bases']) + int(s['del_bases'])),
                                                          '%.4f' % (c[0] / columns) if columns else '.', '%.4f' % kd if kd is not None else '.']))
    return lines


ELEMENTS_HEADER = '\t'.join(('#feature', 'seqid', 'start', 'end', 'kind', 'el_start', 'el_end', 'left_len', 'right_len', 'tr_score', 'tr_identity', 'tr_kd',
                             'tsd_len', 'tsd', 'tsd_mismatches', 'tsd_shift', 'ends', 'orf_strand', 'orf_frame', 'orf_start', 'orf_end', 'orf_codons',
                             'orf_met_codons', 'class'))
MITE_MAX_LEN = 800   # a non-coding TIR element with a duplication is a MITE up to this length, DNA_nonautonomous beyond it


def element_class(kind, has_tsd, coding, length):
    """the class column of --elements: the first rule that applies"""
    if kind == 'LTR':
        return ('LTR_retrotransposon' if coding else 'LTR_nonautonomous') if has_tsd else 'LTR_candidate'
    if kind == 'TIR':
        if not has_tsd:
            return 'TIR_candidate'
        return 'DNA_transposon' if coding else 'MITE' if length <= MITE_MAX_LEN else 'DNA_nonautonomous'
    return 'coding_repeat' if coding else '.'


def element_lines(regions, names_sorted, prefix, rows, min_orf=300, header=True):
    """--elements: ELEMENTS_HEADER (header=True), then one tab-separated line per region, in the order of the GFF3 rows.  ID,
    seqid, start and end are those of the region's GFF3 row, as in terminal_repeat_lines.  rows: per region a dict (what
    workflow.elements_block puts together from kernels K17, K9, K18 and K19) with
      kind      'LTR', 'TIR' or None: the orientation of the terminal repeats that was chosen; with a kind also left_len,
                right_len (bases of the two repeats), score and stats (the record's row of engine.path_stats: tr_identity =
                matches / columns, tr_kd Kimura's distance as in terminal_repeat_lines)
      el        (el_start, el_end): the element, the feature itself where there is no kind
      tsd       None or (len, letters of the left copy, mismatches, dl, dr); tsd_shift prints dl,dr
      ends      the element's first two and last two bases as TG..CA, None for an empty element
      orf       None or (strand 0 / 1, frame 0 .. 2, start, end, codons, met): the best of the six frames — most codons, then
                the plus strand, then the lower frame; orf_frame prints 1 .. 3 and orf_met_codons codons - met, the codons
                from the run's first ATG on (0: none)
    class: element_class, where coding means orf_codons >= min_orf.  A value that is undefined prints as '.'."""
    lines = [ELEMENTS_HEADER] if header else []
    for i, (r, w) in enumerate(zip(regions, rows), 1):
        kind, tsd, orf, (el0, el1) = w['kind'], w['tsd'], w['orf'], w['el']
        tr = ['.'] * 5
        if kind is not None:
            s = w['stats']
            columns = sum(int(s[f]) for f in ('matches', 'transitions', 'transversions', 'ambiguous'))
            kd = divergence_values(s)[3]
            tr = [str(int(w['left_len'])), str(int(w['right_len'])), str(int(w['score'])), '%.4f' % (int(s['matches']) / columns) if columns else '.',
                  '%.4f' % kd if kd is not None else '.']
        td = ['.'] * 4 if tsd is None else [str(int(tsd[0])), tsd[1], str(int(tsd[2])), '%d,%d' % (tsd[3], tsd[4])]
        of = ['.'] * 6 if orf is None else ['+-'[orf[0]], str(orf[1] + 1), str(orf[2]), str(orf[3]), str(orf[4]), str(orf[4] - orf[5])]
        cls = element_class(kind, tsd is not None, orf is not None and orf[4] >= int(min_orf), el1 - el0)
        lines.append('\t'.join(['%s_%05d' % (prefix, i), names_sorted[int(r['chrom'])], str(int(r['start'])), str(int(r['end'])), kind or '.', str(el0), str(el1)] +
                               tr + td + [w['ends'] or '.'] + of + [cls]))
    return lines


FAMILY_HEADER = '\t'.join(('#ID', 'seqid', 'start', 'end', 'family', 'members', 'family_bases', 'links'))


def family_lines(regions, names_sorted, prefix, family, links, suffix='', header=True):
    """--families: FAMILY_HEADER (header=True), then one tab-separated line per region, in the order of the GFF3 rows.  ID,
    seqid, start and end are those of the region's GFF3 row (gff_repeat_lines), as in region_stat_lines; family / links: what
    engine.link_regions returned for the regions.  The families are named F1, F2, ... (+ suffix: the second block of
    --strictSelf) in the order of their first member, a region that is linked to no other being a family of one; members and
    family_bases are the number of regions of the family and their summed length; links is the region's own count."""
    lines = [FAMILY_HEADER] if header else []
    fam = [int(f) for f in family]
    name, members, bases = {}, {}, {}
    for r, f in zip(regions, fam):
        if f not in name:
            name[f] = 'F%d%s' % (len(name) + 1, suffix)
        members[f] = members.get(f, 0) + 1
        bases[f] = bases.get(f, 0) + int(r['end']) - int(r['start'])
    for i, (r, f) in enumerate(zip(regions, fam), 1):
        lines.append('\t'.join(['%s_%05d' % (prefix, i), names_sorted[int(r['chrom'])], str(int(r['start'])), str(int(r['end'])), name[f],
                                str(members[f]), str(bases[f]), str(int(links[i - 1]))]))
    return lines


def family_representatives(regions, family, links):
    """The region that stands for each family in --consensus: the member with the most links (the copy that the most alignments
    tie to the others), among those the longest, among those the first.  family / links: what engine.link_regions returned.
    Returns one (region number, members) per family, in the order of family_lines' names F1, F2, ... (that of the families'
    first members); a family of one is represented by its only member."""
    order, best, members = [], {}, {}
    for i, (r, f) in enumerate(zip(regions, (int(f) for f in family))):
        key = (int(links[i]), int(r['end']) - int(r['start']))
        if f not in best:
            order.append(f)
            best[f] = (key, i)
        elif key > best[f][0]:   # strictly: an equal later member does not replace an earlier one
            best[f] = (key, i)
        members[f] = members.get(f, 0) + 1
    return [(best[f][1], members[f]) for f in order]


PILEUP_DEPTH_FIELDS = ('a', 'c', 'g', 't', 'n', 'del')
CONSENSUS_WIDTH = 60


INSERT_SITE = np.dtype([(n, '<u4') for n in ('window', 'x', 'ncols', 'voters')])   # _ffi.INSERT_SITE (this module does not load the library)
INSERT_MAX_COLS = 1024   # _ffi.INSERT_MAX_COLS


def _pileup_depth(c):
    """a + c + g + t + n + del of _ffi.PILEUP_COLUMN rows, in 64 bits: the alignment rows over every column"""
    return sum(c[f].astype(np.int64) for f in PILEUP_DEPTH_FIELDS) if len(c) else np.zeros(0, dtype=np.int64)


def _ins_site_mask(c, depth):
    """The ins_sites rule: the columns in front of which most of the pile inserts something, 2 * ins_runs > depth + 1 (the own
    copy, which inserts nothing, counted in).  The one statement of it: the header's ins_sites= and insertion_sites share it."""
    return 2 * c['ins_runs'].astype(np.int64) > depth + 1


def insertion_sites(windows, cols):
    """The sites of engine.insertions (kernel K14) from what engine.pileup returned for a run of windows: _ffi.INSERT_SITE rows,
    one per column that the ins_sites rule picks (_ins_site_mask), in the order of the columns — strictly increasing by (window,
    x).  windows: the _ffi.PILEUP_WINDOW rows of the pileup call; cols: its columns.  Per site window is the window's number in
    the run, x the target base, voters = depth + 1 (the region's own copy votes), and ncols = min(ins_bases - ins_runs + 1,
    _ffi.INSERT_MAX_COLS): each run has at least one base, so this bounds the longest run and no second ask is needed."""
    win = np.asarray(windows)
    n = win['end'].astype(np.int64) - win['start'].astype(np.int64)
    depth = _pileup_depth(cols)
    at = np.flatnonzero(_ins_site_mask(cols, depth)) if len(cols) else np.zeros(0, dtype=np.int64)
    col_first = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    g = np.searchsorted(col_first, at, side='right') - 1   # an empty window has no column: 'right' steps over it
    sites = np.zeros(at.size, dtype=INSERT_SITE)
    if at.size:
        sites['window'] = g
        sites['x'] = win['start'].astype(np.int64)[g] + (at - col_first[g])
        sites['ncols'] = np.minimum(cols['ins_bases'].astype(np.int64)[at] - cols['ins_runs'].astype(np.int64)[at] + 1, INSERT_MAX_COLS)
        sites['voters'] = np.minimum(depth[at] + 1, 0xFFFFFFFF)
    return sites


def consensus_records(regions, names_sorted, prefix, reps, cols, call, suffix='', number=1, insertions=None):
    """--consensus: one FASTA record per family, in the order of family_lines' names.  reps: family_representatives; cols / call:
    what engine.pileup returned for the representatives' regions as windows, in the order of reps (window k starts at the summed
    length of the windows before it).  The sequence is the call bytes of the representative's window with '-' removed (a column
    where deletions outnumber every base is not part of the family), CONSENSUS_WIDTH letters per line.  The header is
    >F3 rep=<ID> <seqid>:<start>-<end> members=<m> length=<len> mean_depth=<%.2f> ins_sites=<k>: ID, seqid, start and end those of
    the representative's GFF3 row, length that of the sequence, mean_depth the mean of a + c + g + t + n + del over the window
    (the alignment rows per base; the region's own copy is not counted), ins_sites the number of columns in front of which most
    of the pile inserts something: 2 * ins_runs > a + c + g + t + n + del + 1 (the own copy, which inserts nothing, counted
    in).  pileup v1 inserts nothing into the call; ins_sites says how often that matters.  number: that of the first family of
    reps (a caller that works the families off in runs).  insertions (--consensusInsertions; None: every line as without it):
    (sites, icall) — the sites formats.insertion_sites picked for these windows (window numbers those of reps) and the bytes
    engine.insertions called for their columns (kernel K14, "pileup v2"); the sequence of a window is then, for each column x in
    order, the icall bytes of the site in front of x without '-' (where there is a site) followed by call[x] without '-', and
    the header gains inserted=<bases>, the letters that came from icall, after ins_sites.  Returns the lines."""
    lines, at = [], 0
    if insertions is not None:
        sites, icall = insertions
        icall = np.asarray(icall, dtype=np.uint8)
        icol_first = np.concatenate([[0], np.cumsum(sites['ncols'].astype(np.int64))]).astype(np.int64)
    for k, (i, members) in enumerate(reps, number):
        r = regions[i]
        n = int(r['end']) - int(r['start'])
        c = cols[at:at + n]
        depth = _pileup_depth(c)
        letters = np.asarray(call[at:at + n], dtype=np.uint8)
        at += n
        more = ''
        if insertions is not None:
            s0, s1 = (int(v) for v in np.searchsorted(sites['window'], [k - number, k - number + 1], side='left'))
            ins = icall[int(icol_first[s0]):int(icol_first[s1])]
            # every byte of a site goes in front of column x - start: np.insert keeps the order of equal positions
            where = np.repeat(sites['x'][s0:s1].astype(np.int64) - int(r['start']), sites['ncols'][s0:s1].astype(np.int64))
            letters = np.insert(letters, where, ins)
            more = ' inserted=%d' % int((ins != ord('-')).sum())
        seq = letters.tobytes().replace(b'-', b'').decode('ascii')
        lines.append('>F%d%s rep=%s_%05d %s:%d-%d members=%d length=%d mean_depth=%.2f ins_sites=%d%s' % (
            k, suffix, prefix, i + 1, names_sorted[int(r['chrom'])], int(r['start']), int(r['end']), members, len(seq),
            float(depth.sum()) / n if n else 0.0, int(_ins_site_mask(c, depth).sum()) if n else 0, more))
        lines.extend(seq[j:j + CONSENSUS_WIDTH] for j in range(0, len(seq), CONSENSUS_WIDTH))
    return lines


def stack_sites(windows, cols, max_len=None):
    """The sites of engine.stack (kernel K15) for --familyAlignments from what engine.pileup returned for a run of windows:
    _ffi.INSERT_SITE rows, one per column in front of which ANY row of the pile inserts something (ins_runs > 0, not only the
    majority sites of insertion_sites), in the order of the columns.  voters = depth + 1 as in insertion_sites.  max_len: per
    site the longest run (mimeo_insert_result.max_len of an engine.insertions call over these sites): ncols = min(max_len,
    _ffi.INSERT_MAX_COLS), so that no insertion column is empty; None: ncols = 1, the sites of that first call."""
    win = np.asarray(windows)
    n = win['end'].astype(np.int64) - win['start'].astype(np.int64)
    at = np.flatnonzero(cols['ins_runs'] > 0) if len(cols) else np.zeros(0, dtype=np.int64)
    col_first = np.concatenate([[0], np.cumsum(n)]).astype(np.int64)
    g = np.searchsorted(col_first, at, side='right') - 1   # an empty window has no column: 'right' steps over it
    sites = np.zeros(at.size, dtype=INSERT_SITE)
    if at.size:
        sites['window'] = g
        sites['x'] = win['start'].astype(np.int64)[g] + (at - col_first[g])
        sites['ncols'] = 1 if max_len is None else np.clip(np.asarray(max_len, dtype=np.int64), 1, INSERT_MAX_COLS)
        sites['voters'] = np.minimum(_pileup_depth(cols)[at] + 1, 0xFFFFFFFF)
    return sites


def stockholm_row_name(qname, qlen, qstrand, q_lo, q_hi):
    """<qname>/<s>-<e> of a row of stockholm_blocks: the stretch [q_lo, q_hi) of the aligned strand (engine.stack's res) on the
    query's plus strand, 1-based inclusive; for a minus-strand row s > e, the Pfam / Rfam convention."""
    if qstrand:
        return '%s/%d-%d' % (qname, qlen - q_lo, qlen - q_hi + 1)
    return '%s/%d-%d' % (qname, q_lo + 1, q_hi)


def stockholm_blocks(regions, names_sorted, prefix, reps, sites, own, call, icall, rows, suffix='', number=1):
    """--familyAlignments: one Stockholm 1.0 block per family, in the order of family_lines' names — the copies behind a
    consensus record as one alignment in the representative's coordinates.  reps: family_representatives, whose regions are the
    windows 0, 1, ... of this run; sites: the _ffi.INSERT_SITE rows of these windows (stack_sites: window numbers those of
    reps), whose ncols insertion columns stand directly in front of the column of their base x; own: the representative's own
    letters and call: the consensus byte (engine.pileup) per target column of the windows, one behind the other; icall: the
    consensus byte per insertion column of the sites (engine.insertions); rows: per sequence row (window number, name, text) in
    the order of the file, text the W bytes of engine.stack's row and name stockholm_row_name's.  A block is
        # STOCKHOLM 1.0
        #=GF ID F3
        #=GF DE rep=<ID> <seqid>:<start>-<end> members=<m> rows=<r> columns=<W>
        <seqid>/<start+1>-<end> <the representative's own row: its letters, '.' at insertion columns>
        <name> <text>                 one per row of the window
        #=GC RF <x at target columns, . at insertion columns>
        #=GC cons <call at target columns; icall at insertion columns, its '-' written '.'>
        //
    rows= counts the sequence lines, the representative's own among them; a name that repeats inside a block gets .2, .3, ...
    in order.  With '.' and '-' removed the cons line is the record of consensus_records with insertions for the same family.
    number: that of the first family of reps.  Returns the lines."""
    lines, at = [], 0
    icall = np.asarray(icall, dtype=np.uint8)
    icol_first = np.concatenate([[0], np.cumsum(sites['ncols'].astype(np.int64))]).astype(np.int64)
    by_window = {}
    for g, name, text in rows:
        by_window.setdefault(int(g), []).append((name, text))
    for k, (i, members) in enumerate(reps, number):
        r = regions[i]
        n = int(r['end']) - int(r['start'])
        s0, s1 = (int(v) for v in np.searchsorted(sites['window'], [k - number, k - number + 1], side='left'))
        ins = icall[int(icol_first[s0]):int(icol_first[s1])]
        # every column of a site goes in front of column x - start: np.insert keeps the order of equal positions
        where = np.repeat(sites['x'][s0:s1].astype(np.int64) - int(r['start']), sites['ncols'][s0:s1].astype(np.int64))
        dots = np.full(ins.size, ord('.'), dtype=np.uint8)
        open_up = lambda target, inserted: np.insert(np.asarray(target, dtype=np.uint8), where, inserted).tobytes().decode('ascii')
        seqid = names_sorted[int(r['chrom'])]
        mine = by_window.get(k - number, [])
        seq = [('%s/%d-%d' % (seqid, int(r['start']) + 1, int(r['end'])), open_up(own[at:at + n], dots))]
        seq += [(name, bytes(text).decode('ascii')) for name, text in mine]
        width = n + ins.size
        lines += ['# STOCKHOLM 1.0', '#=GF ID F%d%s' % (k, suffix),
                  '#=GF DE rep=%s_%05d %s:%d-%d members=%d rows=%d columns=%d' % (prefix, i + 1, seqid, int(r['start']), int(r['end']), members, len(seq), width)]
        seen = {}
        for name, text in seq:
            if len(text) != width:
                raise ValueError('row %s has %d bytes for a block of %d columns' % (name, len(text), width))
            seen[name] = seen.get(name, 0) + 1
            lines.append('%s %s' % (name if seen[name] == 1 else '%s.%d' % (name, seen[name]), text))
        lines.append('#=GC RF ' + open_up(np.full(n, ord('x'), dtype=np.uint8), dots))
        lines.append('#=GC cons ' + open_up(call[at:at + n], np.where(ins == ord('-'), ord('.'), ins).astype(np.uint8)))
        lines.append('//')
        at += n
    return lines


CALL_STATS = np.dtype([(n, '<u4') for n in ('matches', 'transitions', 'transversions', 'ambiguous', 'ins_bases', 'del_bases', 'q_lo',
                                             'q_hi')])   # _ffi.CALL_STATS (this module does not load the library)
COPY_DIVERGENCE_HEADER = '\t'.join(('#family', 'role', 'seqid', 'start', 'end', 'strand') + CALL_STATS.names[:6] + ('div', 'kd'))
LANDSCAPE_HEADER = '\t'.join(('#family', 'kd_lo', 'kd_hi', 'copies', 'bases'))
LANDSCAPE_BINS = 50   # bins of 0.01 from 0 up to 0.50; then one for everything from 0.50 on and one for the saturated copies
_LANDSCAPE_EDGES = [k / 100 for k in range(LANDSCAPE_BINS + 1)]   # k / 100 is the double of the decimal: 0.07 falls into [0.07, 0.08)
_CODE = np.full(256, 4, dtype=np.uint8)   # A C G T: 0 .. 3, a transition flips bit 1; everything else 4
_CODE[list(b'ACGT')] = (0, 1, 2, 3)


def own_call_stats(own, call, sites, icall, windows):
    """The representative's own row of --copyDivergence for a run of windows, as engine.call_stats (kernel K16) would count a row
    that lies under every target column and inserts nothing: one CALL_STATS row per window.  own: the representative's own
    letters and call: the consensus byte per target column of the windows, one behind the other (engine.pileup without and with
    items); sites / icall: the _ffi.INSERT_SITE rows of these windows and the consensus byte per insertion column.  Per target
    column with c = call and y = own: c == '-' is an ins_bases; otherwise the pair is ambiguous where either is N, a match where
    they are equal, a transition for A<->G and C<->T and a transversion otherwise.  Every letter column of the window's sites is a
    del_bases.  [q_lo, q_hi) is the window itself."""
    win = np.asarray(windows)
    own, call, icall = (np.asarray(x, dtype=np.uint8) for x in (own, call, icall))
    out = np.zeros(win.size, dtype=CALL_STATS)
    icol_first = np.concatenate([[0], np.cumsum(sites['ncols'].astype(np.int64))]).astype(np.int64)
    at = 0
    for g in range(win.size):
        n = int(win['end'][g]) - int(win['start'][g])
        c, y = call[at:at + n], _CODE[own[at:at + n]]
        at += n
        letter = c != ord('-')
        cc = _CODE[c]
        amb = letter & ((cc == 4) | (y == 4))
        d = cc ^ y
        s0, s1 = (int(v) for v in np.searchsorted(sites['window'], [g, g + 1], side='left'))
        out[g] = (int((letter & ~amb & (d == 0)).sum()), int((letter & ~amb & (d == 2)).sum()), int((letter & ~amb & (d != 0) & (d != 2)).sum()),
                  int(amb.sum()), int((~letter).sum()), int((icall[int(icol_first[s0]):int(icol_first[s1])] != ord('-')).sum()),
                  int(win['start'][g]), int(win['end'][g]))
    return out


def copy_stretch(qlen, qstrand, q_lo, q_hi):
    """(start, end, strand) of a copy on its scaffold's plus strand, 0-based half-open, from the stretch [q_lo, q_hi) of the aligned
    strand (engine.call_stats, engine.stack): the bases that stockholm_row_name names 1-based."""
    return (qlen - q_hi, qlen - q_lo, '-') if qstrand else (q_lo, q_hi, '+')


def _copy_values(s):
    """(div, kd) of one CALL_STATS row: div = (ts + tv) / (m + ts + tv), None without an unambiguous column; kd = Kimura's
    distance as divergence_values computes it, None where it is undefined."""
    m, ts, tv = int(s['matches']), int(s['transitions']), int(s['transversions'])
    kd = divergence_values({'matches': m, 'transitions': ts, 'transversions': tv, 'ambiguous': int(s['ambiguous']), 'ins_runs': 0, 'del_runs': 0})[3]
    return ((ts + tv) / (m + ts + tv) if m + ts + tv else None), kd


def copy_divergence_lines(members, header=True):
    """--copyDivergence: one line per family member with bases — how far the copy is from its family's consensus.  members: per
    line (family name, role 'rep' or 'copy', seqid, start, end, strand, a CALL_STATS row), in the order of the file
    (workflow.divergence_block); start / end the copy's stretch on the plus strand, 0-based half-open.  The columns are
    COPY_DIVERGENCE_HEADER's: the six counts of the row against the consensus (engine.call_stats, kernel K16; own_call_stats for
    the representative), div = (transitions + transversions) / (matches + transitions + transversions) and kd = Kimura's
    two-parameter distance over the same columns, both %.4f, NA where undefined (no unambiguous column; kd also where saturated)."""
    lines = [COPY_DIVERGENCE_HEADER] if header else []
    for family, role, seqid, start, end, strand, s in members:
        div, kd = _copy_values(s)
        lines.append('\t'.join([family, role, seqid, str(int(start)), str(int(end)), strand] + [str(int(s[f])) for f in CALL_STATS.names[:6]] +
                               ['%.4f' % div if div is not None else 'NA', '%.4f' % kd if kd is not None else 'NA']))
    return lines


def landscape_bin(kd):
    """The bin of a copy in the landscape: k for kd in [k / 100, (k + 1) / 100), k < 50; 50 from 0.50 on; 51 where kd is None."""
    if kd is None:
        return LANDSCAPE_BINS + 1
    return min(bisect.bisect_right(_LANDSCAPE_EDGES, kd) - 1, LANDSCAPE_BINS)


def landscape_lines(members, header=True, families=None):
    """--landscape: the repeat landscape — per family the copies binned by their Kimura distance to the family's consensus and
    weighted by bases.  members: as for copy_divergence_lines (the representative counts as a copy of its family); families: the
    family names in the order of the file (None: in the order of their first member; a family without a member writes nothing).
    Lines of LANDSCAPE_HEADER: kd_lo and kd_hi (%.2f) of a bin 0.01 wide from 0 up to 0.50, `0.50 inf` for everything beyond
    and `NA NA` for the copies whose distance is undefined (saturated); copies, and bases = matches + transitions +
    transversions + ambiguous of the copies in the bin.  Only non-empty bins are written, per family in order; the same over all
    families follows under the name `all`."""
    lines = [LANDSCAPE_HEADER] if header else []
    if families is None:
        families = list(dict.fromkeys(m[0] for m in members))
    bins = {f: {} for f in families}
    total = {}
    for m in members:
        s = m[6]
        b = landscape_bin(_copy_values(s)[1])
        bases = int(s['matches']) + int(s['transitions']) + int(s['transversions']) + int(s['ambiguous'])
        for acc in (bins[m[0]], total):
            c = acc.setdefault(b, [0, 0])
            c[0] += 1
            c[1] += bases

    def rows(name, acc):
        for b in sorted(acc):
            lo, hi = ('NA', 'NA') if b > LANDSCAPE_BINS else ('0.50', 'inf') if b == LANDSCAPE_BINS else ('%.2f' % (b / 100), '%.2f' % ((b + 1) / 100))
            yield '\t'.join([name, lo, hi, str(acc[b][0]), str(acc[b][1])])

    for f in families:
        lines.extend(rows(f, bins[f]))
    lines.extend(rows('all', total))
    return lines


def import_align(tab_rows, prefix=None, min_len=100, min_idt=95):
    """wrappers.py:33-117 import_Align: re-filter on int(end)-int(start) and float(pID); sort on
    the STRING columns tName, tStart, tEnd, tStrand (lexicographic, stable); UID = prefix_<rank>
    zero-padded to the width of the hit count.  Exits 1 when nothing passes (wrappers.py:94-96)."""
    hits = [f[:10] for f in tab_rows if int(f[3]) - int(f[2]) >= min_len and float(f[9]) >= min_idt]
    if not hits:
        raise SystemExit(1)
    hits.sort(key=lambda f: (f[0], f[2], f[3], f[1]))
    width = len(str(len(hits)))
    pre = str(prefix) if prefix else 'BHit'
    return [f + ['%s_%s' % (pre, str(i).zfill(width))] for i, f in enumerate(hits, 1)]


def gff_map_lines(rows, chrlens=None, ftype='BHit'):
    """wrappers.py:443-522 writeGFFlines (source mimeo-map, ##sequence-region per chromosome)."""
    yield '##gff-version 3\n'
    for name, maxlen in chrlens or []:
        yield ' '.join(['##sequence-region', str(name), '1', str(maxlen) + '\n'])
    yield '\t'.join(['##seqid', 'source', 'type', 'start', 'end', 'score', 'strand', 'phase', 'attributes' + '\n'])
    for r in rows:
        attributes = ';'.join(['ID=' + r[10], 'identity=' + str(r[9]), 'B_locus=' + r[4] + '_' + r[5] + '_' + str(r[6]) + '_' + str(r[7])])
        yield '\t'.join([r[0], 'mimeo-map', ftype, str(r[2]), str(r[3]), str(r[8]), r[1], '.', attributes + '\n'])


def renumber(rows, prefix=None):
    """UIDs after a filter (wrappers.py:243-259): same string sort as import_Align, then rank."""
    rows = sorted((r[:10] for r in rows), key=lambda f: (f[0], f[2], f[3], f[1]))
    width = len(str(len(rows)))
    pre = str(prefix) if prefix else 'BHit'
    return [f + ['%s_%s' % (pre, str(i).zfill(width))] for i, f in enumerate(rows, 1)]


def write_trf_tab(rows, outtab):
    """wrappers.py:380-440 writetrf: the filtered hits in the 10-column TAB layout, `<outtab>.trf`."""
    outfile = outtab + '.trf'
    with open(outfile, 'w') as f:
        f.write('\t'.join(['#name1', 'strand1', 'start1', 'end1', 'name2', 'strand2', 'start2+', 'end2+', 'score',
                           'identity']) + '\n')
        for r in rows:
            f.write('\t'.join(r[:10]) + '\n')
    return outfile
