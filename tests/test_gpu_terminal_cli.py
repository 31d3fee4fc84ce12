"""`mimeo self --terminalRepeats` end to end on a synthetic genome with planted LTR and TIR elements: the file is the
restatement's (tests/terminal_spec.py) for the features of the GFF3, every planted element is classified, the LTR pairs are
dated in the order of their planted divergence, and nothing else of the job changes.

The seed below was chosen on the CPU before any GPU run: with the planted elements themselves as the features (and with their
ends moved by up to 8 bases either way), the restatement gives assertions 2 - 4."""
import os

import numpy as np
import pytest

from mimeo_amd import formats
from mimeo_amd.synth import write_fasta
from tests import terminal_spec as S

pytestmark = pytest.mark.gpu

SEED = 1717
NSCAF, SCAF_LEN = 4, 60_000
LTR_LEN, LTR_BODY, LTR_DIV = 250, 1500, (0.0, 0.03, 0.08, 0.15)
TIR_LEN, TIR_BODY = 40, 1120
LETTERS = np.frombuffer(b'ACGT', dtype=np.uint8)


def substituted(rng, codes, rate):
    """exactly round(rate * n) substitutions"""
    c = codes.copy()
    at = rng.choice(c.size, size=int(round(rate * c.size)), replace=False)
    c[at] = (c[at] + rng.integers(1, 4, size=at.size, dtype=np.uint8)) % 4
    return c


def planted_genome(seed=SEED):
    """(names, seqs as letters, ltr elements, tir elements): scaffold k holds copy k of a 2 kb element — its interior 3 per cent
    from the ancestor's, its own pair of 250-base LTRs substitution-only and LTR_DIV[k] apart — and copy k of a 1.2 kb element
    with 40-base terminal inverted repeats.  An element is (scaffold, start, end)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ltr0, body0 = rng.integers(0, 4, LTR_LEN, dtype=np.uint8), rng.integers(0, 4, LTR_BODY, dtype=np.uint8)
    tir0, tbody0 = rng.integers(0, 4, TIR_LEN, dtype=np.uint8), rng.integers(0, 4, TIR_BODY, dtype=np.uint8)
    names, seqs, ltrs, tirs = [], [], [], []
    for k in range(NSCAF):
        c = rng.integers(0, 4, SCAF_LEN, dtype=np.uint8)
        left = substituted(rng, ltr0, 0.01)
        el = np.concatenate([left, substituted(rng, body0, 0.03), substituted(rng, left, LTR_DIV[k])])
        a = 7000 + 9000 * k
        c[a:a + el.size] = el
        ltrs.append((k, a, a + el.size))
        tl = substituted(rng, tir0, 0.0)
        tel = np.concatenate([tl, substituted(rng, tbody0, 0.03), (3 - tl)[::-1]])
        b = 50_000 - 4000 * k   # behind the other element in every scaffold: the chains of a scaffold pair keep both
        c[b:b + tel.size] = tel
        tirs.append((k, b, b + tel.size))
        names.append('scaf%d' % k)
        seqs.append(LETTERS[c])
    return names, seqs, ltrs, tirs


def read_features(gff, names):
    """the GFF3's rows as (ID, seqid, start, end) and as region intervals numbered by sorted name"""
    names_sorted = sorted(names, key=lambda s: s.encode())
    rows = [ln.split('\t') for ln in open(gff).read().splitlines() if ln and not ln.startswith('#')]
    feats = [(r[8].split('ID=')[1].split(';')[0], r[0], int(r[3]), int(r[4])) for r in rows]
    reg = np.zeros(len(feats), dtype=np.dtype([('chrom', '<u4'), ('start', '<u4'), ('end', '<u4')]))
    for i, (_, seqid, s, e) in enumerate(feats):
        reg[i] = (names_sorted.index(seqid), s, e)
    return feats, reg, names_sorted


def restated_lines(names, seqs, reg, names_sorted, prefix, **kw):
    iv = [(names.index(names_sorted[int(r['chrom'])]), int(r['start']), int(r['end'])) for r in reg]
    recs, first, blocks = S.terminal_repeats(seqs, iv, **kw)
    return formats.terminal_repeat_lines(reg, names_sorted, prefix, S.params(**kw)['window'], recs, S.column_stats(seqs, recs, first, blocks))


def check_planted(lines, ltrs, tirs, names):
    """assertions 2 - 4 on the lines of a file"""
    rows = [dict(zip(formats.TERMINAL_REPEATS_HEADER.lstrip('#').split('\t'), ln.split('\t'))) for ln in lines[1:]]
    assert lines[0] == formats.TERMINAL_REPEATS_HEADER

    def line_of(el, kind):
        k, a, b = el
        hit = [r for r in rows if r['seqid'] == names[k] and r['kind'] == kind and int(r['start']) < a + 100 and int(r['end']) > b - 100]
        assert len(hit) == 1, (el, kind, hit)
        return hit[0]

    def cover(r, side, lo, hi):
        return max(0, min(int(r[side + '_end']), hi) - max(int(r[side + '_start']), lo))

    kds = []
    for el in ltrs:   # 2: both intervals cover 90 per cent of the planted LTR
        r = line_of(el, 'LTR')
        assert cover(r, 'left', el[1], el[1] + LTR_LEN) >= 0.9 * LTR_LEN and cover(r, 'right', el[2] - LTR_LEN, el[2]) >= 0.9 * LTR_LEN, r
        assert int(r['left_start']) >= el[1] - 20 and int(r['right_end']) <= el[2] + 20
        kds.append(float(r['kd']))
    assert all(x < y for x, y in zip(kds, kds[1:])), kds   # 3: kd rises strictly with the planted divergence
    assert kds[0] == 0.0
    for el in tirs:   # 4: a TIR line on the planted ends
        r = line_of(el, 'TIR')
        assert cover(r, 'left', el[1], el[1] + TIR_LEN) >= 30 and cover(r, 'right', el[2] - TIR_LEN, el[2]) >= 30, r
        assert int(r['left_end']) <= el[1] + TIR_LEN + 10 and int(r['right_start']) >= el[2] - TIR_LEN - 10, r
        assert int(r['score']) >= 60


def test_self_terminal_repeats(tmp_path, monkeypatch, capfd):
    from mimeo_amd import run_self
    names, seqs, ltrs, tirs = planted_genome()
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, term = tmp_path / 'plain', tmp_path / 'term'
    monkeypatch.setenv('MIMEO_TERMINAL_STATS', '1')
    capfd.readouterr()
    run_self.main(['--afasta', fa, '-d', str(plain), '--loglevel', 'WARNING', '--families', str(plain / 'fam.tsv')])
    assert '[k17]' not in capfd.readouterr().err   # 6: without the flag no K17 launch
    run_self.main(['--afasta', fa, '-d', str(term), '--loglevel', 'WARNING', '--families', str(term / 'fam.tsv'), '--terminalRepeats', str(term / 'term.tsv')])
    assert capfd.readouterr().err.count('[k17] terminal repeats') == 1   # one call for the one block of GFF3 rows
    # 5: every other output is byte for byte what a run without the flag writes
    assert sorted(os.listdir(term)) == sorted(os.listdir(plain) + ['term.tsv'])
    for f in os.listdir(plain):
        assert (term / f).read_bytes() == (plain / f).read_bytes(), f
    # 1: the file is the restatement's for the features of the GFF3
    feats, reg, names_sorted = read_features(term / 'mimeo-self_repeats.gff3', names)
    assert len(feats) >= 8
    prefix = feats[0][0].rsplit('_', 1)[0]
    got = (term / 'term.tsv').read_text().splitlines()
    assert got == restated_lines(names, seqs, reg, names_sorted, prefix)
    check_planted(got, ltrs, tirs, names)   # 2 - 4
    # the flag alone, with other parameters: needs neither --paf nor --families
    alone = tmp_path / 'alone'
    run_self.main(['--afasta', fa, '-d', str(alone), '--loglevel', 'WARNING', '--terminalRepeats', str(alone / 't.tsv'), '--terminalWindow', '300',
                   '--terminalMinScore', '25'])
    assert (alone / 't.tsv').read_text().splitlines() == restated_lines(names, seqs, reg, names_sorted, prefix, window=300, min_score=25)
    assert (alone / 'mimeo-self_repeats.gff3').read_bytes() == (plain / 'mimeo-self_repeats.gff3').read_bytes()
