"""Designed inputs for K18 (mimeo_flank_repeats) and K19 (mimeo_open_frames), shared by tests/test_host_elements.py (where the
two restatements of tests/elements_spec.py must agree on them, and give the answers written here) and tests/test_gpu_elements.py
(where the kernels must).  A K18 case is (name, scaffolds, items, params, expected): expected[i] is None (whatever the
restatement says) or (len, mismatches, dl, dr), len 0 for "no duplication".  A K19 case is (name, scaffolds, items)."""
import numpy as np

LETTERS = np.frombuffer(b'ACGT', dtype=np.uint8)
SENSE = [(x, y, z) for x in range(4) for y in range(4) for z in range(4) if (x, y, z) not in ((3, 0, 0), (3, 0, 2), (3, 2, 0))]


def rand(rng, n):
    return LETTERS[rng.integers(0, 4, n)].copy()


def other(rng, *letters):
    """a letter that is none of these"""
    return int(rng.choice([c for c in LETTERS.tolist() if c not in [int(x) for x in letters]]))


def cat(*parts):
    return np.concatenate([np.frombuffer(p, dtype=np.uint8) if isinstance(p, bytes) else np.asarray(p, dtype=np.uint8) for p in parts]).astype(np.uint8)


def site(rng, tsd, el_len=70, pre=60, post=60):
    """pre + tsd + element + tsd + post, planted unambiguously: the base before the left copy differs from the element's last
    base and the base after the right copy from the element's first, and the copies' own neighbours differ, so the duplication
    is neither longer nor shifted.  Returns (sequence, element start, element end)."""
    tsd = np.frombuffer(tsd, dtype=np.uint8) if isinstance(tsd, bytes) else tsd
    el, a, b = rand(rng, el_len), rand(rng, pre), rand(rng, post)
    if pre:
        a[-1] = other(rng, el[-1])
    if post:
        b[0] = other(rng, el[0])
    return cat(a, tsd, el, tsd, b), pre + len(tsd), pre + len(tsd) + el_len


def k18_cases():
    rng = np.random.default_rng(1818)
    out = []
    # exact duplications of min_len and of max_len; 25 bases at max_len 20 are not found
    for name, n, exp in (('min_len', 4, (4, 0, 0, 0)), ('max_len', 20, (20, 0, 0, 0)), ('longer than max_len', 25, (0, 0, 0, 0))):
        s, a, b = site(rng, rand(rng, n))
        out.append((name, [s], [(0, a, b)], {}, [exp]))
    # the corners of the slack square, and one step outside
    s, a, b = site(rng, rand(rng, 9))
    for dl, dr in ((-2, -2), (-2, 2), (2, -2), (2, 2), (0, 0), (1, -2)):
        out.append(('shift %d %d' % (dl, dr), [s], [(0, a - dl, b - dr)], {}, [(9, 0, dl, dr)]))
    out.append(('shift 3 0 is outside the slack', [s], [(0, a - 3, b)], {}, [None]))
    # the full window: max_len 32 at slack 0 and slack 8, duplications of 32 at the far corners
    s, a, b = site(rng, rand(rng, 32))
    out.append(('slack 0, 32 bases', [s], [(0, a, b)], dict(max_len=32, slack=0), [(32, 0, 0, 0)]))
    for dl, dr in ((-8, -8), (8, 8), (-8, 8), (8, -8)):
        out.append(('slack 8, 32 bases, shift %d %d' % (dl, dr), [s], [(0, a - dl, b - dr)], dict(max_len=32, slack=8), [(32, 0, dl, dr)]))
    # the scaffold's ends, an empty item, a scaffold shorter than a word
    s, a, b = site(rng, rand(rng, 7), pre=0, post=0)
    out.append(('copies at base 0 and at the last base', [s], [(0, a, b)], {}, [(7, 0, 0, 0)]))
    out.append(('start 0, end L', [s], [(0, 0, len(s)), (0, 0, 0), (0, len(s), len(s))], {}, [(0, 0, 0, 0)] * 3))
    short = cat(b'GATTACA', b'CCGGTGCATGCAACCGTTGG', b'GATTACA', b'TC')
    out.append(('a scaffold of 36 bases', [short], [(0, 7, 27), (0, 8, 26), (0, 20, 20)], dict(slack=8, max_len=32), [(7, 0, 0, 0), (7, 0, -1, 1), None]))
    out.append(('empty item inside a tandem', [cat(b'ACGTTGCA' * 6)], [(0, 24, 24), (0, 23, 25)], dict(slack=3), [None, None]))
    # N in a column; a mismatch in the middle, with and without room for its charge; a mismatch in an end column
    s, a, b = site(rng, rand(rng, 10))
    n = s.copy()
    n[a - 5] = n[b + 5] = ord('N')
    out.append(('N in both copies is a mismatch', [n], [(0, a, b)], dict(max_mismatch=0), [(0, 0, 0, 0)]))
    out.append(('N under one mismatch', [n], [(0, a, b)], dict(max_mismatch=1), [(10, 1, 0, 0)]))
    m = s.copy()
    m[a - 5] = other(rng, m[a - 5])
    out.append(('mismatch, none allowed', [m], [(0, a, b)], dict(max_mismatch=0), [(0, 0, 0, 0)]))
    out.append(('mismatch, one allowed: 10 - 3 >= 4', [m], [(0, a, b)], dict(max_mismatch=1), [(10, 1, 0, 0)]))
    out.append(('mismatch, one allowed: 10 - 3 < 8', [m], [(0, a, b)], dict(max_mismatch=1, min_len=8), [(0, 0, 0, 0)]))
    out.append(('mismatch, two allowed', [m], [(0, a, b)], dict(max_mismatch=2), [(10, 1, 0, 0)]))
    e = s.copy()
    e[a - 10] = other(rng, e[a - 10])   # the first column of the left copy: the other nine are an exact duplication
    out.append(('mismatch in the first column', [e], [(0, a, b)], dict(max_mismatch=1), [(9, 0, 0, 1)]))
    e = s.copy()
    e[b + 9] = other(rng, e[b + 9])
    out.append(('mismatch in the last column', [e], [(0, a, b)], dict(max_mismatch=1), [(9, 0, -1, 0)]))
    # ties: TTAA twice in reach — equal v, the smaller |dl| + |dr| wins; equal sums: the smaller dl
    t1 = cat(b'GGCGC', b'TTAA', b'C', b'GACCGTGCATCGGATCGGCA', b'G', b'TTAA', b'GCGCC')
    out.append(('equal v, sums 0 and 2', [t1], [(0, 9, 31), (0, 10, 30)], dict(slack=2), [(4, 0, 0, 0), (4, 0, -1, 1)]))
    t2 = cat(b'GGCGC', b'TCAG', b'TCAG', b'GACCGTGCATCGGATCGGCA', b'TCAG', b'GCGCC')
    out.append(('a tandem on the left: the copy next to the element', [t2], [(0, 13, 33)], dict(slack=4, max_len=4), [(4, 0, 0, 0)]))
    t3 = cat(b'GGCGC', b'ACCAGT', b'GACCGTGCATCGGATCGGCA', b'ACCAGT', b'CGCCC')   # six bases duplicated, four allowed: three places
    out.append(('equal sums 2: dl -2, dr 0 before -1, 1 and 0, 2', [t3], [(0, 11, 31)], dict(slack=2, max_len=4), [(4, 0, -2, 0)]))
    # TTAA . TIR ... TIR' . TTAA with the feature cut 4 bases wide: the palindromic duplication is found at dl = +4, dr = -4
    tir = rand(rng, 24)
    tir[0], tir[-1] = ord('C'), ord('G')
    body = rand(rng, 40)
    rc = np.array([{65: 84, 67: 71, 71: 67, 84: 65}[int(x)] for x in tir[::-1]], dtype=np.uint8)
    pal = cat(rand(rng, 30), b'G', b'TTAA', tir, body, rc, b'TTAA', b'C', rand(rng, 30))
    out.append(('palindromic TTAA at slack 4', [pal], [(0, 31, 31 + 4 + 24 + 40 + 24 + 4)], dict(slack=4), [(4, 0, 4, -4)]))
    return out


def k18_random(n=5000, seed=18):
    """n unsorted items over four scaffolds, two of them with N runs, two letters in one: duplications everywhere"""
    rng = np.random.default_rng(seed)
    seqs = [rand(rng, 3000), rand(rng, 997), LETTERS[rng.integers(0, 2, 2000)].copy(), rand(rng, 61)]
    seqs[1][rng.integers(0, 997, 60)] = ord('N')
    items = []
    for _ in range(n):
        c = int(rng.integers(0, 4))
        L = len(seqs[c])
        a = int(rng.integers(0, L + 1))
        b = min(L, a + int(rng.integers(0, 40))) if rng.random() < 0.5 else int(rng.integers(a, L + 1))
        items.append((c, a, b))
    return seqs, items


def sense_run(rng, codons):
    return LETTERS[np.array([SENSE[i] for i in rng.integers(0, len(SENSE), codons)]).ravel()].copy()


def k19_cases():
    rng = np.random.default_rng(1919)
    out = []
    base = rand(rng, 9000)
    for lo, hi in ((0, 6), (62, 68), (4093, 4101)):   # tiny items; a codon over a word's edge; over a step's edge
        out.append(('items of %d..%d bases' % (lo, hi - 1), [base], [(0, a, a + n) for n in range(lo, hi) for a in (0, 1, 2, 777, len(base) - n)]))
    open30 = sense_run(rng, 30)
    out.append(('a stop first and last', [cat(b'TAA', open30, b'TGA'), cat(b'C', b'TAG', open30, b'TAA', b'GG')], [(0, 0, 96), (1, 0, 99), (1, 1, 97), (1, 0, 50)]))
    out.append(('no open codon', [cat(b'TAATAGTGA' * 5)], [(0, 0, 45), (0, 0, 44), (0, 3, 9)]))
    out.append(('N inside a codon', [cat(open30[:30], b'ANC', open30[30:], b'NNNNNNNNNNNN', open30[:45])], [(0, 0, 150), (0, 1, 149), (0, 30, 36)]))
    run = sense_run(rng, 10)
    out.append(('ties in a frame and across frames', [cat(run, b'TAA', run, b'TAG', run[:27]), cat(b'TGA', run, b'TAAC', run, b'TGA')],
                [(0, 0, 93), (0, 0, 66), (1, 0, 70), (1, 3, 67)]))   # two runs of ten in one frame: the first; ten in frame 0 and ten in frame 1
    quiet = LETTERS[np.array([c for c in SENSE if c != (0, 3, 2)])[rng.integers(0, 60, 40)].ravel()].copy()   # no ATG in frame 0
    for name, at in (('first', 0), ('in the middle', 17), ('absent', None)):
        s = quiet.copy()
        if at is not None:
            s[3 * at:3 * at + 3] = np.frombuffer(b'ATG', dtype=np.uint8)
        out.append(('met %s' % name, [cat(b'TAA', s, b'TAA')], [(0, 0, 126), (0, 3, 123)]))
    edge = rand(rng, 300)
    out.append(('items at the scaffold ends', [edge], [(0, 0, 300), (0, 0, 100), (0, 200, 300), (0, 299, 300), (0, 0, 1)]))
    return out


def k19_long(seed=190):
    """10 000 bases whose frame 0 is drawn from the 61 sense codons: one run over three steps"""
    rng = np.random.default_rng(seed)
    return cat(sense_run(rng, 3333), b'A')


def k19_random(n=2000, seed=19):
    rng = np.random.default_rng(seed)
    seqs = [rand(rng, 20000), rand(rng, 5003), rand(rng, 64)]
    seqs[1][rng.integers(0, 5003, 40)] = ord('N')
    items = []
    for _ in range(n):
        c = int(rng.integers(0, 3))
        L = len(seqs[c])
        a = int(rng.integers(0, L + 1))
        items.append((c, a, min(L, a + int(rng.integers(0, 700)))))
    return seqs, items
