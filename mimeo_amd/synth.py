"""Synthetic genomes for tests and bench.py (SURVEY.md §8d "Synthetic inputs").

Upper-case iid-uniform ACGT scaffolds ``scafNNNN`` of equal length with planted repeat
families: ``families`` consensus sequences of length ~U[300, 6000]; copies are placed at
uniform non-overlapping positions on a random strand until ``repeat_frac`` of the genome is
covered; every copy carries substitution divergence ~U[0, max_div] and ``indel_rate`` indels
of length 1-3.  Deterministic in ``seed`` (numpy PCG64).
"""
import numpy as np

_ACGT = np.frombuffer(b'ACGT', dtype=np.uint8)
_COMP = np.array([3, 2, 1, 0], dtype=np.uint8)


def _mutate(rng, cons, div, indel_rate):
    c = cons.copy()
    n = c.size
    sub = rng.random(n) < div
    k = int(sub.sum())
    if k:
        c[sub] = (c[sub] + rng.integers(1, 4, size=k, dtype=np.uint8)) & 3
    nindel = rng.binomial(n, indel_rate)
    if nindel:
        pos = np.sort(rng.integers(0, n, size=nindel))
        pieces, last = [], 0
        for p in pos:
            p = int(p)
            if p < last:
                continue
            ln = int(rng.integers(1, 4))
            pieces.append(c[last:p])
            if rng.random() < 0.5:  # deletion
                last = min(n, p + ln)
            else:  # insertion
                pieces.append(rng.integers(0, 4, size=ln, dtype=np.uint8))
                last = p
        pieces.append(c[last:])
        c = np.concatenate(pieces)
    return c


def synth_genome(seed, total_bp, nscaf, repeat_frac=0.05, families=40, max_div=0.15,
                 indel_rate=0.005, cons_len=(300, 6000), prefix='scaf', shared_families=None, microsat_frac=0.0):
    """Return (names, [uint8 ASCII arrays]).  ``shared_families`` lets two genomes (mimeo x)
    carry copies of the same consensus set: pass the list returned by ``make_families``.
    ``microsat_frac`` (C5: 0.01) overwrites that share of the genome with perfect microsatellites
    of period 1-6 and length 50-500 bp."""
    rng = np.random.Generator(np.random.PCG64(seed))
    L = total_bp // nscaf
    codes = [rng.integers(0, 4, size=L, dtype=np.uint8) for _ in range(nscaf)]
    fams = shared_families if shared_families is not None else make_families(rng, families, cons_len)
    gran = 32
    occ = [np.zeros(L // gran + 2, dtype=bool) for _ in range(nscaf)]
    target = int(repeat_frac * L * nscaf)
    covered, tries = 0, 0
    while covered < target and fams and tries < 50 * (target // cons_len[0] + 10):
        tries += 1
        f = fams[int(rng.integers(0, len(fams)))]
        cp = _mutate(rng, f, float(rng.random()) * max_div, indel_rate)
        if rng.random() < 0.5:
            cp = _COMP[cp[::-1]]
        if cp.size >= L:
            continue
        s = int(rng.integers(0, nscaf))
        p = int(rng.integers(0, L - cp.size))
        a, b = p // gran, (p + cp.size - 1) // gran + 1
        if occ[s][a:b].any():
            continue
        occ[s][a:b] = True
        codes[s][p:p + cp.size] = cp
        covered += cp.size
    target, covered = int(microsat_frac * L * nscaf), 0
    while covered < target:
        period, ln = int(rng.integers(1, 7)), int(rng.integers(50, 501))
        unit = rng.integers(0, 4, size=period, dtype=np.uint8)
        if period > 1 and (unit == unit[0]).all():
            unit[-1] = (unit[0] + 1) & 3
        s, p = int(rng.integers(0, nscaf)), int(rng.integers(0, max(1, L - ln)))
        ln = min(ln, L - p)
        codes[s][p:p + ln] = np.resize(unit, ln)
        covered += ln
    names = ['%s%04d' % (prefix, i) for i in range(nscaf)]
    return names, [_ACGT[c] for c in codes]


def make_families(rng, families=40, cons_len=(300, 6000)):
    if isinstance(rng, (int, np.integer)):
        rng = np.random.Generator(np.random.PCG64(int(rng)))
    return [rng.integers(0, 4, size=int(rng.integers(cons_len[0], cons_len[1] + 1)), dtype=np.uint8)
            for _ in range(families)]


def add_tandem_arrays(seed, arrs, per_scaffold):
    """Tandem arrays written over the scaffolds of synth_genome (new arrays; the input is not changed): `per_scaffold` arrays
    per scaffold, each 8-30 diverged copies (mismatch rate U[0, 0.12]; 30 % of the copies gain or lose 1-20 bases at the end)
    of one of three 150-900 bp units shared by every scaffold.  Chained HSPs on neighbouring diagonals inside one alignment
    box are where the box and path anchor rules part; scripts/box_vs_path.py measures it on these genomes."""
    rng = np.random.default_rng(seed + 7)
    units = [rng.integers(0, 4, size=int(rng.integers(150, 900)), dtype=np.uint8) for _ in range(3)]
    acgt = np.frombuffer(b'ACGT', np.uint8)
    arrs = [a.copy() for a in arrs]
    for a in arrs:
        for _ in range(per_scaffold):
            u = units[int(rng.integers(0, 3))]
            copies = []
            for _c in range(int(rng.integers(8, 31))):
                c = u.copy()
                m = rng.random(c.size) < rng.random() * 0.12
                c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
                if rng.random() < 0.3:   # an indel of 1-20 bases between copies
                    c = np.concatenate([c, rng.integers(0, 4, size=int(rng.integers(1, 21)), dtype=np.uint8)]) if rng.random() < 0.5 else c[:-int(rng.integers(1, 21))]
                copies.append(c)
            arr = acgt[np.concatenate(copies)]
            if arr.size < a.size // 2:
                pos = int(rng.integers(0, a.size - arr.size))
                a[pos:pos + arr.size] = arr
    return arrs


def tandem_genome(seed, nscaf, scaf_bp, per_scaffold=3, repeat_frac=0.05, families=40):
    """synth_genome(seed, nscaf * scaf_bp, nscaf, ...) with add_tandem_arrays on top: (names, list of uint8 ASCII arrays)"""
    names, arrs = synth_genome(seed, nscaf * scaf_bp, nscaf, repeat_frac=repeat_frac, families=families)
    return names, add_tandem_arrays(seed, arrs, per_scaffold)


def flanked_tandem_genome(seed, nscaf, flank=20000, unit=(40, 280), copies=(10, 40), pad=2000, flank_div=0.015, flank_indels=4,
                          copy_div=0.1, delta=5, array_indels=6):
    """Scaffolds that share two unique flanks around a short-unit tandem array: pad | diverged copy of flank 1 | array of
    the scaffold's own copy number | diverged copy of flank 2 | pad.  The array derives from a run of n + delta diverged
    copies (up to `copy_div` substitutions each) of one unit of `unit` bp, n drawn from `copies`; every scaffold loses up
    to 2 delta of them at random places, so that two scaffolds' copy numbers differ by -delta .. +delta around n.  Flanks
    and array carry `flank_div` substitutions per scaffold and `flank_indels` / `array_indels` indels of 1-3 bases.  A gap
    of g bases costs 400 + 30 g against y-drop 9400, so with units below ~300 bp a gapped extension can shift register
    inside the array: under the path anchor rule the chained anchors of the array that the first alignment passed on
    another register are accepted, and each one's extension leaves the array along the flanks unless extensions are
    bounded by the earlier alignments (mimeo_params.bound_extensions; DESIGN.md §2 rule 7).  Deterministic in `seed`.
    Returns (names, uint8 ASCII arrays)."""
    rng = np.random.Generator(np.random.PCG64(seed))
    f1 = rng.integers(0, 4, size=flank, dtype=np.uint8)
    f2 = rng.integers(0, 4, size=flank, dtype=np.uint8)
    u = rng.integers(0, 4, size=int(rng.integers(unit[0], unit[1] + 1)), dtype=np.uint8)
    n0 = int(rng.integers(copies[0], copies[1] + 1))

    def diverged(c, div, nindel):
        c = c.copy()
        m = rng.random(c.size) < div
        c[m] = (c[m] + rng.integers(1, 4, size=int(m.sum()), dtype=np.uint8)) & 3
        for p in sorted(rng.integers(100, max(101, c.size - 100), size=nindel).tolist(), reverse=True):
            ln = int(rng.integers(1, 4))
            c = np.delete(c, slice(p, p + ln)) if rng.random() < 0.5 else np.insert(c, p, rng.integers(0, 4, size=ln, dtype=np.uint8))
        return c

    master = [diverged(u, float(rng.random()) * copy_div, 0) for _ in range(n0 + delta)]
    seqs = []
    for _ in range(nscaf):
        keep = np.sort(rng.permutation(len(master))[:max(2, len(master) - int(rng.integers(0, 2 * delta + 1)))])
        arr = diverged(np.concatenate([master[k] for k in keep]), flank_div, array_indels)
        parts = [rng.integers(0, 4, size=pad, dtype=np.uint8), diverged(f1, flank_div, flank_indels), arr,
                 diverged(f2, flank_div, flank_indels), rng.integers(0, 4, size=pad, dtype=np.uint8)]
        seqs.append(_ACGT[np.concatenate(parts)])
    return ['flk%04d' % i for i in range(nscaf)], seqs


def write_fasta(path, names, seqs, width=60):
    with open(path, 'wb') as f:
        for n, s in zip(names, seqs):
            f.write(b'>' + n.encode() + b'\n')
            b = s.tobytes()
            for i in range(0, len(b), width * 1000):
                chunk = b[i:i + width * 1000]
                f.write(b'\n'.join(chunk[j:j + width] for j in range(0, len(chunk), width)) + b'\n')
