"""Study (CPU, specification only): what does bounding every gapped extension by the earlier alignments of its (pair,
strand) (mimeo_params.bound_extensions; alignment specification v1, rule 7, last clause; tests/bounded_oracle.c) change
against the plain path anchor rule — anchors, alignments, aligned target bases, live DP cells clipped, and downstream the
regions of the coverage collapse at --minIdt 80 --minLen 100 --minCov 3?  Every ordered pair, both strands.  PARITY UNPINNED.

    python scripts/bounds_vs_path.py dispersed [S] [L] [repeat_frac] [seed] [families]    synth_genome
    python scripts/bounds_vs_path.py flanked [S] [seed]                                    synth.flanked_tandem_genome
    python scripts/bounds_vs_path.py tandem [S] [L] [seed]                                 synth.tandem_genome
-> one JSON line (profiles/r06_bounds_vs_path.jsonl; DESIGN.md §2 "Bounds: counted")
"""
import json
import os
import sys
from multiprocessing import Pool

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from mimeo_amd.synth import flanked_tandem_genome, synth_genome, tandem_genome  # noqa: E402
from scripts.box_vs_path import regions  # noqa: E402
from tests import bounded_oracle as B  # noqa: E402

_G = {}


def _init(seqs):
    _G['seqs'] = seqs


def _pair(tq):
    t, q = tq
    T, Q = _G['seqs'][t], _G['seqs'][q]
    cu, cb = [], []
    unb, bnd = B.align_bounded(T, Q, 0, counts=cu), B.align_bounded(T, Q, 1, counts=cb)
    for a in (unb, bnd):
        a['tid'], a['qid'] = t, q
    return unb, bnd, cu, cb


def main():
    kind = sys.argv[1] if len(sys.argv) > 1 else 'flanked'
    arg = lambda k, d: type(d)(float(sys.argv[k])) if len(sys.argv) > k else d
    if kind == 'dispersed':
        S, L, frac, seed, fams = arg(2, 10), arg(3, 1_000_000), arg(4, 0.05), arg(5, 50), arg(6, 40)
        names, arrs = synth_genome(seed, S * L, S, repeat_frac=frac, families=fams)
        what = {'kind': kind, 'scaffolds': S, 'scaffold_bp': L, 'repeat_frac': frac, 'seed': seed, 'families': fams}
    elif kind == 'tandem':
        S, L, seed = arg(2, 8), arg(3, 150_000), arg(4, 7)
        names, arrs = tandem_genome(seed, S, L)
        what = {'kind': kind, 'scaffolds': S, 'scaffold_bp': L, 'seed': seed}
    else:
        S, seed = arg(2, 8), arg(3, 7)
        names, arrs = flanked_tandem_genome(seed, S)
        what = {'kind': kind, 'scaffolds': S, 'seed': seed, 'scaffold_bp': [int(a.size) for a in arrs]}
    seqs = [a.tobytes() for a in arrs]
    B.lib()
    pairs = [(t, q) for t in range(len(seqs)) for q in range(len(seqs))]
    with Pool(min(16, os.cpu_count() or 1), initializer=_init, initargs=(seqs,)) as pool:
        res = pool.map(_pair, pairs, chunksize=1)
    unb = np.concatenate([r[0] for r in res])
    bnd = np.concatenate([r[1] for r in res])
    cu, cb = np.sum([r[2] for r in res], axis=0), np.sum([r[3] for r in res], axis=0)
    ku, ru = regions(names, seqs, unb)
    kb, rb = regions(names, seqs, bnd)
    cov = lambda a: int((a['tend'].astype(np.int64) - a['tstart']).sum())
    print(json.dumps({
        'genome': what, 'pair_strands': 2 * len(pairs), 'anchors': int(cu[0]),
        'path': {'skipped': int(cu[1]), 'alignments': int(cu[2]), 'aligned_target_bases': cov(unb), 'tab_rows_kept': ku, 'regions': len(ru),
                 'bases_in_regions': int(sum(e - s for _, s, e in ru))},
        'path_bounded': {'skipped': int(cb[1]), 'alignments': int(cb[2]), 'aligned_target_bases': cov(bnd), 'tab_rows_kept': kb,
                         'regions': len(rb), 'bases_in_regions': int(sum(e - s for _, s, e in rb)), 'live_cells_clipped': int(cb[3])},
        'pairs_with_different_alignments': int(sum(r[0].tobytes() != r[1].tobytes() for r in res)),
        'regions_only_path': len(set(ru) - set(rb)), 'regions_only_bounded': len(set(rb) - set(ru)),
    }))


if __name__ == '__main__':
    main()
