"""Cost of linking regions into families (profiles/r17_link_regions_cost.json): HIP-event kernel time and wall time of
mimeo_link_regions (K12) and, over the very same items, of mimeo_path_window_stats (K10), which reads the sequences for every
item where K12 reads only blocks and the region table.

The case is the union-find case of tests/test_gpu_families.py scaled up: 7 000 regions of 100 bases — a chain of 4 000 linked
i <-> i + 1, a star of 2 000 around its last region on the minus strand, 500 pairs —, every link an alignment of one 100-column
block in each direction (12 996 records), every item `--repeat` times (770: 10^7 items), in three orders: by record (the order
formats.region_items makes), the list tiled, and shuffled.  One warm-up call, then `--calls` timed ones of each kernel,
alternating.  The kernel times are what the libraries print with MIMEO_LINK_STATS=1 / MIMEO_WINDOW_STATS_STATS=1 on stderr.

    python scripts/gpu_link_regions_cost.py [--repeat 770] [--calls 3] > walls.json 2> kernel_lines.txt   (needs the GPU)
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

L = [600_000, 300_000, 150_000]
CHAIN, STAR, PAIRS = 4000, 2000, 500


def case():
    from mimeo_amd import _ffi
    start = lambda k: 150 * k + 20
    regions = [(0, start(k), start(k) + 100) for k in range(CHAIN)] + [(1, start(k), start(k) + 100) for k in range(STAR)] + \
              [(2, start(k), start(k) + 100) for k in range(2 * PAIRS)]
    recs, blocks, items = [], [], []

    def link(scaf, base, i, j, strand):
        for a, b in ((i, j), (j, i)):
            items.append((len(recs), base + a, start(a), start(a) + 100))
            recs.append((scaf, strand))
            blocks.append((start(a), L[scaf] - (start(b) + 100) if strand else start(b), 100))
    for i in range(CHAIN - 1):
        link(0, 0, i, i + 1, i & 1)
    for j in range(STAR - 1):
        link(1, CHAIN, j, STAR - 1, 1)
    for k in range(PAIRS):
        link(2, CHAIN + STAR, 2 * k, 2 * k + 1, 0)
    r = np.zeros(len(recs), dtype=_ffi.ALIGNMENT)
    r['tid'] = r['qid'] = [x[0] for x in recs]
    r['qstrand'] = [x[1] for x in recs]
    reg = np.zeros(len(regions), dtype=_ffi.INTERVAL)
    reg['chrom'], reg['start'], reg['end'] = zip(*regions)
    return r, np.arange(len(recs) + 1, dtype=np.uint64), np.array(blocks, dtype=_ffi.PATH_BLOCK), reg, np.array(items, dtype=np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--repeat', type=int, default=770)
    ap.add_argument('--calls', type=int, default=3)
    args = ap.parse_args()
    os.environ['MIMEO_LINK_STATS'] = '1'
    os.environ['MIMEO_WINDOW_STATS_STATS'] = '1'
    from mimeo_amd import _ffi, engine
    engine.init(0)
    rng = np.random.default_rng(72)
    acgt = np.frombuffer(b'ACGT', dtype=np.uint8)
    G = engine.Genome(['u0', 'u1', 'u2'], [acgt[rng.integers(0, 4, n)] for n in L])
    recs, first, blocks, reg, items1 = case()
    tiled = np.tile(items1, (args.repeat, 1))
    orders = (('by_record', np.repeat(items1[np.argsort(items1[:, 0], kind='stable')], args.repeat, axis=0)), ('tiled', tiled),
              ('shuffled', tiled[np.random.default_rng(1).permutation(tiled.shape[0])]))
    out = {'records': int(recs.size), 'regions': int(reg.size), 'repeat': args.repeat, 'orders': {}}
    for name, items in orders:
        it = np.zeros(items.shape[0], dtype=_ffi.WINDOW_ITEM)
        it['aln'], it['group'], it['w0'], it['w1'] = items[:, 0], items[:, 1], items[:, 2], items[:, 3]
        walls = {'k12': [], 'k10': []}
        print('== %s: %d items' % (name, it.size), file=sys.stderr, flush=True)
        for k in range(args.calls + 1):   # the first call is the warm-up
            t = time.perf_counter()
            fam, lnk = engine.link_regions(G, recs, first, blocks, reg, None, it, 80)
            w12 = time.perf_counter() - t
            t = time.perf_counter()
            ws = engine.window_stats(G, None, recs, first, blocks, it, reg.size)
            w10 = time.perf_counter() - t
            if k:
                walls['k12'].append(round(w12 * 1e3, 2))
                walls['k10'].append(round(w10 * 1e3, 2))
        assert int(lnk.sum()) == it.size and len(set(fam.tolist())) == 2 + PAIRS
        assert int(sum(ws[f].sum() for f in ('matches', 'transitions', 'transversions', 'ambiguous'))) == 100 * it.size
        out['orders'][name] = {'items': int(it.size), 'wall_ms': walls}
    G.close()
    print(json.dumps(out, indent=1))


if __name__ == '__main__':
    main()
