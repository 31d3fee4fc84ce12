"""Host-side handle on the HIP engine: what the reference's `*_LZ_cmds` + `run_cmd`
(src/mimeo/wrappers.py:899-1271, src/mimeo/utils.py:213-254) become once the shell pipeline
is replaced by calls through the C-ABI."""
import ctypes as C
import os

import numpy as np

from . import _ffi

_initialised_device = None


def init(device=0):
    """Bind this process to one GPU (one process per GPU)."""
    global _initialised_device
    lib = _ffi.load()
    _ffi.check(lib.mimeo_init(int(device)))
    _initialised_device = int(device)


def default_params(**kw):
    p = _ffi.Params()
    _ffi.check(_ffi.load().mimeo_params_default(C.byref(p)))
    for k, v in kw.items():
        setattr(p, k, int(v))
    return p


def stats():
    s = _ffi.Stats()
    _ffi.check(_ffi.load().mimeo_get_stats(C.byref(s)))
    return s.asdict()


class Genome:
    """Device-resident scaffolds (both strands, bit-plane packed)."""

    def __init__(self, names, seqs):
        """names: list[str]; seqs: list of bytes / uint8 arrays of ASCII bases."""
        lib = _ffi.load()
        self.names = list(names)
        arrs = [np.frombuffer(s, dtype=np.uint8) if isinstance(s, (bytes, bytearray)) else np.ascontiguousarray(s, dtype=np.uint8)
                for s in seqs]
        self.lengths = [int(a.size) for a in arrs]
        offsets = np.zeros(len(arrs) + 1, dtype=np.uint64)
        offsets[1:] = np.cumsum(self.lengths, dtype=np.uint64)
        bases = np.concatenate(arrs) if arrs else np.zeros(0, dtype=np.uint8)
        if bases.size == 0:
            bases = np.zeros(1, dtype=np.uint8)
        h = C.c_void_p()
        _ffi.check(lib.mimeo_genome_create(len(arrs), bases.ctypes.data, offsets.ctypes.data, C.byref(h)))
        self._h = h

    @classmethod
    def from_fasta(cls, paths, split_dir=None):
        """Stream FASTA file(s) from disk straight into device memory (native parser thread + K1;
        replaces utils.py:274-309 splitFasta and the Biopython parses).  `split_dir`: also leave one
        `<id>.fa` per record there, like the reference's --adir/--bdir."""
        lib = _ffi.load()
        paths = [paths] if isinstance(paths, (str, bytes)) else list(paths)
        arr = (C.c_char_p * len(paths))(*[os.fsencode(p) for p in paths])
        h = C.c_void_p()
        _ffi.check(lib.mimeo_genome_load_fasta(arr, len(paths), os.fsencode(split_dir) if split_dir else None, C.byref(h)))
        self = cls.__new__(cls)
        self._h = h
        n = C.c_uint32()
        _ffi.check(lib.mimeo_genome_nscaf(h, C.byref(n)))
        self.names, self.lengths = [], []
        for i in range(n.value):
            nm, ln = C.c_char_p(), C.c_uint64()
            _ffi.check(lib.mimeo_genome_name(h, i, C.byref(nm)))
            _ffi.check(lib.mimeo_genome_length(h, i, C.byref(ln)))
            self.names.append(nm.value.decode())
            self.lengths.append(int(ln.value))
        return self

    def keep_indexes(self, keep=True):
        """Seed indexes built by later align_pairs calls stay attached to this genome and are reused
        (lastz rebuilds the table in every run, wrappers.py:1028-1031); results do not change."""
        _ffi.check(_ffi.load().mimeo_genome_keep_indexes(self._h, 1 if keep else 0))

    def build_indexes(self, scaffolds=None):
        """Build and keep the seed indexes of the listed scaffolds now (None = all)."""
        ids = np.ascontiguousarray([] if scaffolds is None else list(scaffolds), dtype=np.uint32)
        if scaffolds is not None and ids.size == 0:
            return
        _ffi.check(_ffi.load().mimeo_genome_build_indexes(self._h, ids.ctypes.data if ids.size else None, ids.size))

    def drop_indexes(self, scaffolds=None):
        """Release the kept seed indexes (both strands) of the listed scaffolds; None = all."""
        ids = np.ascontiguousarray([] if scaffolds is None else list(scaffolds), dtype=np.uint32)
        if scaffolds is not None and ids.size == 0:
            return
        _ffi.check(_ffi.load().mimeo_genome_drop_indexes(self._h, ids.ctypes.data if ids.size else None, ids.size))

    def close(self):
        if getattr(self, '_h', None) is not None and self._h.value:
            _ffi.load().mimeo_genome_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __len__(self):
        return len(self.names)


def seed_hits(T, tid, Q, qid, qstrand=0, params=None):
    p = params or default_params()
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_seed_hits(T._h, tid, Q._h, qid, int(qstrand), C.byref(p), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.SEED_HIT)


def ungapped_hsps(T, tid, Q, qid, qstrand=0, params=None):
    p = params or default_params()
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_ungapped_hsps(T._h, tid, Q._h, qid, int(qstrand), C.byref(p), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.HSP)


def chain_hsps(hsps):
    """lastz --chain on the HSPs of one (target, query, strand): the HSPs in (tstart, qstart, length) order, bit 0 of
    `flags` set on the members of the chain (include/mimeo_hip.h: mimeo_chain_hsps; a test entry like ungapped_hsps)."""
    h = np.ascontiguousarray(hsps, dtype=_ffi.HSP)
    out = np.zeros(h.size, dtype=_ffi.HSP)
    _ffi.check(_ffi.load().mimeo_chain_hsps(h.ctypes.data, h.size, out.ctypes.data))
    return out


def align_pair(T, tid, Q, qid, params=None):
    p = params or default_params()
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_align_pair(T._h, tid, Q._h, qid, C.byref(p), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.ALIGNMENT)


def _align_paths(A, B, pt, pq, ps, p):
    """mimeo_align_units_paths: (records, first, blocks) — alignment i is blocks[first[i]:first[i + 1]]."""
    ptr, n, pf, pb, nb = C.c_void_p(), C.c_uint64(), C.c_void_p(), C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_align_units_paths(A._h, B._h if B is not None else None, pt.ctypes.data, pq.ctypes.data,
                                                   ps.ctypes.data if ps is not None else None, len(pt), C.byref(p),
                                                   C.byref(ptr), C.byref(n), C.byref(pf), C.byref(pb), C.byref(nb)))
    n1 = C.c_uint64(n.value + 1)
    return _ffi.take(ptr, n, _ffi.ALIGNMENT), _ffi.take(pf, n1, np.dtype('<u8')), _ffi.take(pb, nb, _ffi.PATH_BLOCK)


def align_pairs(A, B, pairs, params=None, paths=False):
    """pairs: iterable of (target index in A, query index in B or A).  paths=True: (records, first, blocks) with the path of
    record i as the gap-free blocks blocks[first[i]:first[i + 1]] (_ffi.PATH_BLOCK; include/mimeo_hip.h has the coordinates)."""
    p = params or default_params()
    pr = np.asarray(list(pairs), dtype=np.uint32).reshape(-1, 2)
    pt = np.ascontiguousarray(pr[:, 0])
    pq = np.ascontiguousarray(pr[:, 1])
    if paths:
        return _align_paths(A, B, pt, pq, None, p)
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_align_pairs(A._h, B._h if B is not None else None, pt.ctypes.data, pq.ctypes.data,
                                             len(pt), C.byref(p), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.ALIGNMENT)


def align_units(A, B, units, params=None, paths=False):
    """units: iterable of (target index in A, query index in B or A, strands) with strands = 1 plus, 2 minus, 3 both
    (masked with params.strand): mimeo_align_units — a rank's share of a sharded self job (dist.deal_units).
    paths=True: (records, first, blocks), as align_pairs."""
    p = params or default_params()
    un = np.asarray(list(units), dtype=np.uint32).reshape(-1, 3)
    pt, pq = np.ascontiguousarray(un[:, 0]), np.ascontiguousarray(un[:, 1])
    ps = np.ascontiguousarray(un[:, 2].astype(np.uint8))
    if paths:
        return _align_paths(A, B, pt, pq, ps, p)
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_align_units(A._h, B._h if B is not None else None, pt.ctypes.data, pq.ctypes.data, ps.ctypes.data,
                                             len(pt), C.byref(p), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.ALIGNMENT)


def _paths(records, first, blocks):
    """records / first / blocks of a path call as contiguous arrays of the ABI's types"""
    recs = np.ascontiguousarray(records, dtype=_ffi.ALIGNMENT)
    first = np.ascontiguousarray(first, dtype=np.uint64)
    blk = np.ascontiguousarray(blocks, dtype=_ffi.PATH_BLOCK)
    if first.size != recs.size + 1:
        raise ValueError('first has %d entries for %d records (one more is needed)' % (first.size, recs.size))
    return recs, first, blk


def _window_items(items):
    """_ffi.WINDOW_ITEM rows, or an (n, 4) array of (aln, group, w0, w1), as contiguous _ffi.WINDOW_ITEM rows"""
    it = np.asarray(items)
    if it.dtype != _ffi.WINDOW_ITEM:
        a = np.asarray(it, dtype=np.uint32).reshape(-1, 4)
        it = np.zeros(a.shape[0], dtype=_ffi.WINDOW_ITEM)
        it['aln'], it['group'], it['w0'], it['w1'] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    return np.ascontiguousarray(it)


def path_stats(A, B, records, first, blocks):
    """Column statistics of alignment paths (mimeo_path_stats, kernel K9): one _ffi.COLUMN_STATS row per record — matches,
    transitions, transversions and ambiguous columns of its blocks blocks[first[i]:first[i + 1]], insertion / deletion runs and
    bases between them.  records / first / blocks as align_pairs(..., paths=True) returns them (or any selection of them:
    formats.select_paths); B = None: the queries are scaffolds of A.  A path that breaks the contract of mimeo_path_block is a
    RuntimeError naming the record, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    out = np.zeros(recs.size, dtype=_ffi.COLUMN_STATS)
    if recs.size:
        _ffi.check(_ffi.load().mimeo_path_stats(A._h, B._h if B is not None else None, recs.ctypes.data, recs.size, first.ctypes.data,
                                                blk.ctypes.data if blk.size else None, blk.size, out.ctypes.data))
    return out


def window_stats(A, B, records, first, blocks, items, ngroups):
    """Column statistics of alignment paths clipped to target windows and summed into groups (mimeo_path_window_stats, kernel
    K10): an array of `ngroups` rows of _ffi.WINDOW_STATS.  records / first / blocks as for path_stats; items: _ffi.WINDOW_ITEM
    rows (or an (n, 4) array) of (record number, group, w0, w1) — the columns of that record whose target base lies in
    [w0, w1) of its target scaffold's plus strand, and the gaps that start there (include/mimeo_hip.h has the rules), are added
    to the group.  Items come in any order; a group without items is zero.  A bad path or a bad item is a RuntimeError naming
    it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    it = _window_items(items)
    out = np.zeros(int(ngroups), dtype=_ffi.WINDOW_STATS)
    _ffi.check(_ffi.load().mimeo_path_window_stats(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size,
                                                   first.ctypes.data, blk.ctypes.data if blk.size else None, blk.size,
                                                   it.ctypes.data if it.size else None, it.size, int(ngroups),
                                                   out.ctypes.data if out.size else None))
    return out


def link_regions(A, records, first, blocks, regions, chrom_of_tid, items, min_cover_pct=80):
    """Repeat families (mimeo_link_regions, kernel K12): (family, links), two arrays with one entry per region — family[i] the
    smallest region number of the family of region i (uint32; family[i] <= i), links[i] how often region i was linked to
    another one (uint64).  A self job: records / first / blocks as for path_stats, with the queries scaffolds of A; regions:
    _ffi.INTERVAL rows as coverage_collapse returns them (or an (n, 3) array), sorted by (chrom, start) and disjoint;
    chrom_of_tid[tid]: the region chromosome number of scaffold tid (None: tid itself); items: _ffi.WINDOW_ITEM rows (or an
    (n, 4) array) of (record number, region number, w0, w1) as formats.region_items makes them.  An item whose window covers
    min_cover_pct per cent of its region is projected through the record's path onto the query scaffold, and every other
    region of which the projection covers min_cover_pct per cent joins the family (include/mimeo_hip.h has the rule).  A bad
    path, region or item is a RuntimeError naming it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_link_regions'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_link_regions: rebuild the library')
    reg = np.asarray(regions)
    if reg.dtype != _ffi.INTERVAL:
        a = np.asarray(reg, dtype=np.uint32).reshape(-1, 3)
        reg = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        reg['chrom'], reg['start'], reg['end'] = a[:, 0], a[:, 1], a[:, 2]
    reg = np.ascontiguousarray(reg)
    it = _window_items(items)
    cot = None
    if chrom_of_tid is not None:
        cot = np.ascontiguousarray(chrom_of_tid, dtype=np.uint32)
        if cot.size != len(A.names):
            raise ValueError('chrom_of_tid has %d entries for %d scaffolds' % (cot.size, len(A.names)))
    if not 0 <= int(min_cover_pct) <= 0xFFFFFFFF:
        raise ValueError('min_cover_pct must be in 1..100, not %r' % (min_cover_pct,))
    family, links = np.zeros(reg.size, dtype=np.uint32), np.zeros(reg.size, dtype=np.uint64)
    _ffi.check(lib.mimeo_link_regions(A._h, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                      blk.ctypes.data if blk.size else None, blk.size, reg.ctypes.data if reg.size else None, reg.size,
                                      cot.ctypes.data if cot is not None else None, it.ctypes.data if it.size else None, it.size,
                                      int(min_cover_pct), family.ctypes.data if reg.size else None, links.ctypes.data if reg.size else None))
    return family, links


def pileup(A, B, records, first, blocks, windows, items, counts=True, call=True):
    """Column pileup of alignment paths and a base called from every column (mimeo_path_pileup, kernel K13): (cols, call) —
    cols one _ffi.PILEUP_COLUMN row per column of every window (what the aligned query strands put on that target base: a, c, g,
    t, n, del, and the insertions in front of it), call one byte per column (the letter with the most votes, the target's own
    base voting once; '-' where deletions outnumber every base; include/mimeo_hip.h "pileup v1" has the rules).  The columns of
    window g start at entry sum(end - start of the windows before it).  records / first / blocks as for path_stats; windows:
    _ffi.PILEUP_WINDOW rows (or an (n, 3) array) of (tid, start, end) on the target's plus strand, overlapping or repeated as
    they come; items: _ffi.WINDOW_ITEM rows (or an (n, 4) array) of (record number, window number, w0, w1) with [w0, w1) inside
    the window.  counts=False / call=False: that array is not computed and None comes back in its place.  A bad path, window or
    item is a RuntimeError naming it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_path_pileup'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_path_pileup: rebuild the library')
    win = np.asarray(windows)
    if win.dtype != _ffi.PILEUP_WINDOW:
        a = np.asarray(win, dtype=np.uint32).reshape(-1, 3)
        win = np.zeros(a.shape[0], dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = a[:, 0], a[:, 1], a[:, 2]
    win = np.ascontiguousarray(win)
    it = _window_items(items)
    # the arrays are sized by what the library will accept: a window with start > end is refused there, before anything is written
    ncols = int(np.maximum(win['end'].astype(np.int64) - win['start'].astype(np.int64), 0).sum())
    cols = np.zeros(ncols, dtype=_ffi.PILEUP_COLUMN) if counts else None
    letters = np.zeros(ncols, dtype=np.uint8) if call else None
    _ffi.check(lib.mimeo_path_pileup(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                     blk.ctypes.data if blk.size else None, blk.size, win.ctypes.data if win.size else None, win.size,
                                     it.ctypes.data if it.size else None, it.size, cols.ctypes.data if counts and ncols else None,
                                     letters.ctypes.data if call and ncols else None))
    return cols, letters


def insertions(A, B, records, first, blocks, windows, items, sites, results=True, counts=True, call=True):
    """The insertion columns of a pileup and a base called from each (mimeo_path_insertions, kernel K14): (res, icols, icall) —
    res one _ffi.INSERT_RESULT row per site (the runs that insert in front of the site's target base, their bases, how many are
    longer than the site's columns, and the longest), icols one _ffi.INSERT_COLUMN row and icall one byte per insertion column
    (the inserted bases piled up left-aligned; the letter where it outvotes everyone who inserts nothing there, '-' otherwise;
    include/mimeo_hip.h "pileup v2, insertion columns" has the rules).  The columns of site s start at entry sum(ncols of the
    sites before it).  records / first / blocks / windows / items exactly as for pileup; sites: _ffi.INSERT_SITE rows (or an
    (n, 4) array) of (window number, x, ncols, voters), strictly increasing by (window, x), as formats.insertion_sites makes
    them.  results=False / counts=False / call=False: that array is not computed and None comes back in its place.  A bad path,
    window, item or site is a RuntimeError naming it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_path_insertions'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_path_insertions: rebuild the library')
    win = np.asarray(windows)
    if win.dtype != _ffi.PILEUP_WINDOW:
        a = np.asarray(win, dtype=np.uint32).reshape(-1, 3)
        win = np.zeros(a.shape[0], dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = a[:, 0], a[:, 1], a[:, 2]
    win = np.ascontiguousarray(win)
    it = _window_items(items)
    st = np.asarray(sites)
    if st.dtype != _ffi.INSERT_SITE:
        a = np.asarray(st, dtype=np.uint32).reshape(-1, 4)
        st = np.zeros(a.shape[0], dtype=_ffi.INSERT_SITE)
        st['window'], st['x'], st['ncols'], st['voters'] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    st = np.ascontiguousarray(st)
    # the arrays are sized by what the library will accept: a site with more than INSERT_MAX_COLS columns is refused there,
    # before anything is written
    nicols = int(np.minimum(st['ncols'].astype(np.int64), _ffi.INSERT_MAX_COLS).sum())
    res = np.zeros(st.size, dtype=_ffi.INSERT_RESULT) if results else None
    icols = np.zeros(nicols, dtype=_ffi.INSERT_COLUMN) if counts else None
    icall = np.full(nicols, ord('-'), dtype=np.uint8) if call else None
    _ffi.check(lib.mimeo_path_insertions(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                         blk.ctypes.data if blk.size else None, blk.size, win.ctypes.data if win.size else None, win.size,
                                         it.ctypes.data if it.size else None, it.size, st.ctypes.data if st.size else None, st.size,
                                         res.ctypes.data if results and st.size else None, icols.ctypes.data if counts and nicols else None,
                                         icall.ctypes.data if call and nicols else None))
    return res, icols, icall


def stack(A, B, records, first, blocks, windows, items, sites):
    """The stacked rows of a pile (mimeo_path_stack, kernel K15): (res, row_first, rows) — row k, rows[row_first[k]:row_first[k + 1]],
    is item k as text in the columns of its window with the insertion columns of the window's sites opened up in front of their
    bases: A C G T N under a block, '-' in a gap of the path, '.' where the item does not reach, a c g t n in an insertion column
    (include/mimeo_hip.h "pileup v3, the stack" has the rules); res one _ffi.STACK_ROW row per item: the stretch [q_lo, q_hi) of
    the aligned query strand that the row shows, its letters, and the inserted bases that have no column.  records / first /
    blocks / windows / items / sites exactly as for insertions (voters is not read; no site at all is legal).  The arrays hold the
    whole call: a caller bounds them by what it asks for at once (workflow.alignment_block).  A bad path, window, item or site
    is a RuntimeError naming it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_path_stack'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_path_stack: rebuild the library')
    win = np.asarray(windows)
    if win.dtype != _ffi.PILEUP_WINDOW:
        a = np.asarray(win, dtype=np.uint32).reshape(-1, 3)
        win = np.zeros(a.shape[0], dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = a[:, 0], a[:, 1], a[:, 2]
    win = np.ascontiguousarray(win)
    it = _window_items(items)
    st = np.asarray(sites)
    if st.dtype != _ffi.INSERT_SITE:
        a = np.asarray(st, dtype=np.uint32).reshape(-1, 4)
        st = np.zeros(a.shape[0], dtype=_ffi.INSERT_SITE)
        st['window'], st['x'], st['ncols'], st['voters'] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    st = np.ascontiguousarray(st)
    res = np.zeros(it.size, dtype=_ffi.STACK_ROW)
    pf, pr = C.c_void_p(), C.c_void_p()
    _ffi.check(lib.mimeo_path_stack(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                    blk.ctypes.data if blk.size else None, blk.size, win.ctypes.data if win.size else None, win.size,
                                    it.ctypes.data if it.size else None, it.size, st.ctypes.data if st.size else None, st.size,
                                    res.ctypes.data if it.size else None, C.byref(pf), C.byref(pr)))
    row_first = _ffi.take(pf, C.c_uint64(it.size + 1), np.dtype('<u8'))
    return res, row_first, _ffi.take(pr, C.c_uint64(int(row_first[-1])), np.dtype(np.uint8))


def call_stats(A, B, records, first, blocks, windows, items, sites, call, icall):
    """The rows of a pile against the call (mimeo_path_call_stats, kernel K16): one _ffi.CALL_STATS row per item — the columns of
    the item's aligned query strand against `call`, the consensus byte per target column of the windows as pileup returns it, and
    at the sites against `icall`, the byte per insertion column as insertions returns it: matches, transitions, transversions and
    ambiguous columns, ins_bases (bases of the copy where the consensus has none), del_bases (letters of the consensus where the
    copy has no base) and the stretch [q_lo, q_hi) of the aligned query strand that stack reports (include/mimeo_hip.h "pileup v4,
    rows against the call" has the rules).  records / first / blocks / windows / items / sites exactly as for stack (voters is not
    read; no site at all is legal, icall is then empty or None).  Every byte of call and icall is one of A C G T N -.  A bad
    path, window, item, site or byte is a RuntimeError naming it, raised before anything runs on the device."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_path_call_stats'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_path_call_stats: rebuild the library')
    win = np.asarray(windows)
    if win.dtype != _ffi.PILEUP_WINDOW:
        a = np.asarray(win, dtype=np.uint32).reshape(-1, 3)
        win = np.zeros(a.shape[0], dtype=_ffi.PILEUP_WINDOW)
        win['tid'], win['start'], win['end'] = a[:, 0], a[:, 1], a[:, 2]
    win = np.ascontiguousarray(win)
    it = _window_items(items)
    st = np.asarray(sites)
    if st.dtype != _ffi.INSERT_SITE:
        a = np.asarray(st, dtype=np.uint32).reshape(-1, 4)
        st = np.zeros(a.shape[0], dtype=_ffi.INSERT_SITE)
        st['window'], st['x'], st['ncols'], st['voters'] = a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    st = np.ascontiguousarray(st)
    as_bytes = lambda b: np.zeros(0, dtype=np.uint8) if b is None else np.ascontiguousarray(np.frombuffer(b, dtype=np.uint8) if isinstance(b, (bytes, bytearray))
                                                                                            else np.asarray(b, dtype=np.uint8))
    cl, icl = as_bytes(call), as_bytes(icall)
    # the library reads as many bytes as the windows and sites have columns: a shorter array never reaches it
    ncols = int(np.maximum(win['end'].astype(np.int64) - win['start'].astype(np.int64), 0).sum())
    nicols = int(np.minimum(st['ncols'].astype(np.int64), _ffi.INSERT_MAX_COLS).sum())
    # (None is NULL to the library, which refuses it where there are columns)
    if (call is not None and cl.size != ncols) or (icall is not None and icl.size != nicols):
        raise ValueError('call_stats: call has %d bytes for %d columns, icall %d for %d insertion columns' % (cl.size, ncols, icl.size, nicols))
    out = np.zeros(it.size, dtype=_ffi.CALL_STATS)
    _ffi.check(lib.mimeo_path_call_stats(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                         blk.ctypes.data if blk.size else None, blk.size, win.ctypes.data if win.size else None, win.size,
                                         it.ctypes.data if it.size else None, it.size, st.ctypes.data if st.size else None, st.size,
                                         cl.ctypes.data if cl.size else None, icl.ctypes.data if icl.size else None, out.ctypes.data if it.size else None))
    return out


def path_text(A, B, records, first, blocks):
    """The text of alignment paths (mimeo_path_text, kernel K11): (row_first, trow, qrow) as numpy arrays (<u8, uint8, uint8).
    Row i is trow[row_first[i]:row_first[i + 1]] over the same range of qrow: the target's letters over the aligned query
    strand's, '-' where the other sequence jumps (insertions before deletions), A C G T and N for everything else — the device
    keeps neither case nor IUPAC codes (include/mimeo_hip.h has the rules).  records / first / blocks and the errors as for
    path_stats.  The arrays hold the whole call: a caller bounds them by what it asks for at once (workflow.text_runs)."""
    recs, first, blk = _paths(records, first, blocks)
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_path_text'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_path_text: rebuild the library')
    pf, pt, pq = C.c_void_p(), C.c_void_p(), C.c_void_p()
    _ffi.check(lib.mimeo_path_text(A._h, B._h if B is not None else None, recs.ctypes.data if recs.size else None, recs.size, first.ctypes.data,
                                   blk.ctypes.data if blk.size else None, blk.size, C.byref(pf), C.byref(pt), C.byref(pq)))
    row_first = _ffi.take(pf, C.c_uint64(recs.size + 1), np.dtype('<u8'))
    total = C.c_uint64(int(row_first[-1]))
    return row_first, _ffi.take(pt, total, np.dtype(np.uint8)), _ffi.take(pq, total, np.dtype(np.uint8))


def terminal_repeats(A, intervals, **params):
    """Terminal repeats of features (mimeo_terminal_repeats, kernel K17): for every (scaffold id, start, end) of genome A a full
    affine-gap local alignment of its first w bases against its last w bases (record 2k, qstrand 0: a direct repeat, the LTRs of a
    retrotransposon) and against the reverse complement of the last w bases (record 2k + 1, qstrand 1: an inverted repeat, the
    TIRs of a DNA transposon), w = min(window, length // 2).  Returns (records[2n], first[2n + 1], blocks) in the dtypes of
    align_pairs(..., paths=True), so path_stats, path_text and formats.cigar take them as they are; an orientation that scores
    below min_score is a record of zeros (but tid, qid, qstrand) with an empty path.  params: window (1024; 1 .. 4096), match (2),
    mismatch (3), gap_open (5), gap_extend (2), min_score (40) — include/mimeo_hip.h has the rules, ties included.  A bad
    parameter or item is a RuntimeError naming it, raised before anything runs on the device."""
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_terminal_repeats'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_terminal_repeats: rebuild the library')
    P = _ffi.TerminalParams()
    _ffi.check(lib.mimeo_terminal_params_default(C.byref(P)))
    for k, v in params.items():
        if k not in _ffi.TerminalParams.NAMES:
            raise TypeError('unknown terminal-repeat parameter %r' % k)
        setattr(P, k, int(v))
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    iv = np.ascontiguousarray(iv)
    recs = np.zeros(2 * iv.size, dtype=_ffi.ALIGNMENT)
    pf, pb, nb = C.c_void_p(), C.c_void_p(), C.c_uint64()
    _ffi.check(lib.mimeo_terminal_repeats(A._h, iv.ctypes.data if iv.size else None, iv.size, C.byref(P), recs.ctypes.data if iv.size else None,
                                          C.byref(pf), C.byref(pb), C.byref(nb)))
    return recs, _ffi.take(pf, C.c_uint64(2 * iv.size + 1), np.dtype('<u8')), _ffi.take(pb, nb, _ffi.PATH_BLOCK)


def _intervals(intervals):
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    return np.ascontiguousarray(iv)


def flank_repeats(A, intervals, **params):
    """Flank repeats (mimeo_flank_repeats, kernel K18): for every (scaffold id, start, end) of genome A the target-site duplication
    of the element — the direct repeat of min_len .. max_len bases immediately outside its two ends, either end free to move by
    up to `slack` bases.  Returns one record of _ffi.FLANK_REPEAT per interval: the two copies [left_start, left_start + len) and
    [right_start, right_start + len), mismatches, and dl, dr: the element is [start + dl, end + dr); all zero (len 0) where there
    is none.  params: min_len (4; 2 .. 32), max_len (20; min_len .. 32), slack (2; 0 .. 8), max_mismatch (0; 0 .. 2) —
    include/mimeo_hip.h has the rules, ties included.  A bad parameter or item is a RuntimeError naming it, raised before anything
    runs on the device."""
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_flank_repeats'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_flank_repeats: rebuild the library')
    P = _ffi.FlankParams()
    _ffi.check(lib.mimeo_flank_params_default(C.byref(P)))
    for k, v in params.items():
        if k not in _ffi.FlankParams.NAMES:
            raise TypeError('unknown flank-repeat parameter %r' % k)
        setattr(P, k, int(v))
    iv = _intervals(intervals)
    out = np.zeros(iv.size, dtype=_ffi.FLANK_REPEAT)
    _ffi.check(lib.mimeo_flank_repeats(A._h, iv.ctypes.data if iv.size else None, iv.size, C.byref(P), out.ctypes.data if iv.size else None))
    return out


def open_frames(A, intervals):
    """Open frames (mimeo_open_frames, kernel K19): for every (scaffold id, start, end) of genome A and each of its six reading
    frames the longest run of codons without a stop and without a non-ACGT base.  Returns an array of shape (n, 6) of
    _ffi.OPEN_FRAME, column 3 * strand + frame (strand 1: the reverse complement; frame: the offset of the first codon from the
    interval's 5' end on that strand): start, end on the plus strand, codons, and met — the index within the run of its first ATG,
    codons where it has none; all zero for a frame without an open codon.  include/mimeo_hip.h has the rules.  A bad item is a
    RuntimeError naming it, raised before anything runs on the device."""
    lib = _ffi.load()
    if not hasattr(lib, 'mimeo_open_frames'):
        raise RuntimeError('libmimeo_hip.so has no mimeo_open_frames: rebuild the library')
    iv = _intervals(intervals)
    out = np.zeros((iv.size, 6), dtype=_ffi.OPEN_FRAME)
    _ffi.check(lib.mimeo_open_frames(A._h, iv.ctypes.data if iv.size else None, iv.size, 0, out.ctypes.data if iv.size else None))
    return out


def failed_pairs():
    """Pairs of the last align_pairs / align_units call that hit a documented limit and were left out (the reference's script
    loses only the failing lastz run's rows: utils.py:125-128): [(index into the call's pair list, error code)]."""
    lib = _ffi.load()
    n = C.c_uint64()
    _ffi.check(lib.mimeo_get_failed_pairs(None, None, 0, C.byref(n)))
    if not n.value:
        return []
    idx = np.zeros(n.value, dtype=np.uint64)
    code = np.zeros(n.value, dtype=np.int32)
    _ffi.check(lib.mimeo_get_failed_pairs(idx.ctypes.data, code.ctypes.data, n.value, C.byref(n)))
    return list(zip(idx.tolist(), code.tolist()))


def last_error():
    return _ffi.load().mimeo_last_error().decode()


def coverage_collapse(intervals, chrom_len, min_cov, min_len):
    """intervals: structured array (_ffi.INTERVAL) or (n,3) ints of (chrom id, start, end)."""
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    iv = np.ascontiguousarray(iv)
    cl = np.ascontiguousarray(chrom_len, dtype=np.uint32)
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_coverage_collapse(iv.ctypes.data if iv.size else None, iv.size, cl.ctypes.data,
                                                   cl.size, int(min_cov), int(min_len), C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.INTERVAL)


def coverage_bedgraph(intervals, chrom_len):
    """bedtools genomecov -bg: maximal runs of equal depth > 0 (records of _ffi.DEPTH_RUN, in chrom / start order)."""
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    iv = np.ascontiguousarray(iv)
    cl = np.ascontiguousarray(chrom_len, dtype=np.uint32)
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_coverage_bedgraph(iv.ctypes.data if iv.size else None, iv.size, cl.ctypes.data, cl.size,
                                                   C.byref(ptr), C.byref(n)))
    return _ffi.take(ptr, n, _ffi.DEPTH_RUN)


def tandem_masked(A, intervals, match=2, mismatch=7, minscore=50, maxperiod=50, delta=7):
    """Bases of each (scaffold id, start, end) slice of genome A marked by the tandem scorer (K8)."""
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    iv = np.ascontiguousarray(iv)
    out = np.zeros(iv.size, dtype=np.uint32)
    if iv.size:
        _ffi.check(_ffi.load().mimeo_tandem_masked(A._h, iv.ctypes.data, iv.size, int(match), int(mismatch), int(delta),
                                                   int(minscore), int(maxperiod), out.ctypes.data))
    return out


def tandem_mask(A, intervals, match=2, mismatch=7, minscore=50, maxperiod=50, delta=7, counts=False):
    """The positions behind tandem_masked, from the same device call: one bool array per slice, as long as the slice
    clipped to its scaffold (empty for an empty or inverted slice); element i says whether base start + i is marked.
    counts=True: (masks, the uint32 counts the device summed from the same words)."""
    iv = np.asarray(intervals)
    if iv.dtype != _ffi.INTERVAL:
        a = np.asarray(iv, dtype=np.uint32).reshape(-1, 3)
        iv = np.zeros(a.shape[0], dtype=_ffi.INTERVAL)
        iv['chrom'], iv['start'], iv['end'] = a[:, 0], a[:, 1], a[:, 2]
    iv = np.ascontiguousarray(iv)
    out = np.zeros(iv.size, dtype=np.uint32)
    ptr, n = C.c_void_p(), C.c_uint64()
    _ffi.check(_ffi.load().mimeo_tandem_mask(A._h, iv.ctypes.data if iv.size else None, iv.size, int(match), int(mismatch), int(delta),
                                             int(minscore), int(maxperiod), out.ctypes.data if iv.size else None, C.byref(ptr),
                                             C.byref(n)))
    words = _ffi.take(ptr, n, np.dtype('<u4'))
    masks, w = [], 0
    for c, s, e in iv.tolist():
        ln = max(0, min(e, A.lengths[c]) - s)
        nw = (ln + 31) // 32
        bits = np.unpackbits(words[w:w + nw].view(np.uint8), bitorder='little')
        if bits[ln:].any():
            raise RuntimeError('tandem scorer: a slice mask has bits beyond its slice')
        masks.append(bits[:ln].astype(bool))
        w += nw
    if w != words.size:
        raise RuntimeError('tandem scorer: %d mask words for slices of %d' % (words.size, w))
    return (masks, out) if counts else masks
