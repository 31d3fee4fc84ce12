// insert_host.h — HIP-free host side of mimeo_path_insertions (K14, k14_insertions.hip): the checks on the sites (the paths, the
// windows and the items are checked as for mimeo_path_pileup, under this entry point's name), the prefix sum of the sites'
// insertion columns, the cut of the sites into tiles and of the tiles into batches of a bounded number of columns, the
// distribution of a slice's items over the site tiles they touch (a CSR of tile -> (alignment, run of sites)), and the cut of a
// tile's entries into the kernel's jobs.  Kept apart from the device code so that it runs under the CPU sanitizers
// (tests/sanitize/insert_check.cc, tests/test_host_insertions.py).  The items go to the slices of path_stats_host::plan_slices
// with window_stats_host::bucket_items, as for K13.
#pragma once
#include <algorithm>

#include "pileup_host.h"

namespace mimeo {
namespace insert_host {

constexpr const char *NAME = "mimeo_path_insertions";
// Insertion columns of one site, at most.  Ample: with the default gap penalties and y-drop (gap_open 400, gap_extend 30, ydrop
// 9400) a single gap run that the gapped extension survives is at most about (ydrop - gap_open) / gap_extend = 300 bases.  With
// other parameters a longer run is truncated to the site's columns and counted in mimeo_insert_result.longer.
constexpr uint32_t INSERT_MAX_COLS = 1024;
constexpr uint32_t TILE_COLS = 1024;                 // insertion columns of a site tile, at most: five counter planes of 4 KiB in LDS
constexpr uint32_t JOB_ITEMS = 64;                   // entries of a job, at most (default; below 65 536: Job::nitems)
constexpr uint64_t MAX_BATCH_COLUMNS = 1ull << 28;   // a job numbers the columns of its batch in 32 bits, five counters each
static_assert(INSERT_MAX_COLS <= TILE_COLS, "a site is never split: it fits a tile");

// The sites against the windows, which have passed their checks.  `name`: the entry point the message starts with
// (mimeo_path_stack, stack_host.h, makes the same checks under its own name).
inline bool validate_sites(const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_insert_site *sites, uint64_t nsites, std::string *msg,
                           const char *name = NAME) {
    char buf[320];
    auto fail = [&](uint64_t s, const char *what) {
        snprintf(buf, sizeof buf, "%s: site %llu (window %u, x %u, ncols %u): %s", name, (unsigned long long)s, sites[s].window, sites[s].x, sites[s].ncols, what);
        *msg = buf;
        return false;
    };
    if (!nsites) return true;
    if (!sites) { *msg = std::string(name) + ": null argument"; return false; }
    if (nsites > 0xFFFFFFFFull) { *msg = std::string(name) + ": more than 2^32 - 1 sites"; return false; }
    for (uint64_t s = 0; s < nsites; s++) {
        const mimeo_insert_site &v = sites[s];
        if (v.window >= nwin) return fail(s, "window is not below nwin");
        if (v.x < windows[v.window].start || v.x >= windows[v.window].end) return fail(s, "x does not lie inside the window");
        if (v.ncols < 1 || v.ncols > INSERT_MAX_COLS) return fail(s, "ncols is not in 1 .. 1024");
        if (s && (v.window < sites[s - 1].window || (v.window == sites[s - 1].window && v.x <= sites[s - 1].x)))
            return fail(s, "the sites are not strictly increasing by (window, x)");
    }
    return true;
}

// Every check of mimeo_path_insertions, in the order the messages are promised: the paths, the windows, the items — those of
// mimeo_path_pileup — and then the sites.
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                     uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, std::string *msg,
                     uint64_t max_window_items = pileup_host::MAX_WINDOW_ITEMS, const char *name = NAME) {
    return path_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, msg, name) && pileup_host::validate_windows(len_t, windows, nwin, msg, name) &&
           pileup_host::validate_items(aln, n, windows, nwin, items, nitems, msg, max_window_items, name) && validate_sites(windows, nwin, sites, nsites, msg, name);
}

// One site tile: the consecutive sites [site0, site0 + nsites) of one window, whose columns are the entries
// [icol0, icol0 + ncols) of the call, ncols <= tile_cols.
struct SiteTile { uint64_t site0, icol0; uint32_t nsites, ncols, window; };

// The sites of the call as the planner sees them.  icol_first[s]: the entry of site s's first column in icols / icall (the
// prefix sum of ncols in 64 bits, nsites + 1 entries).  win_first[g] .. win_first[g + 1]: the sites of window g (nwin + 1
// entries; the sites are sorted by window).  tiles: runs of consecutive sites of one window whose ncols sum to at most
// tile_cols; a site is never split (ncols <= INSERT_MAX_COLS <= tile_cols), and a tile is as long as it can be.
struct Sites {
    uint32_t tile_cols = TILE_COLS;
    std::vector<uint64_t> icol_first, win_first;
    std::vector<SiteTile> tiles;
    uint64_t nicols() const { return icol_first.back(); }
    uint64_t nsites() const { return icol_first.size() - 1; }
};
inline Sites plan_sites(const mimeo_insert_site *sites, uint64_t nsites, uint64_t nwin, uint32_t tile_cols = TILE_COLS) {
    Sites p;
    p.tile_cols = tile_cols;
    p.icol_first.assign(nsites + 1, 0);
    p.win_first.assign(nwin + 1, 0);
    for (uint64_t s = 0; s < nsites; s++) {
        p.icol_first[s + 1] = p.icol_first[s] + sites[s].ncols;
        p.win_first[(uint64_t)sites[s].window + 1]++;
        if (p.tiles.empty() || p.tiles.back().window != sites[s].window || p.tiles.back().ncols + sites[s].ncols > tile_cols)
            p.tiles.push_back(SiteTile{s, p.icol_first[s], 0, 0, sites[s].window});
        p.tiles.back().nsites++;
        p.tiles.back().ncols += sites[s].ncols;
    }
    for (uint64_t g = 0; g < nwin; g++) p.win_first[g + 1] += p.win_first[g];
    return p;
}

// A batch: the consecutive tiles [tile0, tile1): the sites [site0, site0 + nsites) and the columns [icol0, icol0 + ncols) of
// the call.  Tiles are added while the columns stay at most max_columns; the first tile goes in whatever its size.
struct Batch { uint64_t tile0 = 0, tile1 = 0, site0 = 0, nsites = 0, icol0 = 0, ncols = 0; };
inline Batch plan_batch(const Sites &p, uint64_t tile0, uint64_t max_columns) {
    Batch b;
    b.tile0 = b.tile1 = tile0;
    b.site0 = p.tiles[tile0].site0;
    b.icol0 = p.tiles[tile0].icol0;
    while (b.tile1 < p.tiles.size() && (b.tile1 == tile0 || b.ncols + p.tiles[b.tile1].ncols <= max_columns)) {
        b.ncols += p.tiles[b.tile1].ncols;
        b.nsites += p.tiles[b.tile1].nsites;
        b.tile1++;
    }
    return b;
}

// A site as the kernels see it: target base x, the entry `off` of its first column in the BATCH, its columns and its voters.
struct SiteDesc { uint32_t x, off, ncols, voters; };
inline void batch_sites(const Sites &p, const Batch &b, const mimeo_insert_site *sites, std::vector<SiteDesc> &out) {
    out.resize(b.nsites);
    for (uint64_t s = 0; s < b.nsites; s++)
        out[s] = SiteDesc{sites[b.site0 + s].x, (uint32_t)(p.icol_first[b.site0 + s] - b.icol0), sites[b.site0 + s].ncols, sites[b.site0 + s].voters};
}

// An item on one site tile: the path of alignment `aln` (index inside the slice), which has at least one block, asked about the
// sites [s0, s1) of the BATCH — never empty, all of one tile, and every x of them inside the item's window clipped to the
// alignment's own [first block's t, last block's end): the kernel's block search relies on it.
struct Entry { uint32_t aln, s0, s1; };

// CSR of tile -> entries for one batch: the entries of tile tile0 + k are entries[start[k] .. start[k + 1]).
struct TileItems {
    std::vector<uint64_t> start;
    std::vector<Entry> entries;
};

// The sites [s0, s1) of the call that item `it`, clipped to its alignment, holds: two binary searches over the sorted sites of
// its window.  false where there is none (the window misses the alignment, is empty, has no site there, or the alignment has no
// block: an insertion run lies between two blocks, so what lies outside [first block's t, last block's end) holds none).
inline bool item_sites(const Sites &p, const uint64_t *first, const mimeo_path_block *blocks, const mimeo_insert_site *sites, const mimeo_window_item &it,
                       uint64_t *s0, uint64_t *s1) {
    const uint64_t b0 = first[it.aln], b1 = first[(uint64_t)it.aln + 1];
    if (b0 == b1) return false;
    const uint64_t lo = blocks[b0].t, hi = (uint64_t)blocks[b1 - 1].t + blocks[b1 - 1].len;   // hi <= the scaffold's length < 2^32
    const uint64_t w0 = std::max<uint64_t>(it.w0, lo), w1 = std::min<uint64_t>(it.w1, hi);
    if (w0 >= w1) return false;
    const mimeo_insert_site *f = sites + p.win_first[it.group], *l = sites + p.win_first[(uint64_t)it.group + 1];
    auto below = [](const mimeo_insert_site &s, uint64_t x) { return s.x < x; };
    *s0 = (uint64_t)(std::lower_bound(f, l, w0, below) - sites);
    *s1 = (uint64_t)(std::lower_bound(f, l, w1, below) - sites);
    return *s0 < *s1;
}

// The items order[i0 .. i1), all of alignments of the slice that begins at alignment a0, onto the tiles of batch b: every item
// makes one entry per tile of the batch of whose sites it holds some, in the order of the items.  At most max_entries entries
// are made (an item is never split over two calls; the first one goes in whatever it makes): returns the number i_end <= i1 of
// the first item that was not taken, so that a caller works a slice off in runs of bounded size.
inline uint64_t bucket_tiles(const Sites &p, const Batch &b, const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0, const mimeo_insert_site *sites,
                             const mimeo_window_item *items, const uint64_t *order, uint64_t i0, uint64_t i1, uint64_t max_entries, TileItems &out) {
    const uint64_t nt = b.tile1 - b.tile0;
    out.start.assign(nt + 1, 0);
    out.entries.clear();
    // the item's sites inside the batch [s0, s1) and the batch's tiles [lo, hi) (numbers inside the batch) that hold them
    auto range = [&](const mimeo_window_item &it, uint64_t *s0, uint64_t *s1, uint64_t *lo, uint64_t *hi) {
        if (!item_sites(p, first, blocks, sites, it, s0, s1)) return false;
        *s0 = std::max(*s0, b.site0);
        *s1 = std::min(*s1, b.site0 + b.nsites);
        if (*s0 >= *s1) return false;
        auto starts_behind = [](uint64_t s, const SiteTile &t) { return s < t.site0; };
        const SiteTile *tf = p.tiles.data() + b.tile0, *tl = p.tiles.data() + b.tile1;
        *lo = (uint64_t)(std::upper_bound(tf, tl, *s0, starts_behind) - tf) - 1;   // the tile that holds site s0
        *hi = (uint64_t)(std::upper_bound(tf, tl, *s1 - 1, starts_behind) - tf);   // behind the tile that holds site s1 - 1
        return true;
    };
    uint64_t total = 0, i_end = i0, s0, s1, lo, hi;
    for (; i_end < i1; i_end++) {
        if (!range(items[order[i_end]], &s0, &s1, &lo, &hi)) continue;
        if (total && total + (hi - lo) > max_entries) break;
        total += hi - lo;
        for (uint64_t k = lo; k < hi; k++) out.start[k + 1]++;
    }
    for (uint64_t k = 0; k < nt; k++) out.start[k + 1] += out.start[k];
    out.entries.resize(total);
    std::vector<uint64_t> at(out.start.begin(), out.start.end() - 1);
    for (uint64_t i = i0; i < i_end; i++) {
        const mimeo_window_item &it = items[order[i]];
        if (!range(it, &s0, &s1, &lo, &hi)) continue;
        for (uint64_t k = lo; k < hi; k++) {
            const SiteTile &t = p.tiles[b.tile0 + k];
            out.entries[at[k]++] = Entry{(uint32_t)(it.aln - a0), (uint32_t)(std::max(s0, t.site0) - b.site0), (uint32_t)(std::min(s1, t.site0 + t.nsites) - b.site0)};
        }
    }
    return i_end;
}

// One job = one workgroup of the kernel: the tile whose sites are [site0, site0 + nsites) of the batch and whose columns are the
// entries [icol0, icol0 + ncols) of the batch, and the run [item0, item0 + nitems) of the entries of TileItems.
struct Job { uint32_t site0, icol0, item0; uint16_t nsites, ncols, nitems; };

// The jobs of a batch's tiles: a tile with entries makes ceil(entries / job_items) jobs of at most job_items consecutive
// entries (1 .. 65 535; anything else is JOB_ITEMS); a tile without entries makes none.
inline void plan_jobs(const Sites &p, const Batch &b, const TileItems &ti, uint64_t job_items, std::vector<Job> &jobs) {
    jobs.clear();
    if (job_items < 1 || job_items > 0xFFFFu) job_items = JOB_ITEMS;
    for (size_t k = 0; k + 1 < ti.start.size(); k++) {
        const SiteTile &t = p.tiles[b.tile0 + k];
        for (uint64_t e = ti.start[k]; e < ti.start[k + 1]; e += job_items)
            jobs.push_back(Job{(uint32_t)(t.site0 - b.site0), (uint32_t)(t.icol0 - b.icol0), (uint32_t)e, (uint16_t)t.nsites, (uint16_t)t.ncols,
                               (uint16_t)std::min(job_items, ti.start[k + 1] - e)});
    }
}

}  // namespace insert_host
}  // namespace mimeo
