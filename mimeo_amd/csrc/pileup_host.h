// pileup_host.h — HIP-free host side of mimeo_path_pileup (K13, k13_pileup.hip): the checks on the windows and the items, the
// cut of the windows into tiles and of the tiles into batches of a bounded number of columns, the distribution of a slice's
// items over the tiles they touch (a CSR of tile -> clipped items), and the cut of a tile's items into the kernel's jobs.  Kept
// apart from the device code so that it runs under the CPU sanitizers (tests/sanitize/pileup_check.cc,
// tests/test_host_pileup.py).  The paths are checked by path_stats_host::validate, the items go to the slices of
// path_stats_host::plan_slices with window_stats_host::bucket_items.
#pragma once
#include <algorithm>

#include "window_stats_host.h"

namespace mimeo {
namespace pileup_host {

constexpr const char *NAME = "mimeo_path_pileup";
constexpr uint32_t TILE = 1024;                      // columns of a tile: 8 counters x 4 bytes x 1024 = 32 KiB of LDS
constexpr uint32_t JOB_ITEMS = 64;                   // items of a job, at most (default; below 65 536: Job::nitems)
constexpr uint64_t MAX_BATCH_COLUMNS = 1ull << 28;   // a job numbers the columns of its batch in 32 bits, eight counters each
constexpr uint64_t MAX_WINDOW_ITEMS = 0xFFFFFFFFull; // items that may name one window: the counters are 32 bits

// The windows against the target scaffolds.  `name`: the entry point the message starts with (mimeo_path_insertions,
// insert_host.h, makes the same checks under its own name).
inline bool validate_windows(const std::vector<uint64_t> &len_t, const mimeo_pileup_window *windows, uint64_t nwin, std::string *msg, const char *name = NAME) {
    char buf[320];
    auto fail = [&](uint64_t g, const char *what) {
        snprintf(buf, sizeof buf, "%s: window %llu (tid %u, [%u, %u)): %s", name, (unsigned long long)g, windows[g].tid, windows[g].start, windows[g].end, what);
        *msg = buf;
        return false;
    };
    if (!nwin) return true;
    if (!windows) { *msg = std::string(name) + ": null argument"; return false; }
    if (nwin > 0xFFFFFFFFull) { *msg = std::string(name) + ": more than 2^32 - 1 windows"; return false; }
    for (uint64_t g = 0; g < nwin; g++) {
        const mimeo_pileup_window &w = windows[g];
        if (w.tid >= len_t.size()) return fail(g, "tid is not a scaffold of the target genome");
        if (w.start > w.end) return fail(g, "start is beyond end");
        if (w.end > len_t[w.tid]) return fail(g, "end is beyond its scaffold");
    }
    return true;
}

// The items against the records and the windows; the paths and the windows have passed their checks.  max_window_items: a
// window that more items name is refused (a counter of one of its columns could wrap).
inline bool validate_items(const mimeo_alignment *aln, uint64_t n, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                           uint64_t nitems, std::string *msg, uint64_t max_window_items = MAX_WINDOW_ITEMS, const char *name = NAME) {
    char buf[320];
    auto fail = [&](uint64_t i, const char *what) {
        const mimeo_window_item &it = items[i];
        snprintf(buf, sizeof buf, "%s: item %llu (aln %u, window %u, [%u, %u)): %s", name, (unsigned long long)i, it.aln, it.group, it.w0, it.w1, what);
        *msg = buf;
        return false;
    };
    if (!nitems) return true;
    if (!items || (n && !aln)) { *msg = std::string(name) + ": null argument"; return false; }
    for (uint64_t i = 0; i < nitems; i++) {
        const mimeo_window_item &it = items[i];
        if (it.aln >= n) return fail(i, "aln is not a record of the call");
        if (it.group >= nwin) return fail(i, "window is not below nwin");
        const mimeo_pileup_window &w = windows[it.group];
        if (w.tid != aln[it.aln].tid) return fail(i, "the window does not lie on the record's target scaffold");
        if (it.w0 > it.w1) return fail(i, "w0 is beyond w1");
        if (it.w0 < w.start || it.w1 > w.end) return fail(i, "[w0, w1) does not lie inside the window");
    }
    if (nitems > max_window_items) {   // only then can a window have too many
        std::vector<uint64_t> per(nwin, 0);
        for (uint64_t i = 0; i < nitems; i++)
            if (++per[items[i].group] > max_window_items) {
                snprintf(buf, sizeof buf, "%s: window %u (tid %u, [%u, %u)): more than %llu items name it (item %llu): the counters are 32 bits", name,
                         items[i].group, windows[items[i].group].tid, windows[items[i].group].start, windows[items[i].group].end,
                         (unsigned long long)max_window_items, (unsigned long long)i);
                *msg = buf;
                return false;
            }
    }
    return true;
}

// Every check of mimeo_path_pileup, in the order the messages are promised: the paths, the windows, the items.
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                     uint64_t nitems, std::string *msg, uint64_t max_window_items = MAX_WINDOW_ITEMS) {
    return path_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, msg, NAME) && validate_windows(len_t, windows, nwin, msg) &&
           validate_items(aln, n, windows, nwin, items, nitems, msg, max_window_items);
}

// The tiles of the call.  Window g is cut into ceil((end - start) / tile) tiles of `tile` columns (its last one may be shorter;
// an empty window has none); they are numbered window by window: tile_first[g] .. tile_first[g + 1].  col_first[g]: the entry of
// the window's first column in the call's arrays, col_first[nwin] = ncols.  Both have nwin + 1 entries, in 64 bits.
struct Tiles {
    uint32_t tile = TILE;
    std::vector<uint64_t> col_first, tile_first;
    uint64_t ncols() const { return col_first.back(); }
    uint64_t ntiles() const { return tile_first.back(); }
};
inline Tiles plan_tiles(const mimeo_pileup_window *windows, uint64_t nwin, uint32_t tile = TILE) {
    Tiles t;
    t.tile = tile;
    t.col_first.assign(nwin + 1, 0);
    t.tile_first.assign(nwin + 1, 0);
    for (uint64_t g = 0; g < nwin; g++) {
        const uint64_t len = (uint64_t)windows[g].end - windows[g].start;
        t.col_first[g + 1] = t.col_first[g] + len;
        t.tile_first[g + 1] = t.tile_first[g] + (len + tile - 1) / tile;
    }
    return t;
}

// One tile as the call kernel sees it: columns [t0, t0 + ncols) of scaffold tid; its first column is entry col0 of the BATCH.
struct TileDesc { uint32_t tid, t0, col0, ncols; };

// A batch: the consecutive tiles [tile0, tile1), of the windows [win0, win1) (the first and the last may be shared with the
// neighbouring batches), whose columns are the entries [col0, col0 + ncols) of the call: consecutive tiles are consecutive
// columns.  desc[k]: tile tile0 + k.
struct Batch {
    uint64_t tile0 = 0, tile1 = 0, win0 = 0, win1 = 0, col0 = 0, ncols = 0;
    std::vector<TileDesc> desc;
};
// The batch that starts at tile `tile0` (< ntiles) of window `win0` (the window that holds it): tiles are added while the columns
// stay at most max_columns; the first tile goes in whatever its size.
inline Batch plan_batch(const Tiles &t, const mimeo_pileup_window *windows, uint64_t nwin, uint64_t win0, uint64_t tile0, uint64_t max_columns) {
    Batch b;
    b.tile0 = tile0;
    b.win0 = win0;
    uint64_t g = win0, k = tile0 - t.tile_first[win0];   // the next tile: number k of window g
    b.col0 = t.col_first[g] + k * t.tile;
    while (g < nwin) {
        const uint64_t nk = t.tile_first[g + 1] - t.tile_first[g];
        if (k >= nk) { g++; k = 0; continue; }
        const uint64_t s = (uint64_t)windows[g].start + k * t.tile;
        const uint32_t nc = (uint32_t)std::min<uint64_t>(t.tile, windows[g].end - s);
        if (!b.desc.empty() && b.ncols + nc > max_columns) break;
        b.desc.push_back(TileDesc{windows[g].tid, (uint32_t)s, (uint32_t)b.ncols, nc});
        b.ncols += nc;
        b.win1 = g + 1;
        k++;
    }
    b.tile1 = b.tile0 + b.desc.size();
    return b;
}

// An item clipped to one tile: the path of alignment `aln` (index inside the slice), which has at least one block, over the
// target bases [w0, w1) — never empty, inside the tile and inside the alignment's own [first block's t, last block's end): the
// kernel's block search relies on it.
struct Entry { uint32_t aln, w0, w1; };

// CSR of tile -> entries for one batch: the entries of tile tile0 + k are entries[start[k] .. start[k + 1]).
struct TileItems {
    std::vector<uint64_t> start;
    std::vector<Entry> entries;
};

// The tiles [k0, k1) of its window (numbers inside the window) that item `it`, clipped to its alignment, touches, and the clipped
// [w0, w1); false where nothing is left (the window misses the alignment, is empty, or the alignment has no block: every gap of
// a path starts and ends inside it, so what lies outside counts nothing).
inline bool item_tiles(const uint64_t *first, const mimeo_path_block *blocks, const mimeo_pileup_window &w, const mimeo_window_item &it, uint32_t tile,
                       uint64_t *w0, uint64_t *w1, uint64_t *k0, uint64_t *k1) {
    const uint64_t b0 = first[it.aln], b1 = first[(uint64_t)it.aln + 1];
    if (b0 == b1) return false;
    const uint64_t lo = blocks[b0].t, hi = (uint64_t)blocks[b1 - 1].t + blocks[b1 - 1].len;   // hi <= the scaffold's length < 2^32
    *w0 = std::max<uint64_t>(it.w0, lo);
    *w1 = std::min<uint64_t>(it.w1, hi);
    if (*w0 >= *w1) return false;
    *k0 = (*w0 - w.start) / tile;
    *k1 = (*w1 - 1 - w.start) / tile + 1;
    return true;
}

// The items order[i0 .. i1), all of alignments of the slice that begins at alignment a0, onto the tiles of batch b: every item
// makes one entry per tile of the batch that its clipped window touches, clipped to the tile, in the order of the items.  At most
// max_entries entries are made (an item is never split over two calls; the first one goes in whatever it makes): returns the
// number i_end <= i1 of the first item that was not taken, so that a caller works a slice off in runs of bounded size.
inline uint64_t bucket_tiles(const Tiles &t, const Batch &b, const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0,
                             const mimeo_pileup_window *windows, const mimeo_window_item *items, const uint64_t *order, uint64_t i0, uint64_t i1,
                             uint64_t max_entries, TileItems &out) {
    const uint64_t nt = b.tile1 - b.tile0;
    out.start.assign(nt + 1, 0);
    out.entries.clear();
    // the range of the batch's tiles that an item touches: [lo, hi) as numbers inside the batch
    auto range = [&](const mimeo_window_item &it, uint64_t *w0, uint64_t *w1, uint64_t *lo, uint64_t *hi) {
        if (it.group < b.win0 || it.group >= b.win1) return false;
        uint64_t k0, k1;
        if (!item_tiles(first, blocks, windows[it.group], it, t.tile, w0, w1, &k0, &k1)) return false;
        const uint64_t g0 = t.tile_first[it.group] + k0, g1 = t.tile_first[it.group] + k1;
        *lo = std::max(g0, b.tile0) - b.tile0;
        *hi = std::min(g1, b.tile1) - b.tile0;
        return g0 < b.tile1 && g1 > b.tile0;
    };
    uint64_t total = 0, i_end = i0, w0, w1, lo, hi;
    for (; i_end < i1; i_end++) {
        if (!range(items[order[i_end]], &w0, &w1, &lo, &hi)) continue;
        if (total && total + (hi - lo) > max_entries) break;
        total += hi - lo;
        for (uint64_t k = lo; k < hi; k++) out.start[k + 1]++;
    }
    for (uint64_t k = 0; k < nt; k++) out.start[k + 1] += out.start[k];
    out.entries.resize(total);
    std::vector<uint64_t> at(out.start.begin(), out.start.end() - 1);
    for (uint64_t i = i0; i < i_end; i++) {
        const mimeo_window_item &it = items[order[i]];
        if (!range(it, &w0, &w1, &lo, &hi)) continue;
        for (uint64_t k = lo; k < hi; k++) {
            const TileDesc &d = b.desc[k];
            out.entries[at[k]++] = Entry{(uint32_t)(it.aln - a0), (uint32_t)std::max<uint64_t>(w0, d.t0), (uint32_t)std::min<uint64_t>(w1, (uint64_t)d.t0 + d.ncols)};
        }
    }
    return i_end;
}

// One job = one workgroup of the kernel: the tile whose columns [t0, t0 + ncols) are the entries [col0, col0 + ncols) of the
// batch, and the run [item0, item0 + nitems) of the entries of TileItems.
struct Job { uint32_t t0, col0, item0; uint16_t ncols, nitems; };

// The jobs of a batch's tiles: a tile with entries makes ceil(entries / job_items) jobs of at most job_items consecutive
// entries (1 .. 65 535; anything else is JOB_ITEMS); a tile without entries makes none.
inline void plan_jobs(const Batch &b, const TileItems &ti, uint64_t job_items, std::vector<Job> &jobs) {
    jobs.clear();
    if (job_items < 1 || job_items > 0xFFFFu) job_items = JOB_ITEMS;
    for (size_t k = 0; k + 1 < ti.start.size(); k++)
        for (uint64_t e = ti.start[k]; e < ti.start[k + 1]; e += job_items)
            jobs.push_back(Job{b.desc[k].t0, b.desc[k].col0, (uint32_t)e, (uint16_t)b.desc[k].ncols, (uint16_t)std::min(job_items, ti.start[k + 1] - e)});
}

}  // namespace pileup_host
}  // namespace mimeo
