// stack_host.h — HIP-free host side of mimeo_path_stack (K15, k15_stack.hip): the checks (those of mimeo_path_insertions, under
// this entry point's name), the column layout of every window with its sites' insertion columns opened up (the prefix the
// kernel searches, the analogue of K11's bcol), the rows' offsets in the output, the query stretch of an item, and the cut of a
// slice's rows into device batches of bounded bytes and into the kernel's jobs of a bounded number of columns.  Kept apart from
// the device code so that it runs under the CPU sanitizers (tests/sanitize/stack_check.cc, tests/test_host_stack.py).  The
// items go to the slices of path_stats_host::plan_slices with window_stats_host::bucket_items, as for K13 and K14.
#pragma once
#include <algorithm>

#include "insert_host.h"

namespace mimeo {
namespace stack_host {

constexpr const char *NAME = "mimeo_path_stack";
constexpr uint64_t DEFAULT_BATCH_BYTES = 1ull << 28;   // row bytes of one device batch; a row goes in whole whatever its size
constexpr uint64_t DEFAULT_JOB_COLUMNS = 16384;        // columns of one job (one wavefront), at most

// Every check of mimeo_path_stack, in the order the messages are promised: those of mimeo_path_insertions.
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                     uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, std::string *msg,
                     uint64_t max_window_items = pileup_host::MAX_WINDOW_ITEMS) {
    return insert_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, windows, nwin, items, nitems, sites, nsites, msg, max_window_items, NAME);
}

// A window as the kernel sees it: [start, end) and its sites [site0, site1) of the call.
struct WinDesc { uint32_t start, end, site0, site1; };
// A site as the kernel sees it: target base x, its insertion columns, and the column `col` of its window that holds its
// insertion column 0: (x - start) + the ncols of the window's sites in front of it.  The column of x itself is col + ncols.
struct SiteDesc { uint32_t x, ncols; uint64_t col; };

// The column layout of the call.  width[g]: W_g = (end - start) + the ncols of the window's sites, in 64 bits.
struct Layout {
    std::vector<WinDesc> win;
    std::vector<SiteDesc> site;
    std::vector<uint64_t> width;
};
inline Layout plan_layout(const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_insert_site *sites, uint64_t nsites) {
    Layout L;
    L.win.resize(nwin);
    L.site.resize(nsites);
    L.width.resize(nwin);
    uint64_t s = 0;
    for (uint64_t g = 0; g < nwin; g++) {   // the sites are sorted by (window, x)
        uint64_t ins = 0;
        const uint64_t s0 = s;
        for (; s < nsites && sites[s].window == g; s++) {
            L.site[s] = SiteDesc{sites[s].x, sites[s].ncols, (uint64_t)(sites[s].x - windows[g].start) + ins};
            ins += sites[s].ncols;
        }
        L.win[g] = WinDesc{windows[g].start, windows[g].end, (uint32_t)s0, (uint32_t)s};
        L.width[g] = (uint64_t)(windows[g].end - windows[g].start) + ins;
    }
    return L;
}

// row_first[k]: the prefix sum of the width of item k's window, nitems + 1 entries
inline void row_first_of(const Layout &L, const mimeo_window_item *items, uint64_t nitems, uint64_t *row_first) {
    row_first[0] = 0;
    for (uint64_t k = 0; k < nitems; k++) row_first[k + 1] = row_first[k] + L.width[items[k].group];
}

// The first block of [lo, hi) that ends behind target base x; hi where none does (path_call.h has the device's twin).
inline uint64_t first_block_ending_behind(const mimeo_path_block *blocks, uint64_t lo, uint64_t hi, uint64_t x) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if ((uint64_t)blocks[mid].t + blocks[mid].len > x) hi = mid; else lo = mid + 1;
    }
    return lo;
}

// The query stretch [q_lo, q_hi) of an item on the aligned strand: the bases under its target columns in [w0, w1) and its
// insertion runs with w0 <= p_k < w1.  false (and both zero) for an item without a query base: no block, a window that misses
// the alignment, or one that lies inside a deletion behind the deletion's first base.
inline bool query_stretch(const uint64_t *first, const mimeo_path_block *blocks, const mimeo_window_item &it, uint32_t *q_lo, uint32_t *q_hi) {
    *q_lo = *q_hi = 0;
    const uint64_t b0 = first[it.aln], b1 = first[(uint64_t)it.aln + 1];
    if (b0 == b1) return false;
    const uint64_t lo = blocks[b0].t, hi = (uint64_t)blocks[b1 - 1].t + blocks[b1 - 1].len;
    const uint64_t w0 = std::max<uint64_t>(it.w0, lo), w1 = std::min<uint64_t>(it.w1, hi);
    if (w0 >= w1) return false;
    // the first base: the block that ends behind w0 holds it, or starts behind it; a run that starts at p_k == w0 goes in front
    const uint64_t kf = first_block_ending_behind(blocks, b0, b1, w0);   // < b1: w0 < hi
    const mimeo_path_block &bf = blocks[kf];
    uint64_t ql, qh;
    if (kf > b0 && (uint64_t)blocks[kf - 1].t + blocks[kf - 1].len == w0) ql = (uint64_t)blocks[kf - 1].q + blocks[kf - 1].len;
    else ql = bf.t <= w0 ? bf.q + (w0 - bf.t) : bf.q;
    // behind the last base: inside the block that holds w1 - 1; in a gap the run in front of it where the gap starts inside
    // the window (p_k >= w0), otherwise nothing of that block's jump
    const uint64_t kl = first_block_ending_behind(blocks, b0, b1, w1 - 1);   // < b1: w1 <= hi
    const mimeo_path_block &bl = blocks[kl];
    if (bl.t <= w1 - 1) qh = bl.q + (w1 - bl.t);
    else qh = (uint64_t)blocks[kl - 1].t + blocks[kl - 1].len >= w0 ? bl.q : (uint64_t)blocks[kl - 1].q + blocks[kl - 1].len;   // kl > b0: w1 - 1 >= lo
    if (ql >= qh) return false;
    *q_lo = (uint32_t)ql;
    *q_hi = (uint32_t)qh;
    return true;
}

// A row of a batch as the kernel sees it: the path of alignment `aln` (index inside the slice) over [w0, w1) of window
// `window`, written from byte `off` of the batch's row buffer.
struct RowDesc { uint64_t off; uint32_t aln, window, w0, w1; };
// One job = one wavefront of the kernel: the columns [c0, c1) of row `row` of the batch, c0 < c1.
struct Job { uint64_t c0, c1; uint32_t row, pad; };

// A batch: the items order[i0 .. i1) of a slice, their rows packed one behind the other in `bytes` bytes of the row buffer.
struct Batch {
    uint64_t i0 = 0, i1 = 0, bytes = 0;
    std::vector<RowDesc> rows;
    std::vector<Job> jobs;
};
// The batch that starts at item order[i0] of the slice that begins at alignment a0 and ends in front of order[i_end]: rows are
// added while the bytes stay at most max_bytes; the first row goes in whatever its size.  A row of more than job_columns
// columns is cut into jobs of job_columns (0: the default); a row without a column makes none.
inline void plan_batch(const Layout &L, const mimeo_window_item *items, const uint64_t *order, uint64_t a0, uint64_t i0, uint64_t i_end, uint64_t max_bytes,
                       uint64_t job_columns, Batch &b) {
    if (!job_columns) job_columns = DEFAULT_JOB_COLUMNS;
    b.i0 = b.i1 = i0;
    b.bytes = 0;
    b.rows.clear();
    b.jobs.clear();
    for (; b.i1 < i_end; b.i1++) {
        const mimeo_window_item &it = items[order[b.i1]];
        const uint64_t w = L.width[it.group];
        if (b.i1 > i0 && b.bytes + w > max_bytes) break;
        const uint32_t row = (uint32_t)b.rows.size();
        b.rows.push_back(RowDesc{b.bytes, (uint32_t)(it.aln - a0), it.group, it.w0, it.w1});
        for (uint64_t c = 0; c < w; c += job_columns) b.jobs.push_back(Job{c, std::min(c + job_columns, w), row, 0u});
        b.bytes += w;
        if (b.rows.size() == 0xFFFFFFFFull) { b.i1++; break; }   // a job numbers its row in 32 bits
    }
}

}  // namespace stack_host
}  // namespace mimeo
