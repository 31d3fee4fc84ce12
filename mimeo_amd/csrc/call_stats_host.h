// call_stats_host.h — HIP-free host side of mimeo_path_call_stats (K16, k16_call_stats.hip): the checks (those of
// mimeo_path_stack, under this entry point's name, and then the bytes of the two calls), the offsets of the windows' columns in
// `call` and of the sites' columns in `icall`, `iletters` — the prefix count of the letter columns of `icall` per site, so that
// the sites an item spans without a run cost the host one subtraction per job and the device nothing — and the cut of an item's
// [lo, hi) into the kernel's jobs of a bounded number of target columns.  Kept apart from the device code so that it runs
// under the CPU sanitizers (tests/sanitize/call_stats_check.cc, tests/test_host_call_stats.py).  The items go to the slices of
// path_stats_host::plan_slices with window_stats_host::bucket_items, as for K13, K14 and K15; the query stretch of an item is
// stack_host::query_stretch.
#pragma once
#include <algorithm>

#include "stack_host.h"

namespace mimeo {
namespace call_stats_host {

constexpr const char *NAME = "mimeo_path_call_stats";
constexpr uint64_t DEFAULT_JOB_COLUMNS = 1ull << 16;   // target columns of one job (one wavefront), at most
// A job numbers its columns of `call`, and the columns of its sites in `icall`, in 32 bits from its own first one: at most 2^20
// target columns, hence at most 2^20 sites of at most 1024 columns.
constexpr uint64_t MAX_JOB_COLUMNS = 1ull << 20;

// Every check of mimeo_path_call_stats on the paths, windows, items and sites, in the order the messages are promised: those
// of mimeo_path_stack.
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                     uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, std::string *msg,
                     uint64_t max_window_items = pileup_host::MAX_WINDOW_ITEMS) {
    return insert_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, windows, nwin, items, nitems, sites, nsites, msg, max_window_items, NAME);
}

inline bool call_byte(uint8_t b) { return b == 'A' || b == 'C' || b == 'G' || b == 'T' || b == 'N' || b == '-'; }
inline bool call_letter(uint8_t b) { return b != '-'; }   // of a checked byte: A C G T N

// The bytes of the two calls, after everything else has passed: every byte one of A C G T N -.  `call` holds one byte per
// column of the windows, one window behind the other; `icall` one per insertion column of the sites.
inline bool validate_calls(const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_insert_site *sites, uint64_t nsites, const uint8_t *call,
                           const uint8_t *icall, std::string *msg) {
    char buf[320];
    uint64_t at = 0;
    for (uint64_t g = 0; g < nwin; g++) {
        const uint64_t w = (uint64_t)windows[g].end - windows[g].start;
        if (w && !call) { *msg = std::string(NAME) + ": null argument"; return false; }
        for (uint64_t i = 0; i < w; i++)
            if (!call_byte(call[at + i])) {
                snprintf(buf, sizeof buf, "%s: column %llu of call (window %llu, x %llu): byte 0x%02x is not one of A C G T N -", NAME,
                         (unsigned long long)(at + i), (unsigned long long)g, (unsigned long long)(windows[g].start + i), call[at + i]);
                *msg = buf;
                return false;
            }
        at += w;
    }
    at = 0;
    for (uint64_t s = 0; s < nsites; s++) {
        if (!icall) { *msg = std::string(NAME) + ": null argument"; return false; }
        for (uint64_t j = 0; j < sites[s].ncols; j++)
            if (!call_byte(icall[at + j])) {
                snprintf(buf, sizeof buf, "%s: insertion column %llu of icall (site %llu, column %llu): byte 0x%02x is not one of A C G T N -", NAME,
                         (unsigned long long)(at + j), (unsigned long long)s, (unsigned long long)j, icall[at + j]);
                *msg = buf;
                return false;
            }
        at += sites[s].ncols;
    }
    return true;
}

// A site as the kernel sees it: target base x, its columns, and the entry of its column 0 in `icall`.
struct SiteDesc { uint32_t x, ncols; uint64_t icol; };

// The offsets of the call.  col_first[g]: the entry of window g's first column in `call` (nwin + 1 entries, in 64 bits);
// win_first[g] .. win_first[g + 1]: the sites of window g; site[s].icol: the entry of site s's column 0 in `icall`;
// iletters[s]: the letter columns (not '-') of `icall` in front of site s (nsites + 1 entries).
struct Plan {
    std::vector<uint64_t> col_first, win_first, iletters;
    std::vector<SiteDesc> site;
    uint64_t ncols() const { return col_first.back(); }
    uint64_t nicols() const { return site.empty() ? 0 : site.back().icol + site.back().ncols; }
};
inline Plan plan_call(const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_insert_site *sites, uint64_t nsites, const uint8_t *icall) {
    Plan p;
    p.col_first.assign(nwin + 1, 0);
    p.win_first.assign(nwin + 1, 0);
    p.iletters.assign(nsites + 1, 0);
    p.site.resize(nsites);
    for (uint64_t g = 0; g < nwin; g++) p.col_first[g + 1] = p.col_first[g] + ((uint64_t)windows[g].end - windows[g].start);
    uint64_t at = 0;
    for (uint64_t s = 0; s < nsites; s++) {
        p.site[s] = SiteDesc{sites[s].x, sites[s].ncols, at};
        p.win_first[(uint64_t)sites[s].window + 1]++;
        uint64_t letters = 0;
        for (uint32_t j = 0; j < sites[s].ncols; j++) letters += call_letter(icall[at + j]);
        p.iletters[s + 1] = p.iletters[s] + letters;
        at += sites[s].ncols;
    }
    for (uint64_t g = 0; g < nwin; g++) p.win_first[g + 1] += p.win_first[g];
    return p;
}

// One job = one wavefront of the kernel: the path of alignment `aln` (index inside the slice) over the target bases [w0, w1),
// added to out[item].  [w0, w1) is never empty and lies inside the item's window clipped to the alignment's own [first block's
// t, last block's end): the kernel's block search relies on it.  col: the entry of base w0's column in `call`.  [site0, site1):
// the sites of the item's window with x in [w0, w1) that the alignment spans — x == the first block's t is left out; icol0: the
// entry of site0's column 0 in `icall` (0 without a site); site_letters: the letter columns of `icall` at those sites, which
// the kernel adds to del_bases before it takes off what the item's runs hold there.
struct Job { uint32_t aln, item, w0, w1, site0, site1, site_letters, pad; uint64_t col, icol0; };

// The jobs of the items order[i0 .. i1), all of alignments of the slice that begins at alignment a0.  An item is clipped to its
// alignment first; one left empty makes no job.  What is left is cut into consecutive pieces of job_columns target bases (0 or
// more than MAX_JOB_COLUMNS: the default): every rule of the header is additive over a partition of [lo, hi) — a run and a site
// belong to the piece that holds their target base.
inline void plan_jobs(const Plan &p, const mimeo_pileup_window *windows, const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0,
                      const mimeo_window_item *items, const uint64_t *order, uint64_t i0, uint64_t i1, uint64_t job_columns, std::vector<Job> &jobs) {
    jobs.clear();
    if (!job_columns || job_columns > MAX_JOB_COLUMNS) job_columns = DEFAULT_JOB_COLUMNS;
    auto below = [](const SiteDesc &s, uint64_t x) { return s.x < x; };
    for (uint64_t i = i0; i < i1; i++) {
        const mimeo_window_item &it = items[order[i]];
        const uint64_t b0 = first[it.aln], b1 = first[(uint64_t)it.aln + 1];
        if (b0 == b1) continue;   // an alignment without blocks counts nothing
        const uint64_t lo = blocks[b0].t, hi = (uint64_t)blocks[b1 - 1].t + blocks[b1 - 1].len;   // hi <= the scaffold's length < 2^32
        const uint64_t w0 = std::max<uint64_t>(it.w0, lo), w1 = std::min<uint64_t>(it.w1, hi);
        if (w0 >= w1) continue;
        const SiteDesc *f = p.site.data() + p.win_first[it.group], *l = p.site.data() + p.win_first[(uint64_t)it.group + 1];
        const uint64_t col0 = p.col_first[it.group] - windows[it.group].start;   // + x: the column of target base x (mod 2^64)
        for (uint64_t a = w0; a < w1; a += job_columns) {
            const uint64_t b = std::min(a + job_columns, w1);
            const uint64_t s0 = (uint64_t)(std::lower_bound(f, l, std::max(a, lo + 1), below) - p.site.data());
            const uint64_t s1 = std::max(s0, (uint64_t)(std::lower_bound(f, l, b, below) - p.site.data()));
            jobs.push_back(Job{(uint32_t)(it.aln - a0), (uint32_t)order[i], (uint32_t)a, (uint32_t)b, (uint32_t)s0, (uint32_t)s1,
                               (uint32_t)(p.iletters[s1] - p.iletters[s0]), 0u, col0 + a, s0 < s1 ? p.site[s0].icol : 0});
        }
    }
}

}  // namespace call_stats_host
}  // namespace mimeo
