// window_stats_host.h — HIP-free host side of mimeo_path_window_stats (K10, k10_window_stats.hip): the checks on the items,
// their distribution over the slices of path_stats_host::plan_slices, and the cut of an item into the kernel's jobs.  Kept
// apart from the device code so that it runs under the CPU sanitizers (tests/sanitize/window_stats_check.cc,
// tests/test_host_window_stats.py).  The paths themselves are checked by path_stats_host::validate.
#pragma once
#include <algorithm>

#include "path_stats_host.h"

namespace mimeo {
namespace window_stats_host {

// The items against the records, the groups and the target scaffolds; the paths have passed path_stats_host::validate.
// Returns true when every item is sound; otherwise *msg names the item that is not.
inline bool validate_items(const std::vector<uint64_t> &len_t, const mimeo_alignment *aln, uint64_t n, const mimeo_window_item *items,
                           uint64_t nitems, uint64_t ngroups, std::string *msg) {
    char buf[320];
    auto fail = [&](uint64_t i, const char *what) {
        const mimeo_window_item &it = items[i];
        snprintf(buf, sizeof buf, "mimeo_path_window_stats: item %llu (aln %u, group %u, window [%u, %u)): %s", (unsigned long long)i, it.aln,
                 it.group, it.w0, it.w1, what);
        *msg = buf;
        return false;
    };
    if (!nitems) return true;
    if (!items || (n && !aln)) { *msg = "mimeo_path_window_stats: null argument"; return false; }
    for (uint64_t i = 0; i < nitems; i++) {
        const mimeo_window_item &it = items[i];
        if (it.aln >= n) return fail(i, "aln is not a record of the call");
        if (it.group >= ngroups) return fail(i, "group is not below ngroups");
        if (it.w0 > it.w1) return fail(i, "w0 is beyond w1");
        if (it.w1 > len_t[aln[it.aln].tid]) return fail(i, "w1 is beyond the target scaffold");
    }
    return true;
}

// Every check of mimeo_path_window_stats, in the order the messages are promised: the paths (path_stats_host::validate), then
// the items.
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n,
                     const uint64_t *first, const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_window_item *items, uint64_t nitems,
                     uint64_t ngroups, std::string *msg) {
    return path_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, msg) && validate_items(len_t, aln, n, items, nitems, ngroups, msg);
}

// The items of every slice: order[start[s] .. start[s + 1]) are the numbers of the items whose alignment lies in slice s, in
// the order of the call (a counting sort; `slices` are consecutive ranges of alignments that begin at 0).
inline void bucket_items(const std::vector<std::pair<uint64_t, uint64_t>> &slices, const mimeo_window_item *items, uint64_t nitems,
                         std::vector<uint64_t> &order, std::vector<uint64_t> &start) {
    std::vector<uint64_t> ends(slices.size());
    for (size_t s = 0; s < slices.size(); s++) ends[s] = slices[s].second;
    auto slice_of = [&](uint32_t a) { return (size_t)(std::upper_bound(ends.begin(), ends.end(), (uint64_t)a) - ends.begin()); };
    start.assign(slices.size() + 1, 0);
    for (uint64_t i = 0; i < nitems; i++) start[slice_of(items[i].aln) + 1]++;
    for (size_t s = 0; s < slices.size(); s++) start[s + 1] += start[s];
    order.resize(nitems);
    std::vector<uint64_t> at(start.begin(), start.end() - 1);
    for (uint64_t i = 0; i < nitems; i++) order[at[slice_of(items[i].aln)]++] = i;
}

// One job = one wavefront of the kernel: the path of alignment `aln` (index inside the slice) clipped to the target window
// [w0, w1), added to group `group`.  The window of a job is never empty and lies inside the alignment's own
// [first block's t, last block's end): the kernel's block search relies on it.
struct Job { uint32_t aln, group, w0, w1; };

// The jobs of the items order[i0 .. i1), all of alignments of the slice that begins at alignment a0.  A window is clipped to
// its alignment first (what lies outside counts nothing: every gap of a path starts and ends inside it); an item left empty
// makes no job.  A clipped window of more than split_bases target bases is cut into consecutive pieces of split_bases
// (0: never): the statistics are additive over any partition of a window, so the pieces need no special first job.
inline void plan_jobs(const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0, const mimeo_window_item *items, const uint64_t *order,
                      uint64_t i0, uint64_t i1, uint64_t split_bases, std::vector<Job> &jobs) {
    jobs.clear();
    for (uint64_t i = i0; i < i1; i++) {
        const mimeo_window_item &it = items[order[i]];
        const uint64_t b0 = first[it.aln], b1 = first[(uint64_t)it.aln + 1];
        if (b0 == b1) continue;   // an alignment without blocks counts nothing
        const uint64_t lo = blocks[b0].t, hi = (uint64_t)blocks[b1 - 1].t + blocks[b1 - 1].len;   // hi <= the scaffold's length < 2^32
        const uint64_t w0 = std::max<uint64_t>(it.w0, lo), w1 = std::min<uint64_t>(it.w1, hi);
        if (w0 >= w1) continue;
        const uint32_t a = (uint32_t)(it.aln - a0);
        if (!split_bases || w1 - w0 <= split_bases) { jobs.push_back(Job{a, it.group, (uint32_t)w0, (uint32_t)w1}); continue; }
        for (uint64_t p = w0; p < w1; p += split_bases) jobs.push_back(Job{a, it.group, (uint32_t)p, (uint32_t)std::min(p + split_bases, w1)});
    }
}

}  // namespace window_stats_host
}  // namespace mimeo
