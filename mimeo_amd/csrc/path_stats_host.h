// path_stats_host.h — HIP-free host side of mimeo_path_stats (K9, k9_path_stats.hip): the checks that keep a bad path
// away from the kernel, and the cut of a call into slices of bounded size.  Kept apart from the device code so that it
// runs under the CPU sanitizers (tests/sanitize/path_stats_check.cc, tests/test_host_divergence.py).
#pragma once
#include <cstdint>
#include <cstdio>
#include <string>
#include <utility>
#include <vector>

#include "../../include/mimeo_hip.h"

namespace mimeo {
namespace path_stats_host {

// Everything the kernel relies on, checked before anything is uploaded.  All arithmetic in 64 bits: t = 0xFFFFFFF0 with
// len = 0x20 is beyond every scaffold, not at base 0x10.  len_t / len_q: bases per scaffold of the target and of the query
// genome.  Returns true when the call is sound; otherwise *msg names the record (and the block) that is not.  `name`: the entry
// point the message starts with (mimeo_path_text makes the same checks under its own name).
inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n,
                     const uint64_t *first, const mimeo_path_block *blocks, uint64_t nblocks, std::string *msg,
                     const char *name = "mimeo_path_stats") {
    char buf[320];
    auto fail = [&](const char *what, uint64_t rec, bool has_block, uint64_t blk) {
        if (has_block) {
            const mimeo_path_block &b = blocks[blk];
            snprintf(buf, sizeof buf, "%s: record %llu, block %llu (t %u, q %u, len %u): %s", name, (unsigned long long)rec,
                     (unsigned long long)blk, b.t, b.q, b.len, what);
        } else {
            snprintf(buf, sizeof buf, "%s: record %llu: %s", name, (unsigned long long)rec, what);
        }
        *msg = buf;
        return false;
    };
    if (!n) return true;
    if (!aln || !first || (nblocks && !blocks)) { *msg = std::string(name) + ": null argument"; return false; }
    // the offsets first: no block is looked at before every range is known to lie inside blocks[0 .. nblocks)
    if (first[0] != 0) return fail("path_first[0] is not 0", 0, false, 0);
    for (uint64_t i = 0; i < n; i++)
        if (first[i + 1] < first[i]) return fail("path_first decreases behind this record", i, false, 0);
    if (first[n] != nblocks) return fail("path_first[n] is not nblocks", n - 1, false, 0);
    for (uint64_t i = 0; i < n; i++) {
        const mimeo_alignment &a = aln[i];
        if (a.tid >= len_t.size()) return fail("tid is not a scaffold of the target genome", i, false, 0);
        if (a.qid >= len_q.size()) return fail("qid is not a scaffold of the query genome", i, false, 0);
        if (a.qstrand > 1) return fail("qstrand is neither 0 nor 1", i, false, 0);
        const uint64_t Lt = len_t[a.tid], Lq = len_q[a.qid];
        uint64_t t_end = 0, q_end = 0;   // end of the block before
        for (uint64_t k = first[i]; k < first[i + 1]; k++) {
            const uint64_t t = blocks[k].t, q = blocks[k].q, len = blocks[k].len;
            if (len < 1) return fail("len is 0", i, true, k);
            if (t + len > Lt) return fail("t + len is beyond the target scaffold", i, true, k);
            if (q + len > Lq) return fail("q + len is beyond the query scaffold", i, true, k);
            if (k > first[i] && (t < t_end || q < q_end)) return fail("overlaps the block before it or lies in front of it", i, true, k);
            t_end = t + len;
            q_end = q + len;
        }
    }
    return true;
}

// 64-column chunks of one alignment: what the kernel's work is counted in
inline uint64_t chunks_of(const uint64_t *first, const mimeo_path_block *blocks, uint64_t i) {
    uint64_t c = 0;
    for (uint64_t k = first[i]; k < first[i + 1]; k++) c += ((uint64_t)blocks[k].len + 63) / 64;
    return c;
}

// The call as slices [a0, a1) of whole alignments: at most max_records records and max_blocks blocks each, so that the
// upload of a slice is bounded whatever the job's size.  An alignment with more blocks than max_blocks is a slice of its own
// (12 bytes per block: 2^24 blocks are 192 MiB, and no alignment comes near).  `first` has passed validate().
// row_first (optional; K11, path_text_host.h): alignment i also makes row_first[i + 1] - row_first[i] output columns, and a
// slice holds at most max_columns of them; an alignment of more is a slice of its own.
inline std::vector<std::pair<uint64_t, uint64_t>> plan_slices(const uint64_t *first, uint64_t n, uint64_t max_records, uint64_t max_blocks,
                                                              const uint64_t *row_first = nullptr, uint64_t max_columns = 0) {
    std::vector<std::pair<uint64_t, uint64_t>> s;
    if (max_records < 1) max_records = 1;
    if (max_blocks < 1) max_blocks = 1;
    if (max_columns < 1) max_columns = 1;
    uint64_t a0 = 0;
    while (a0 < n) {
        uint64_t a1 = a0 + 1;
        while (a1 < n && a1 - a0 < max_records && first[a1 + 1] - first[a0] <= max_blocks &&
               (!row_first || row_first[a1 + 1] - row_first[a0] <= max_columns))
            a1++;
        s.emplace_back(a0, a1);
        a0 = a1;
    }
    return s;
}

// One job = one wavefront of the kernel: the 64-column chunks [c0, c1) of alignment `aln` (index inside the slice), counted
// through the alignment's blocks in order.  An alignment of more than split_chunks chunks is cut into jobs of split_chunks
// (split = 1: its jobs add their counts to the alignment's with integer atomics; the job with c0 == 0 counts the gaps);
// split_chunks == 0: never.  A chromosome-long self diagonal would otherwise be one wavefront's work.
struct Job { uint32_t aln, split, c0, c1; };
inline void plan_jobs(const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0, uint64_t a1, uint64_t split_chunks, std::vector<Job> &jobs) {
    jobs.clear();
    for (uint64_t i = a0; i < a1; i++) {
        const uint64_t c = chunks_of(first, blocks, i);   // at most the alignment's columns, and its blocks lie side by side inside a scaffold of less than 2^32 bases
        if (!split_chunks || c <= split_chunks) { jobs.push_back(Job{(uint32_t)(i - a0), 0u, 0u, (uint32_t)c}); continue; }
        for (uint64_t c0 = 0; c0 < c; c0 += split_chunks)
            jobs.push_back(Job{(uint32_t)(i - a0), 1u, (uint32_t)c0, (uint32_t)(c0 + split_chunks < c ? c0 + split_chunks : c)});
    }
}

}  // namespace path_stats_host
}  // namespace mimeo
