// path_text_host.h — HIP-free host side of mimeo_path_text (K11, k11_path_text.hip): the column count of every alignment and
// row_first, the column at which every block's region of its row starts (what the kernel searches), the cut of a call into
// slices of bounded output and of a long alignment into the kernel's jobs.  The paths are checked by
// path_stats_host::validate under this entry point's name.  Kept apart from the device code so that it runs under the CPU
// sanitizers (tests/sanitize/path_text_check.cc, tests/test_host_path_text.py).
//
// A row, for the blocks b_0 .. b_{m-1} of an alignment: for every k > 0 the dq_k insertion columns and then the dt_k deletion
// columns of the jump from b_{k-1} to b_k, then the len_k columns of b_k.  All counts in 64 bits: a path between two
// scaffolds of 2^31 bases spans up to 2^32 columns, and a call's rows add up beyond that.
#pragma once
#include "path_stats_host.h"

namespace mimeo {
namespace path_text_host {

constexpr uint64_t DEFAULT_SLICE_COLUMNS = 1ull << 28;   // two row buffers of 256 MiB (DESIGN.md "Alignment text")
constexpr uint64_t DEFAULT_SPLIT_COLUMNS = 16384;        // 16 passes of a wavefront's 64 x 16 columns
constexpr uint64_t SLICE_RECORDS = 1ull << 22;           // as K9: 48 + 8 + 8 bytes per record
constexpr uint64_t SLICE_BLOCKS = 1ull << 24;            // 12 + 8 bytes per block: 320 MiB

inline bool validate(const std::vector<uint64_t> &len_t, const std::vector<uint64_t> &len_q, const mimeo_alignment *aln, uint64_t n,
                     const uint64_t *first, const mimeo_path_block *blocks, uint64_t nblocks, std::string *msg) {
    return path_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, msg, "mimeo_path_text");
}

// columns of alignment i: (t_end - t_first) + (q_end - q_first) - sum of len; 0 without blocks.  The paths have passed validate().
inline uint64_t columns_of(const uint64_t *first, const mimeo_path_block *blocks, uint64_t i) {
    const uint64_t k0 = first[i], k1 = first[i + 1];
    if (k0 == k1) return 0;
    uint64_t sum = 0;
    for (uint64_t k = k0; k < k1; k++) sum += blocks[k].len;
    const mimeo_path_block &a = blocks[k0], &z = blocks[k1 - 1];
    return ((uint64_t)z.t + z.len - a.t) + ((uint64_t)z.q + z.len - a.q) - sum;
}

// row_first[0 .. n]: row i is bytes [row_first[i], row_first[i + 1]) of both outputs
inline void row_first_of(const uint64_t *first, const mimeo_path_block *blocks, uint64_t n, uint64_t *row_first) {
    row_first[0] = 0;
    for (uint64_t i = 0; i < n; i++) row_first[i + 1] = row_first[i] + columns_of(first, blocks, i);
}

// bcol[k - first[a0]] for the blocks k of the alignments [a0, a1): the column of its alignment's row at which block k's region
// — its insertion columns, its deletion columns, its diagonal — starts.  Strictly increasing inside an alignment (len >= 1),
// 0 at an alignment's first block.
inline void block_columns(const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0, uint64_t a1, std::vector<uint64_t> &bcol) {
    bcol.assign(first[a1] - first[a0], 0);
    for (uint64_t i = a0; i < a1; i++) {
        uint64_t c = 0;
        for (uint64_t k = first[i]; k < first[i + 1]; k++) {
            bcol[k - first[a0]] = c;
            if (k > first[i]) c += ((uint64_t)blocks[k].t - ((uint64_t)blocks[k - 1].t + blocks[k - 1].len)) + ((uint64_t)blocks[k].q - ((uint64_t)blocks[k - 1].q + blocks[k - 1].len));
            c += blocks[k].len;
        }
    }
}

// The call as slices [a0, a1) of whole alignments: at most max_records records, max_blocks blocks and max_columns output columns
// each, so that the uploads and the two row buffers of a slice are bounded whatever the job's size.  An alignment beyond a
// cap is a slice of its own.
inline std::vector<std::pair<uint64_t, uint64_t>> plan_slices(const uint64_t *row_first, const uint64_t *first, uint64_t n, uint64_t max_records,
                                                              uint64_t max_blocks, uint64_t max_columns) {
    return path_stats_host::plan_slices(first, n, max_records, max_blocks, row_first, max_columns);
}

// One job = one wavefront of the kernel: the columns [c0, c1) of the row of alignment `aln` (index inside the slice).  An
// alignment without columns has no job.  A row of more than split_columns columns is cut into jobs of split_columns (rounded
// down to a multiple of 16, at least 16); split_columns == 0: never.  The cuts lie at multiples of 16 OUTPUT columns — of
// row_first[i] + c, the byte of the output arrays — because that is what a lane's 16-byte store is aligned to: no 16-byte group
// is shared by two jobs of an alignment, and only a row's own head and tail are written narrower.
struct Job { uint64_t c0, c1; uint32_t aln, pad; };
inline void plan_jobs(const uint64_t *row_first, uint64_t a0, uint64_t a1, uint64_t split_columns, std::vector<Job> &jobs) {
    jobs.clear();
    const uint64_t step = split_columns < 16 ? 16 : split_columns & ~15ull;
    for (uint64_t i = a0; i < a1; i++) {
        const uint64_t base = row_first[i], cols = row_first[i + 1] - base;
        if (!cols) continue;
        if (!split_columns || cols <= split_columns) { jobs.push_back(Job{0, cols, (uint32_t)(i - a0), 0u}); continue; }
        uint64_t c0 = 0;
        while (c0 < cols) {
            uint64_t c1 = ((base + c0 + step) & ~15ull) - base;   // > c0: step >= 16
            if (c1 > cols) c1 = cols;
            jobs.push_back(Job{c0, c1, (uint32_t)(i - a0), 0u});
            c0 = c1;
        }
    }
}

}  // namespace path_text_host
}  // namespace mimeo
