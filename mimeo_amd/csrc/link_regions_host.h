// link_regions_host.h — HIP-free host side of mimeo_link_regions (K12, k12_link_regions.hip): the checks on the regions, the
// scaffold-to-chromosome table and the items, the per-chromosome offsets into the region table, and the cut of the items into
// the kernel's jobs (rule A of "family linking v1" is decided here: an item that fails it makes no job).  Kept apart from the
// device code so that it runs under the CPU sanitizers (tests/sanitize/link_regions_check.cc, tests/test_host_families.py).
// The paths are checked by path_stats_host::validate, the items go to the slices of path_stats_host::plan_slices with
// window_stats_host::bucket_items.
#pragma once
#include <algorithm>

#include "window_stats_host.h"

namespace mimeo {
namespace link_regions_host {

constexpr const char *NAME = "mimeo_link_regions";

// chrom_of_scaf (null: identity) must number the scaffolds 0 .. nscaf - 1, each once: the device indexes the per-chromosome
// offsets and the scaffold lengths with it.  chrom[i] receives the chromosome of scaffold i.
inline bool validate_chroms(uint64_t nscaf, const uint32_t *chrom_of_scaf, std::vector<uint32_t> &chrom, std::string *msg) {
    char buf[320];
    chrom.resize(nscaf);
    std::vector<uint32_t> scaf_of(nscaf, 0xFFFFFFFFu);
    for (uint64_t i = 0; i < nscaf; i++) {
        const uint32_t c = chrom_of_scaf ? chrom_of_scaf[i] : (uint32_t)i;
        if (c >= nscaf) {
            snprintf(buf, sizeof buf, "%s: chrom_of_scaf[%llu] = %u is not below the number of scaffolds", NAME, (unsigned long long)i, c);
            *msg = buf;
            return false;
        }
        if (scaf_of[c] != 0xFFFFFFFFu) {
            snprintf(buf, sizeof buf, "%s: chrom_of_scaf[%llu] = %u is also the chromosome of scaffold %u", NAME, (unsigned long long)i, c, scaf_of[c]);
            *msg = buf;
            return false;
        }
        scaf_of[c] = (uint32_t)i;
        chrom[i] = c;
    }
    return true;
}

// The region table: sorted by (chrom, start), disjoint, no region empty, every region inside its scaffold.  len_t[i]: bases of
// scaffold i; chrom: what validate_chroms made.
inline bool validate_regions(const std::vector<uint64_t> &len_t, const std::vector<uint32_t> &chrom, const mimeo_interval *regions, uint64_t nreg,
                             std::string *msg) {
    char buf[320];
    auto fail = [&](uint64_t r, const char *what) {
        snprintf(buf, sizeof buf, "%s: region %llu (chrom %u, [%u, %u)): %s", NAME, (unsigned long long)r, regions[r].chrom, regions[r].start,
                 regions[r].end, what);
        *msg = buf;
        return false;
    };
    if (!nreg) return true;
    if (!regions) { *msg = std::string(NAME) + ": null argument"; return false; }
    if (nreg > 0xFFFFFFFFull) { *msg = std::string(NAME) + ": more than 2^32 - 1 regions"; return false; }
    std::vector<uint64_t> len_c(chrom.size());
    for (size_t i = 0; i < chrom.size(); i++) len_c[chrom[i]] = len_t[i];
    for (uint64_t r = 0; r < nreg; r++) {
        const mimeo_interval &v = regions[r];
        if (v.chrom >= len_c.size()) return fail(r, "chrom is not a chromosome of the genome");
        if (v.start >= v.end) return fail(r, "start is not below end");
        if (v.end > len_c[v.chrom]) return fail(r, "end is beyond its scaffold");
        if (r && (v.chrom < regions[r - 1].chrom || (v.chrom == regions[r - 1].chrom && v.start < regions[r - 1].end)))
            return fail(r, "lies in front of the region before it or overlaps it");
    }
    return true;
}

// The items against the records and the regions; the paths, the table and the regions have passed their checks.
inline bool validate_items(const std::vector<uint32_t> &chrom, const mimeo_alignment *aln, uint64_t n, const mimeo_interval *regions, uint64_t nreg,
                           const mimeo_window_item *items, uint64_t nitems, std::string *msg) {
    char buf[320];
    auto fail = [&](uint64_t i, const char *what) {
        const mimeo_window_item &it = items[i];
        snprintf(buf, sizeof buf, "%s: item %llu (aln %u, region %u, window [%u, %u)): %s", NAME, (unsigned long long)i, it.aln, it.group, it.w0, it.w1,
                 what);
        *msg = buf;
        return false;
    };
    if (!nitems) return true;
    if (!items || (n && !aln)) { *msg = std::string(NAME) + ": null argument"; return false; }
    for (uint64_t i = 0; i < nitems; i++) {
        const mimeo_window_item &it = items[i];
        if (it.aln >= n) return fail(i, "aln is not a record of the call");
        if (it.group >= nreg) return fail(i, "region is not below nreg");
        const mimeo_interval &r = regions[it.group];
        if (r.chrom != chrom[aln[it.aln].tid]) return fail(i, "the region does not lie on the record's target scaffold");
        if (it.w0 > it.w1) return fail(i, "w0 is beyond w1");
        if (it.w0 < r.start || it.w1 > r.end) return fail(i, "the window does not lie inside the region");
    }
    return true;
}

// Every check of mimeo_link_regions, in the order the messages are promised: min_cover_pct, the paths (a self job: the query
// scaffolds are the target's), chrom_of_scaf, the regions, the items.  chrom receives the table (validate_chroms).
inline bool validate(const std::vector<uint64_t> &len_t, const mimeo_alignment *aln, uint64_t n, const uint64_t *first, const mimeo_path_block *blocks,
                     uint64_t nblocks, const mimeo_interval *regions, uint64_t nreg, const uint32_t *chrom_of_scaf, const mimeo_window_item *items,
                     uint64_t nitems, uint32_t min_cover_pct, std::vector<uint32_t> &chrom, std::string *msg) {
    if (min_cover_pct < 1 || min_cover_pct > 100) {
        char buf[160];
        snprintf(buf, sizeof buf, "%s: min_cover_pct %u is not in 1 .. 100", NAME, min_cover_pct);
        *msg = buf;
        return false;
    }
    return path_stats_host::validate(len_t, len_t, aln, n, first, blocks, nblocks, msg, NAME) && validate_chroms(len_t.size(), chrom_of_scaf, chrom, msg) &&
           validate_regions(len_t, chrom, regions, nreg, msg) && validate_items(chrom, aln, n, regions, nreg, items, nitems, msg);
}

// chrom_first[c] .. chrom_first[c + 1]: the regions of chromosome c in the sorted table (nchrom + 1 entries)
inline std::vector<uint32_t> chrom_offsets(const mimeo_interval *regions, uint64_t nreg, uint64_t nchrom) {
    std::vector<uint32_t> off(nchrom + 1, 0);
    for (uint64_t r = 0; r < nreg; r++) off[regions[r].chrom + 1]++;
    for (uint64_t c = 0; c < nchrom; c++) off[c + 1] += off[c];
    return off;
}

// rule A: the window [w0, w1) covers at least pct per cent of the region [rs, re); 64 bits
inline bool covers(uint64_t w0, uint64_t w1, uint64_t rs, uint64_t re, uint64_t pct) { return 100 * (w1 - w0) >= pct * (re - rs); }

// One job = one lane of the kernel: the path of alignment `aln` (index inside the slice), which has at least one block,
// projected from the target window [w0, w1) of region `region`.
struct Job { uint32_t aln, region, w0, w1; };

// The jobs of the items order[i0 .. i1), all of alignments of the slice that begins at alignment a0, in that order.  An item
// whose window fails rule A, or whose alignment has no block, links nothing and makes no job.
inline void plan_jobs(const uint64_t *first, uint64_t a0, const mimeo_interval *regions, const mimeo_window_item *items, const uint64_t *order, uint64_t i0,
                      uint64_t i1, uint32_t pct, std::vector<Job> &jobs) {
    jobs.clear();
    for (uint64_t i = i0; i < i1; i++) {
        const mimeo_window_item &it = items[order[i]];
        if (first[it.aln] == first[(uint64_t)it.aln + 1]) continue;
        const mimeo_interval &r = regions[it.group];
        if (!covers(it.w0, it.w1, r.start, r.end, pct)) continue;
        jobs.push_back(Job{(uint32_t)(it.aln - a0), it.group, it.w0, it.w1});
    }
}

}  // namespace link_regions_host
}  // namespace mimeo
