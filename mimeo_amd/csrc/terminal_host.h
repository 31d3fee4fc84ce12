// terminal_host.h — HIP-free host side of mimeo_terminal_repeats (K17, k17_terminal.hip): the checks with their messages, the
// window and the three origins of an item, the layout of a job's traceback scratch (which the kernels share) and the cut of the
// jobs into launches whose scratch fits a budget.  Kept apart from the device code so that it runs under the CPU sanitizers
// (tests/sanitize/terminal_check.cc, tests/test_host_terminal.py).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mimeo_hip.h"

#if defined(__HIPCC__)
#define MIMEO_TERMINAL_HD __host__ __device__
#else
#define MIMEO_TERMINAL_HD
#endif

namespace mimeo {
namespace terminal_host {

constexpr const char *NAME = "mimeo_terminal_repeats";
constexpr int32_t MAX_WINDOW = 4096, MAX_WEIGHT = 1000;
// jobs of one launch, at most: a job's slot and its block count are 32 bits (the scan adds them up in 64), and the job table,
// records and counters of a launch stay a few tens of MiB
constexpr uint64_t MAX_LAUNCH_JOBS = 1ull << 20;

inline void defaults(mimeo_terminal_params *p) {
    *p = mimeo_terminal_params{};
    p->window = 1024;
    p->match = 2;
    p->mismatch = 3;
    p->gap_open = 5;
    p->gap_extend = 2;
    p->min_score = 40;
}

// MIMEO_OK, or MIMEO_ERR_LIMIT for a window outside 1 .. MAX_WINDOW, or MIMEO_ERR_ARG for every other parameter out of range
inline int check_params(const mimeo_terminal_params *p, std::string *msg) {
    char buf[200];
    auto bad = [&](const char *name, int32_t v, const char *range, int code) {
        snprintf(buf, sizeof buf, "%s: %s = %d is outside %s", NAME, name, v, range);
        *msg = buf;
        return code;
    };
    if (p->window < 1 || p->window > MAX_WINDOW) return bad("window", p->window, "1 .. 4096", MIMEO_ERR_LIMIT);
    if (p->match < 1 || p->match > MAX_WEIGHT) return bad("match", p->match, "1 .. 1000", MIMEO_ERR_ARG);
    if (p->mismatch < 1 || p->mismatch > MAX_WEIGHT) return bad("mismatch", p->mismatch, "1 .. 1000", MIMEO_ERR_ARG);
    if (p->gap_open < 0 || p->gap_open > MAX_WEIGHT) return bad("gap_open", p->gap_open, "0 .. 1000", MIMEO_ERR_ARG);
    if (p->gap_extend < 1 || p->gap_extend > MAX_WEIGHT) return bad("gap_extend", p->gap_extend, "1 .. 1000", MIMEO_ERR_ARG);
    if (p->min_score < 1) return bad("min_score", p->min_score, ">= 1", MIMEO_ERR_ARG);
    if (p->reserved[0] || p->reserved[1]) {
        *msg = std::string(NAME) + ": reserved must be 0";
        return MIMEO_ERR_ARG;
    }
    return MIMEO_OK;
}

// every item inside its scaffold; the message names the first one that is not
inline bool validate_items(const std::vector<uint64_t> &len, const mimeo_interval *iv, uint64_t n, std::string *msg) {
    char buf[240];
    for (uint64_t k = 0; k < n; k++) {
        if (iv[k].chrom >= len.size()) {
            snprintf(buf, sizeof buf, "%s: item %llu: chrom %u is outside the genome (%zu scaffolds)", NAME, (unsigned long long)k, iv[k].chrom, len.size());
            *msg = buf;
            return false;
        }
        if (iv[k].start > iv[k].end || iv[k].end > len[iv[k].chrom]) {
            snprintf(buf, sizeof buf, "%s: item %llu: [%u, %u) is not an interval of scaffold %u (%llu bases)", NAME, (unsigned long long)k, iv[k].start,
                     iv[k].end, iv[k].chrom, (unsigned long long)len[iv[k].chrom]);
            *msg = buf;
            return false;
        }
    }
    return true;
}

// The window of an item and where its three stretches begin: the head and the direct tail on the forward strand, the inverted
// tail on the stored reverse complement.  All three lie inside the scaffold, and the head never overlaps the direct tail.
struct Windows { uint32_t w, head, direct, inverted; };
inline Windows windows(const mimeo_interval &iv, uint64_t len, int32_t window) {
    const uint32_t w = std::min<uint32_t>((uint32_t)window, (iv.end - iv.start) / 2u);
    return Windows{w, iv.start, iv.end - w, (uint32_t)(len - iv.end)};
}

// ---- the traceback scratch of one job ------------------------------------------------------------------------------------------
// The DP kernel sweeps a strip of 64 columns in w + 63 steps, lane l at row t - l in step t, and a lane packs the nibbles of
// eight consecutive STEPS into a word, so that all 64 lanes store together: word (strip, t >> 3, lane), nibble t & 7.
MIMEO_TERMINAL_HD inline uint32_t strips(uint32_t w) { return (w + 63u) >> 6; }
MIMEO_TERMINAL_HD inline uint32_t step_groups(uint32_t w) { return (w + 63u + 7u) >> 3; }
MIMEO_TERMINAL_HD inline uint64_t trace_words(uint32_t w) { return w ? (uint64_t)strips(w) * step_groups(w) * 64u : 0u; }
// the word and the nibble of cell (i, j) inside a job's scratch
MIMEO_TERMINAL_HD inline uint64_t trace_word(uint32_t w, uint32_t i, uint32_t j) {
    const uint32_t l = j & 63u, t = i + l;
    return ((uint64_t)(j >> 6) * step_groups(w) + (t >> 3)) * 64u + l;
}
MIMEO_TERMINAL_HD inline uint32_t trace_shift(uint32_t i, uint32_t j) { return ((i + (j & 63u)) & 7u) * 4u; }

// One job = one wavefront of the DP kernel: orientation `strand` (0 direct, 1 inverted) of item slot / 2 of the launch.
// trace_off: its first word of the launch's scratch; blk_off: its first block of the launch's block region, w blocks long (a
// path has at most one block per row).
struct Job { uint32_t chrom, w, a0, b0, strand, slot; uint64_t trace_off, blk_off; };
inline uint64_t job_bytes(uint32_t w) { return trace_words(w) * 4u + (uint64_t)w * sizeof(mimeo_path_block); }

// The cut into launches: consecutive items, as many as fit `budget` bytes of scratch (a single item always goes, whatever its
// size) and MAX_LAUNCH_JOBS jobs.  [first, second) are items; a launch runs both orientations of each.
inline std::vector<std::pair<uint64_t, uint64_t>> plan_launches(const std::vector<uint32_t> &w_of_item, uint64_t budget, uint64_t max_jobs = MAX_LAUNCH_JOBS) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    uint64_t k0 = 0, bytes = 0;
    for (uint64_t k = 0; k < w_of_item.size(); k++) {
        const uint64_t b = 2u * job_bytes(w_of_item[k]);
        if (k > k0 && (bytes + b > budget || 2u * (k - k0) + 2u > max_jobs)) {
            out.emplace_back(k0, k);
            k0 = k;
            bytes = 0;
        }
        bytes += b;
    }
    if (k0 < w_of_item.size()) out.emplace_back(k0, (uint64_t)w_of_item.size());
    return out;
}

// The jobs of the items [k0, k1), the longest windows first (equal windows in the order of their slots): the wavefronts that
// run longest start first.  *trace_total and *blk_total: the words and the blocks of scratch that the launch needs.
inline void plan_jobs(const mimeo_interval *iv, const std::vector<uint64_t> &len, int32_t window, uint64_t k0, uint64_t k1, std::vector<Job> &jobs,
                      uint64_t *trace_total, uint64_t *blk_total) {
    jobs.clear();
    for (uint64_t k = k0; k < k1; k++) {
        const Windows W = windows(iv[k], len[iv[k].chrom], window);
        jobs.push_back(Job{iv[k].chrom, W.w, W.head, W.direct, 0u, (uint32_t)(2u * (k - k0)), 0u, 0u});
        jobs.push_back(Job{iv[k].chrom, W.w, W.head, W.inverted, 1u, (uint32_t)(2u * (k - k0) + 1u), 0u, 0u});
    }
    std::stable_sort(jobs.begin(), jobs.end(), [](const Job &x, const Job &y) { return x.w > y.w; });
    uint64_t tw = 0, nb = 0;
    for (Job &j : jobs) {
        j.trace_off = tw;
        j.blk_off = nb;
        tw += trace_words(j.w);
        nb += j.w;
    }
    *trace_total = tw;
    *blk_total = nb;
}

}  // namespace terminal_host
}  // namespace mimeo
