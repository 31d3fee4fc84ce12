// flank_host.h — HIP-free host side of mimeo_flank_repeats (K18, k18_flank.hip): the checks with their messages, the two
// regions of an item, the packed key that orders the candidates as the header does (which the kernel shares) and the choice of
// dr among the candidates of one row.  Kept apart from the device code so that it runs under the CPU sanitizers
// (tests/sanitize/elements_check.cc, tests/test_host_elements.py).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <vector>

#include "../../include/mimeo_hip.h"

#if defined(__HIPCC__)
#define MIMEO_FLANK_HD __host__ __device__
#else
#define MIMEO_FLANK_HD
#endif

namespace mimeo {
namespace flank_host {

constexpr const char *NAME = "mimeo_flank_repeats";
constexpr int32_t MAX_LEN = 32, MAX_SLACK = 8, MAX_MISMATCH = 2, MISMATCH_CHARGE = 3;
constexpr uint32_t REGION_MAX = MAX_LEN + 2 * MAX_SLACK;   // 48 bases on either side: the lanes of a wavefront hold a region

inline void defaults(mimeo_flank_params *p) {
    *p = mimeo_flank_params{};
    p->min_len = 4;
    p->max_len = 20;
    p->slack = 2;
    p->max_mismatch = 0;
}

inline int check_params(const mimeo_flank_params *p, std::string *msg) {
    char buf[200];
    auto bad = [&](const char *name, int32_t v, const char *range) {
        snprintf(buf, sizeof buf, "%s: %s = %d is outside %s", NAME, name, v, range);
        *msg = buf;
        return MIMEO_ERR_ARG;
    };
    if (p->min_len < 2 || p->min_len > MAX_LEN) return bad("min_len", p->min_len, "2 .. 32");
    if (p->max_len < p->min_len || p->max_len > MAX_LEN) return bad("max_len", p->max_len, "min_len .. 32");
    if (p->slack < 0 || p->slack > MAX_SLACK) return bad("slack", p->slack, "0 .. 8");
    if (p->max_mismatch < 0 || p->max_mismatch > MAX_MISMATCH) return bad("max_mismatch", p->max_mismatch, "0 .. 2");
    for (int k = 0; k < 4; k++)
        if (p->reserved[k]) {
            *msg = std::string(NAME) + ": reserved must be 0";
            return MIMEO_ERR_ARG;
        }
    return MIMEO_OK;
}

// every item inside its scaffold; the message starts with `name` and names the first one that is not (K19 shares it)
inline bool validate_items(const char *name, const std::vector<uint64_t> &len, const mimeo_interval *iv, uint64_t n, std::string *msg) {
    char buf[240];
    for (uint64_t k = 0; k < n; k++) {
        if (iv[k].chrom >= len.size()) {
            snprintf(buf, sizeof buf, "%s: item %llu: chrom %u is outside the genome (%zu scaffolds)", name, (unsigned long long)k, iv[k].chrom, len.size());
            *msg = buf;
            return false;
        }
        if (iv[k].start > iv[k].end || iv[k].end > len[iv[k].chrom]) {
            snprintf(buf, sizeof buf, "%s: item %llu: [%u, %u) is not an interval of scaffold %u (%llu bases)", name, (unsigned long long)k, iv[k].start,
                     iv[k].end, iv[k].chrom, (unsigned long long)len[iv[k].chrom]);
            *msg = buf;
            return false;
        }
    }
    return true;
}

// ---- the order of the candidates as one word ---------------------------------------------------------------------------------
// Larger is better: v, then the smaller |dl| + |dr|, the smaller m, the smaller dl, the smaller dr.  v >= 2, so a key is never 0:
// 0 is "no candidate".  v <= 32 (6 bits), |dl| + |dr| <= 16 (5), m <= 2 (2), dl and dr in -8 .. 8 (5 each).
MIMEO_FLANK_HD inline uint32_t pack_key(uint32_t v, int32_t dl, int32_t dr, uint32_t m) {
    const uint32_t sum = (uint32_t)((dl < 0 ? -dl : dl) + (dr < 0 ? -dr : dr));
    return (v << 17) | ((16u - sum) << 12) | ((2u - m) << 10) | ((uint32_t)(8 - dl) << 5) | (uint32_t)(8 - dr);
}
// the record of a key for the item [start, end)
MIMEO_FLANK_HD inline mimeo_flank_repeat unpack_key(uint32_t key, uint32_t start, uint32_t end) {
    mimeo_flank_repeat r{};
    if (!key) return r;
    const uint32_t v = key >> 17, m = 2u - ((key >> 10) & 3u);
    const int32_t dl = 8 - (int32_t)((key >> 5) & 31u), dr = 8 - (int32_t)(key & 31u);
    const uint32_t k = v + (uint32_t)MISMATCH_CHARGE * m;
    r.left_start = (uint32_t)((int64_t)start + dl - (int64_t)k);
    r.right_start = (uint32_t)((int64_t)end + dr);
    r.len = (uint16_t)k;
    r.mismatches = (uint16_t)m;
    r.dl = (int8_t)dl;
    r.dr = (int8_t)dr;
    return r;
}
// Of the candidates of one row, run length and mismatch count — bit b of `w` (b <= 2 slack): dr = b - slack is one — the dr
// that the order prefers: the smallest |dr|, of two the negative one.  w != 0.
MIMEO_FLANK_HD inline int32_t best_dr(uint32_t w, int32_t slack) {
    const uint32_t low = w & ((2u << slack) - 1u), high = w >> (slack + 1);   // dr <= 0, dr > 0
    const int32_t dneg = low ? slack - (31 - __builtin_clz(low)) : 99, dpos = high ? __builtin_ctz(high) + 1 : 99;
    return dneg <= dpos ? -dneg : dpos;
}

}  // namespace flank_host
}  // namespace mimeo
