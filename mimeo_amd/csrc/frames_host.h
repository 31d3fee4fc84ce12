// frames_host.h — HIP-free host side of mimeo_open_frames (K19, k19_frames.hip): the checks, the cut of the items into chunk
// jobs, and the monoid of a frame's codons with its combine, the reduction of one 64-base word to it and the record made from
// it (which the kernels share).  Kept apart from the device code so that it runs under the CPU sanitizers
// (tests/sanitize/elements_check.cc, tests/test_host_elements.py).
#pragma once
#include <stdint.h>
#include <stdio.h>

#include <algorithm>
#include <string>
#include <vector>

#include "flank_host.h"

namespace mimeo {
namespace frames_host {

constexpr const char *NAME = "mimeo_open_frames";
constexpr uint32_t STEP = 4096;            // bases of one wavefront step: 64 lanes of 64
constexpr uint32_t DEFAULT_CHUNK = 1u << 16;
constexpr uint64_t MAX_LAUNCH_JOBS = 1ull << 20;   // chunk jobs of one launch, at most
constexpr uint64_t MAX_LAUNCH_ITEMS = 1ull << 22;  // items of one launch, at most: six records each, numbered in 32 bits

inline int check_flags(uint32_t flags, std::string *msg) {
    if (!flags) return MIMEO_OK;
    char buf[120];
    snprintf(buf, sizeof buf, "%s: flags = %u must be 0", NAME, flags);
    *msg = buf;
    return MIMEO_ERR_ARG;
}

// the chunk that is used for a wish (MIMEO_FRAMES_CHUNK; 0: the default): whole steps, one at least, below 2^30
inline uint32_t chunk_bases(uint64_t wish) {
    if (!wish) wish = DEFAULT_CHUNK;
    wish = std::min<uint64_t>(wish, 1u << 30);
    return (uint32_t)((wish + STEP - 1) / STEP * STEP);
}

// ---- the codons of one frame over a stretch, as a monoid -------------------------------------------------------------------
// Codon indices are those of the item's frame (t of the header), so the elements of different chunks combine as they are.
// t0: the first codon of the stretch; n: its codons; pre / suf: the open codons at its start / end; best, bs: its longest run of
// open codons and where it starts, the earliest of equal ones.  n == 0 is the identity.
struct Monoid { uint32_t t0, n, pre, suf, best, bs; };

// a (the earlier stretch) followed by b; associative
MIMEO_FLANK_HD inline Monoid combine(const Monoid &a, const Monoid &b) {
    if (!a.n) return b;
    if (!b.n) return a;
    Monoid r;
    r.t0 = a.t0;
    r.n = a.n + b.n;
    r.pre = a.pre == a.n ? a.n + b.pre : a.pre;
    r.suf = b.suf == b.n ? b.n + a.suf : b.suf;
    const uint32_t cross = a.suf + b.pre;   // the run over the seam starts where a's last run does
    r.best = a.best;
    r.bs = a.bs;
    if (cross > r.best) { r.best = cross; r.bs = b.t0 - a.suf; }
    if (b.best > r.best) { r.best = b.best; r.bs = b.bs; }
    return r;
}

// The codon starts of frame `phi` inside the 64-base word at item offset X (a multiple of 64): bit b of `closed` says that the
// codon that starts at offset X + b is closed, and the first `vb` bits (0 .. 64) are codon starts of the item at all.
MIMEO_FLANK_HD inline Monoid word_monoid(uint64_t closed, uint32_t vb, uint32_t X, uint32_t phi) {
    const uint32_t rho = (phi + 3u - X % 3u) % 3u;   // the first bit of the frame: X + rho = phi (mod 3)
    Monoid r{(X + rho - phi) / 3u, 0u, 0u, 0u, 0u, 0u};
    if (vb <= rho) return r;
    r.n = (vb - rho + 2u) / 3u;
    uint64_t c = closed & (0x9249249249249249ull << rho) & (vb >= 64u ? ~0ull : (1ull << vb) - 1ull);
    uint32_t prev = 0;   // the first codon (counted inside the word) behind the last closed one
    r.pre = c ? ((uint32_t)__builtin_ctzll(c) - rho) / 3u : r.n;
    while (c) {
        const uint32_t u = ((uint32_t)__builtin_ctzll(c) - rho) / 3u;
        if (u - prev > r.best) { r.best = u - prev; r.bs = prev; }
        prev = u + 1u;
        c &= c - 1ull;
    }
    r.suf = r.n - prev;
    if (r.suf > r.best) { r.best = r.suf; r.bs = prev; }
    r.bs += r.t0;
    return r;
}

// the record of (sigma, phi) of the item [start, end) from its frame's element; met is filled in later
MIMEO_FLANK_HD inline mimeo_open_frame record(const Monoid &m, uint32_t start, uint32_t end, uint32_t sigma, uint32_t phi) {
    mimeo_open_frame r{};
    if (!m.best) return r;
    const uint32_t a = phi + 3u * m.bs, b = phi + 3u * (m.bs + m.best);
    r.start = sigma ? end - b : start + a;
    r.end = sigma ? end - a : start + b;
    r.codons = m.best;
    r.met = m.best;
    return r;
}

// ---- the cut into chunk jobs ---------------------------------------------------------------------------------------------------
// One job = one wavefront: the codons of strand `strand` of item `item` (of the launch) that start in [x0, x0 + bases) of the
// item's m bases; origin: the strand's base at item offset 0 (start on fwd, L - end on rc).  Its three elements are
// out[3 * slot + phi]; the slots of an item's strand are consecutive, first_slot .. first_slot + chunks - 1.
struct Job { uint32_t chrom, strand, origin, x0, bases, m, slot, pad; };
MIMEO_FLANK_HD inline uint32_t chunks_of(uint32_t m, uint32_t chunk) { return m < 3u ? 0u : (m - 2u + chunk - 1u) / chunk; }   // codon starts: m - 2

// the items [k0, k1) of one launch: as many as keep the chunk jobs at max_jobs (a single item always goes) and the items at max_items
inline std::vector<std::pair<uint64_t, uint64_t>> plan_launches(const mimeo_interval *iv, uint64_t n, uint32_t chunk, uint64_t max_jobs = MAX_LAUNCH_JOBS,
                                                                uint64_t max_items = MAX_LAUNCH_ITEMS) {
    std::vector<std::pair<uint64_t, uint64_t>> out;
    uint64_t k0 = 0, jobs = 0;
    for (uint64_t k = 0; k < n; k++) {
        const uint64_t j = 2ull * chunks_of(iv[k].end - iv[k].start, chunk);
        if (k > k0 && (jobs + j > max_jobs || k - k0 >= max_items)) {
            out.emplace_back(k0, k);
            k0 = k;
            jobs = 0;
        }
        jobs += j;
    }
    if (k0 < n) out.emplace_back(k0, n);
    return out;
}

// The jobs of the items [k0, k1), the longest first.  first_slot[2 (k - k0) + strand]: the first slot of that strand's chunks.
inline void plan_jobs(const mimeo_interval *iv, const std::vector<uint64_t> &len, uint32_t chunk, uint64_t k0, uint64_t k1, std::vector<Job> &jobs,
                      std::vector<uint32_t> &first_slot) {
    jobs.clear();
    first_slot.assign(2 * (k1 - k0) + 1, 0u);
    uint32_t slot = 0;
    for (uint64_t k = k0; k < k1; k++) {
        const uint32_t m = iv[k].end - iv[k].start, nc = chunks_of(m, chunk);
        for (uint32_t strand = 0; strand < 2u; strand++) {
            first_slot[2 * (k - k0) + strand] = slot;
            const uint32_t origin = strand ? (uint32_t)(len[iv[k].chrom] - iv[k].end) : iv[k].start;
            for (uint32_t c = 0; c < nc; c++) {
                const uint32_t x0 = c * chunk;
                jobs.push_back(Job{iv[k].chrom, strand, origin, x0, std::min(chunk, m - 2u - x0), m, slot++, 0u});
            }
        }
    }
    first_slot[2 * (k1 - k0)] = slot;
    std::stable_sort(jobs.begin(), jobs.end(), [](const Job &x, const Job &y) { return x.bases > y.bases; });
}

}  // namespace frames_host
}  // namespace mimeo
