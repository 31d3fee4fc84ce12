// Stand-alone check of mimeo_amd/csrc/flank_host.h and frames_host.h (the HIP-free host sides of mimeo_flank_repeats, K18, and
// mimeo_open_frames, K19) under the CPU sanitizers: every check with its message, the packed key against the header's order, the
// choice of dr, the chunk cut at tiny chunks, and the monoid — words, combine in every bracketing, chunks — against a plain scan.
// Built and run by tests/test_host_elements.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>
#include <tuple>

#include "../../mimeo_amd/csrc/frames_host.h"

using namespace mimeo;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
    rng_state ^= rng_state >> 12; rng_state ^= rng_state << 25; rng_state ^= rng_state >> 27;
    return rng_state * 0x2545F4914F6CDD1Dull;
}

static void expect_param(void (*change)(mimeo_flank_params *), const char *text) {
    mimeo_flank_params p;
    flank_host::defaults(&p);
    change(&p);
    std::string msg;
    const int rc = flank_host::check_params(&p, &msg);
    if (rc != MIMEO_ERR_ARG || msg.find(text) == std::string::npos || msg.find("mimeo_flank_repeats: ") != 0) {
        fprintf(stderr, "expected '%s', got %d '%s'\n", text, rc, msg.c_str());
        exit(1);
    }
}

static void params() {
    mimeo_flank_params p;
    memset(&p, 0xff, sizeof p);
    flank_host::defaults(&p);
    CHECK(p.min_len == 4 && p.max_len == 20 && p.slack == 2 && p.max_mismatch == 0 && !p.reserved[0] && !p.reserved[1] && !p.reserved[2] && !p.reserved[3]);
    std::string msg;
    CHECK(flank_host::check_params(&p, &msg) == MIMEO_OK && msg.empty());
    expect_param([](mimeo_flank_params *q) { q->min_len = 1; }, "min_len = 1 is outside 2 .. 32");
    expect_param([](mimeo_flank_params *q) { q->min_len = 33; q->max_len = 33; }, "min_len = 33 is outside 2 .. 32");
    expect_param([](mimeo_flank_params *q) { q->max_len = 3; }, "max_len = 3 is outside min_len .. 32");
    expect_param([](mimeo_flank_params *q) { q->max_len = 33; }, "max_len = 33 is outside min_len .. 32");
    expect_param([](mimeo_flank_params *q) { q->slack = -1; }, "slack = -1 is outside 0 .. 8");
    expect_param([](mimeo_flank_params *q) { q->slack = 9; }, "slack = 9 is outside 0 .. 8");
    expect_param([](mimeo_flank_params *q) { q->max_mismatch = -1; }, "max_mismatch = -1 is outside 0 .. 2");
    expect_param([](mimeo_flank_params *q) { q->max_mismatch = 3; }, "max_mismatch = 3 is outside 0 .. 2");
    expect_param([](mimeo_flank_params *q) { q->reserved[0] = 1; }, "reserved must be 0");
    expect_param([](mimeo_flank_params *q) { q->reserved[3] = -1; }, "reserved must be 0");
    p.min_len = 2; p.max_len = 2; p.slack = 0; p.max_mismatch = 2;
    CHECK(flank_host::check_params(&p, &msg) == MIMEO_OK);
    p.min_len = 32; p.max_len = 32; p.slack = 8;
    CHECK(flank_host::check_params(&p, &msg) == MIMEO_OK);
    CHECK(frames_host::check_flags(0, &msg) == MIMEO_OK && msg.empty());
    CHECK(frames_host::check_flags(4, &msg) == MIMEO_ERR_ARG && msg == "mimeo_open_frames: flags = 4 must be 0");
}

static void items() {
    const std::vector<uint64_t> len = {100, 7, 0};
    std::string msg;
    const mimeo_interval good[] = {{0, 0, 100}, {0, 50, 50}, {1, 0, 7}, {1, 7, 7}, {2, 0, 0}};
    CHECK(flank_host::validate_items(flank_host::NAME, len, good, 5, &msg) && msg.empty());
    CHECK(flank_host::validate_items(frames_host::NAME, len, nullptr, 0, &msg));
    auto bad = [&](mimeo_interval x, const char *text) {
        for (const char *name : {flank_host::NAME, frames_host::NAME}) {
            mimeo_interval iv[3] = {good[0], good[2], x};
            std::string m;
            if (flank_host::validate_items(name, len, iv, 3, &m) || m.find(text) == std::string::npos || m.find(std::string(name) + ": item 2: ") != 0) {
                fprintf(stderr, "expected '%s', got '%s'\n", text, m.c_str());
                exit(1);
            }
        }
    };
    bad({3, 0, 0}, "chrom 3 is outside the genome (3 scaffolds)");
    bad({0xFFFFFFFFu, 0, 0}, "chrom 4294967295 is outside the genome");
    bad({0, 11, 10}, "[11, 10) is not an interval of scaffold 0 (100 bases)");
    bad({0, 0, 101}, "[0, 101) is not an interval of scaffold 0 (100 bases)");
    bad({2, 0, 1}, "[0, 1) is not an interval of scaffold 2 (0 bases)");
}

// the packed key orders every pair of candidates as the header does, and comes back as the record
static void keys() {
    typedef std::tuple<int, int, int, int, int> Order;   // -v, |dl| + |dr|, m, dl, dr: smaller is better
    std::vector<std::pair<Order, uint32_t>> all;
    for (int k = 2; k <= 32; k++)
        for (int m = 0; m <= 2; m++)
            for (int dl = -8; dl <= 8; dl++)
                for (int dr = -8; dr <= 8; dr++) {
                    const int v = k - 3 * m;
                    if (v < 2) continue;
                    const uint32_t key = flank_host::pack_key((uint32_t)v, dl, dr, (uint32_t)m);
                    CHECK(key != 0);
                    all.emplace_back(Order(-v, abs(dl) + abs(dr), m, dl, dr), key);
                    const mimeo_flank_repeat r = flank_host::unpack_key(key, 1000, 2000);
                    CHECK(r.len == k && r.mismatches == m && r.dl == dl && r.dr == dr && r.reserved == 0);
                    CHECK(r.left_start == (uint32_t)(1000 + dl - k) && r.right_start == (uint32_t)(2000 + dr));
                }
    for (int t = 0; t < 200000; t++) {
        const auto &x = all[rnd() % all.size()], &y = all[rnd() % all.size()];
        CHECK((x.first < y.first) == (x.second > y.second) && (x.first == y.first) == (x.second == y.second));
    }
    const mimeo_flank_repeat none = flank_host::unpack_key(0, 5, 9);
    const char zero[sizeof none] = {};
    CHECK(!memcmp(&none, zero, sizeof none));
    const mimeo_flank_repeat edge = flank_host::unpack_key(flank_host::pack_key(2, -8, 8, 0), 10, 0xFFFFFFF0u);   // no wrap in 32 bits on the way
    CHECK(edge.left_start == 0 && edge.right_start == 0xFFFFFFF8u);
    for (int slack = 0; slack <= 8; slack++)
        for (uint32_t w = 1; w < (2u << (2 * slack)); w += 1 + (uint32_t)(rnd() % 3) * (slack > 5)) {
            int best = 99;
            for (int b = 0; b <= 2 * slack; b++)
                if ((w >> b) & 1u) {
                    const int dr = b - slack;
                    if (best == 99 || abs(dr) < abs(best) || (abs(dr) == abs(best) && dr < best)) best = dr;
                }
            CHECK(flank_host::best_dr(w, slack) == best);
        }
}

// ---- K19 -----------------------------------------------------------------------------------------------------------------------

// frame phi of a stretch of m bases whose closed codon starts are closed[x]: the header's record, by a plain scan
static frames_host::Monoid scan(const std::vector<uint8_t> &closed, uint32_t m, uint32_t phi) {
    frames_host::Monoid r{};
    const uint32_t T = m >= phi ? (m - phi) / 3 : 0;
    uint32_t run = 0;
    for (uint32_t t = 0; t < T; t++) {
        run = closed[phi + 3 * t] ? 0 : run + 1;
        if (run > r.best) { r.best = run; r.bs = t + 1 - run; }
    }
    return r;
}

static void monoid() {
    using namespace frames_host;
    CHECK(chunk_bases(0) == 65536 && chunk_bases(1) == 4096 && chunk_bases(4096) == 4096 && chunk_bases(4097) == 8192 && chunk_bases(~0ull) == (1u << 30));
    CHECK(chunks_of(0, 4096) == 0 && chunks_of(2, 4096) == 0 && chunks_of(3, 4096) == 1 && chunks_of(4098, 4096) == 1 && chunks_of(4099, 4096) == 2);
    for (int trial = 0; trial < 300; trial++) {
        const uint32_t m = trial < 70 ? (uint32_t)trial : (uint32_t)(rnd() % 20000);
        const uint32_t density = (uint32_t)(rnd() % 4);   // closed codons from none to one in two
        std::vector<uint8_t> closed(m + 130, 1);
        for (uint32_t x = 0; x < m; x++) closed[x] = density == 0 ? 0 : rnd() % (density == 1 ? 60 : density == 2 ? 8 : 2) == 0;
        const uint32_t chunk = chunk_bases(4096u * (1 + rnd() % 3));
        const uint32_t nc = chunks_of(m, chunk);
        for (uint32_t phi = 0; phi < 3; phi++) {
            Monoid total{};
            std::vector<Monoid> words;
            for (uint32_t c = 0; c < nc; c++) {   // the chunk job: steps of 64 words, a tree over the lanes, a carry over the steps
                const uint32_t x0 = c * chunk, limit = x0 + std::min(chunk, m - 2 - x0);
                Monoid carry{};
                for (uint32_t x = x0; x < limit; x += STEP) {
                    Monoid lane[64];
                    for (uint32_t l = 0; l < 64; l++) {
                        const uint32_t X = x + 64 * l, vb = X < limit ? std::min(64u, limit - X) : 0;
                        uint64_t bits = rnd();   // what lies behind the valid starts must not matter
                        for (uint32_t b = 0; b < vb; b++) bits = (bits & ~(1ull << b)) | ((uint64_t)closed[X + b] << b);
                        lane[l] = word_monoid(bits, vb, X, phi);
                        words.push_back(lane[l]);
                    }
                    for (uint32_t d = 1; d < 64; d <<= 1)
                        for (uint32_t l = 0; l < 64; l += 2 * d) lane[l] = combine(lane[l], lane[l + d]);
                    carry = combine(carry, lane[0]);
                }
                total = combine(total, carry);
            }
            const Monoid want = scan(closed, m, phi);
            CHECK(total.best == want.best && (!want.best || total.bs == want.bs));
            CHECK(total.n == (m >= phi + 3 ? (m - phi) / 3 : 0));
            // any bracketing gives the same: fold from the right, and from a random split
            Monoid right{};
            for (size_t k = words.size(); k-- > 0;) right = combine(words[k], right);
            CHECK(!memcmp(&right, &total, sizeof total) || (!total.n && !right.n));
            if (!words.empty()) {
                const size_t cut = rnd() % words.size();
                Monoid a{}, b{};
                for (size_t k = 0; k < cut; k++) a = combine(a, words[k]);
                for (size_t k = cut; k < words.size(); k++) b = combine(b, words[k]);
                const Monoid ab = combine(a, b);
                CHECK(!memcmp(&ab, &total, sizeof total) || (!total.n && !ab.n));
            }
            for (uint32_t sigma = 0; sigma < 2; sigma++) {
                const mimeo_open_frame r = record(total, 1000, 1000 + m, sigma, phi);
                if (!want.best) { CHECK(!r.start && !r.end && !r.codons && !r.met); continue; }
                CHECK(r.codons == want.best && r.met == want.best && r.end - r.start == 3 * want.best && r.start >= 1000 && r.end <= 1000 + m);
                CHECK(sigma ? r.end == 1000 + m - phi - 3 * want.bs : r.start == 1000 + phi + 3 * want.bs);
            }
        }
    }
}

static void jobs() {
    using namespace frames_host;
    const std::vector<uint64_t> len = {20000, 300};
    const mimeo_interval iv[] = {{0, 100, 102}, {0, 0, 20000}, {1, 0, 300}, {1, 7, 7}, {0, 9000, 13099}, {1, 1, 4}};
    std::vector<Job> jobs;
    std::vector<uint32_t> first;
    plan_jobs(iv, len, 4096, 0, 6, jobs, first);
    CHECK(first.size() == 13 && first[0] == 0 && first[2] == 0 && first[12] == jobs.size());
    CHECK(jobs.size() == 2 * (0 + 5 + 1 + 0 + 2 + 1));
    std::set<uint32_t> slots;
    for (size_t k = 0; k < jobs.size(); k++) {
        const Job &j = jobs[k];
        CHECK(!k || jobs[k - 1].bases >= j.bases);
        CHECK(slots.insert(j.slot).second && j.slot < jobs.size() && j.bases >= 1 && j.bases <= 4096 && j.x0 % 4096 == 0 && j.x0 + j.bases <= j.m - 2);
        uint32_t item = 0;
        while (!(first[2 * item + j.strand] <= j.slot && j.slot < first[2 * item + j.strand + 1])) item++;
        const mimeo_interval &x = iv[item];
        CHECK(j.chrom == x.chrom && j.m == x.end - x.start && j.origin == (j.strand ? len[x.chrom] - x.end : x.start));
        CHECK(j.x0 == (j.slot - first[2 * item + j.strand]) * 4096u && (uint64_t)j.origin + j.m <= len[x.chrom]);
    }
    plan_jobs(iv, len, 4096, 3, 4, jobs, first);
    CHECK(jobs.empty() && first.size() == 3 && first[2] == 0);
    auto L = plan_launches(iv, 6, 4096);
    CHECK(L.size() == 1 && L[0].first == 0 && L[0].second == 6);
    L = plan_launches(iv, 6, 4096, 4);   // jobs 0, 10, 2, 0, 4, 2 at four a launch: {0} | {10} | {2, 0} | {4} | {2} — an item with more than the cap goes alone
    CHECK(L.size() == 5 && L[1].first == 1 && L[1].second == 2 && L[2].second == 4 && L[3].second == 5);
    L = plan_launches(iv, 6, 4096, ~0ull, 2);
    CHECK(L.size() == 3 && L[2].first == 4);
    CHECK(plan_launches(iv, 0, 4096).empty());
}

int main() {
    params();
    items();
    keys();
    monoid();
    jobs();
    printf("elements_check: ok\n");
    return 0;
}
