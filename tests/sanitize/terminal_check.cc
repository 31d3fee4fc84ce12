// Stand-alone check of mimeo_amd/csrc/terminal_host.h (the HIP-free host side of mimeo_terminal_repeats, K17) under the CPU
// sanitizers: every check with its message, the window and the origins at odd and tiny lengths, the layout of the traceback
// scratch, and the cut into launches under tiny budgets.  Built and run by tests/test_host_terminal.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <set>

#include "../../mimeo_amd/csrc/terminal_host.h"

using namespace mimeo;
using namespace mimeo::terminal_host;

#define CHECK(c)                                                                   \
    do {                                                                           \
        if (!(c)) { fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #c); exit(1); } \
    } while (0)

static void expect_param(void (*change)(mimeo_terminal_params *), int code, const char *text) {
    mimeo_terminal_params p;
    defaults(&p);
    change(&p);
    std::string msg;
    const int rc = check_params(&p, &msg);
    if (rc != code || msg.find(text) == std::string::npos || msg.find("mimeo_terminal_repeats: ") != 0) {
        fprintf(stderr, "expected %d '%s', got %d '%s'\n", code, text, rc, msg.c_str());
        exit(1);
    }
}

static void params() {
    mimeo_terminal_params p;
    memset(&p, 0xff, sizeof p);
    defaults(&p);
    CHECK(p.window == 1024 && p.match == 2 && p.mismatch == 3 && p.gap_open == 5 && p.gap_extend == 2 && p.min_score == 40 && !p.reserved[0] && !p.reserved[1]);
    std::string msg;
    CHECK(check_params(&p, &msg) == MIMEO_OK && msg.empty());
    expect_param([](mimeo_terminal_params *q) { q->window = 0; }, MIMEO_ERR_LIMIT, "window = 0 is outside 1 .. 4096");
    expect_param([](mimeo_terminal_params *q) { q->window = 4097; }, MIMEO_ERR_LIMIT, "window = 4097 is outside 1 .. 4096");
    expect_param([](mimeo_terminal_params *q) { q->window = -5; }, MIMEO_ERR_LIMIT, "window = -5");
    expect_param([](mimeo_terminal_params *q) { q->match = 0; }, MIMEO_ERR_ARG, "match = 0 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->match = 1001; }, MIMEO_ERR_ARG, "match = 1001 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->mismatch = 0; }, MIMEO_ERR_ARG, "mismatch = 0 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->mismatch = 1001; }, MIMEO_ERR_ARG, "mismatch = 1001 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->gap_open = -1; }, MIMEO_ERR_ARG, "gap_open = -1 is outside 0 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->gap_open = 1001; }, MIMEO_ERR_ARG, "gap_open = 1001 is outside 0 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->gap_extend = 0; }, MIMEO_ERR_ARG, "gap_extend = 0 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->gap_extend = 1001; }, MIMEO_ERR_ARG, "gap_extend = 1001 is outside 1 .. 1000");
    expect_param([](mimeo_terminal_params *q) { q->min_score = 0; }, MIMEO_ERR_ARG, "min_score = 0 is outside >= 1");
    expect_param([](mimeo_terminal_params *q) { q->reserved[0] = 1; }, MIMEO_ERR_ARG, "reserved must be 0");
    expect_param([](mimeo_terminal_params *q) { q->reserved[1] = -1; }, MIMEO_ERR_ARG, "reserved must be 0");
    // the extremes pass
    expect_param([](mimeo_terminal_params *q) { q->window = 4096; q->match = q->mismatch = q->gap_open = q->gap_extend = 1000; q->min_score = 1; q->window = 0; }, MIMEO_ERR_LIMIT, "window");
    defaults(&p);
    p.window = 4096; p.match = p.mismatch = p.gap_open = p.gap_extend = 1000; p.min_score = 1;
    CHECK(check_params(&p, &msg) == MIMEO_OK);
    p.window = 1; p.match = p.mismatch = p.gap_extend = 1; p.gap_open = 0; p.min_score = 0x7fffffff;
    CHECK(check_params(&p, &msg) == MIMEO_OK);
}

static void items() {
    const std::vector<uint64_t> len = {100, 7, 0};
    std::string msg;
    const mimeo_interval good[] = {{0, 0, 100}, {0, 50, 50}, {1, 0, 7}, {1, 7, 7}, {2, 0, 0}};
    CHECK(validate_items(len, good, 5, &msg) && msg.empty());
    CHECK(validate_items(len, nullptr, 0, &msg));
    auto bad = [&](mimeo_interval x, const char *text) {
        mimeo_interval iv[3] = {good[0], good[2], x};
        std::string m;
        if (validate_items(len, iv, 3, &m) || m.find(text) == std::string::npos || m.find("mimeo_terminal_repeats: item 2: ") != 0) {
            fprintf(stderr, "expected '%s', got '%s'\n", text, m.c_str());
            exit(1);
        }
    };
    bad({3, 0, 0}, "chrom 3 is outside the genome (3 scaffolds)");
    bad({0xFFFFFFFFu, 0, 0}, "chrom 4294967295 is outside the genome");
    bad({0, 11, 10}, "[11, 10) is not an interval of scaffold 0 (100 bases)");
    bad({0, 0, 101}, "[0, 101) is not an interval of scaffold 0 (100 bases)");
    bad({1, 8, 8}, "[8, 8) is not an interval of scaffold 1 (7 bases)");
    bad({2, 0, 1}, "[0, 1) is not an interval of scaffold 2 (0 bases)");
    bad({0, 0xFFFFFFFFu, 0xFFFFFFFFu}, "is not an interval of scaffold 0");
}

static void the_windows() {
    // lengths 0, 1, 2 and 3; odd lengths; the window as the bound and the item as the bound
    struct { mimeo_interval iv; uint64_t len; int32_t window; Windows want; } cases[] = {
        {{0, 5, 5}, 100, 1024, {0, 5, 5, 95}},
        {{0, 5, 6}, 100, 1024, {0, 5, 6, 94}},
        {{0, 5, 7}, 100, 1024, {1, 5, 6, 93}},
        {{0, 5, 8}, 100, 1024, {1, 5, 7, 92}},
        {{0, 0, 100}, 100, 1024, {50, 0, 50, 0}},
        {{0, 0, 99}, 100, 1024, {49, 0, 50, 1}},
        {{0, 1, 100}, 100, 1024, {49, 1, 51, 0}},
        {{0, 0, 100}, 100, 50, {50, 0, 50, 0}},
        {{0, 0, 100}, 100, 49, {49, 0, 51, 0}},
        {{0, 0, 100}, 100, 1, {1, 0, 99, 0}},
        {{0, 10, 90}, 100, 7, {7, 10, 83, 10}},
        {{0, 0, 0}, 0, 4096, {0, 0, 0, 0}},
        {{0, 0, 4000000000u}, 4000000000ull, 4096, {4096, 0, 4000000000u - 4096u, 0}},
        {{0, 3999990000u, 4000000000u}, 4294967295ull, 4096, {4096, 3999990000u, 4000000000u - 4096u, 294967295u}},
    };
    for (const auto &c : cases) {
        const Windows W = windows(c.iv, c.len, c.window);
        CHECK(W.w == c.want.w && W.head == c.want.head && W.direct == c.want.direct && W.inverted == c.want.inverted);
        // all three stretches inside the scaffold, and the head in front of the direct tail
        CHECK((uint64_t)W.head + W.w <= W.direct && (uint64_t)W.direct + W.w <= c.len && (uint64_t)W.inverted + W.w <= c.len);
    }
}

static void scratch() {
    CHECK(trace_words(0) == 0 && strips(1) == 1 && step_groups(1) == 8 && trace_words(1) == 512);
    CHECK(strips(64) == 1 && strips(65) == 2 && step_groups(64) == 16 && step_groups(65) == 16 && step_groups(66) == 17);
    CHECK(trace_words(1024) * 4 == 16u * 136u * 256u && trace_words(4096) * 4 == 64u * 520u * 256u);
    for (uint32_t w : {1u, 2u, 63u, 64u, 65u, 127u, 129u, 200u}) {
        // every cell has a nibble of its own, inside the job's words; a lane's eight steps share a word
        std::set<uint64_t> seen;
        for (uint32_t i = 0; i < w; i++)
            for (uint32_t j = 0; j < w; j++) {
                const uint64_t word = trace_word(w, i, j);
                const uint32_t sh = trace_shift(i, j);
                CHECK(word < trace_words(w) && sh < 32 && sh % 4 == 0);
                CHECK(seen.insert(word * 8 + sh / 4).second);
                CHECK(word % 64 == j % 64);
                if (i + 1 < w && ((i + (j & 63u)) & 7u) != 7u) CHECK(trace_word(w, i + 1, j) == word && trace_shift(i + 1, j) == sh + 4);
            }
        CHECK(job_bytes(w) == trace_words(w) * 4 + 12ull * w);
    }
}

static void launches() {
    const std::vector<uint32_t> w = {10, 0, 200, 200, 1, 4096, 3, 0, 0, 64};
    auto whole = [&](const std::vector<std::pair<uint64_t, uint64_t>> &L) {   // consecutive, none empty, all items
        uint64_t at = 0;
        for (const auto &l : L) { CHECK(l.first == at && l.second > l.first); at = l.second; }
        CHECK(at == w.size());
    };
    auto L = plan_launches(w, ~0ull);
    CHECK(L.size() == 1);
    whole(L);
    for (uint64_t budget : {0ull, 1ull, 1000ull}) {   // a single item always goes; items without a window cost nothing and share a launch
        L = plan_launches(w, budget);
        whole(L);
        CHECK(L.size() == 9 && L[7].first == 7 && L[7].second == 9);
    }
    const uint64_t b200 = 2 * job_bytes(200);
    L = plan_launches(w, 2 * b200 + 2 * job_bytes(10));   // {10, 0, 200, 200} | {1} | {4096} | {3, 0, 0, 64}
    whole(L);
    CHECK(L.size() == 4 && L[0].second == 4 && L[1].second == 5 && L[2].second == 6);
    for (const auto &l : L) {
        uint64_t bytes = 0;
        for (uint64_t k = l.first; k < l.second; k++) bytes += 2 * job_bytes(w[k]);
        CHECK(l.second - l.first == 1 || bytes <= 2 * b200 + 2 * job_bytes(10));
    }
    L = plan_launches(w, ~0ull, 4);   // at most four jobs: two items
    whole(L);
    CHECK(L.size() == 5);
    L = plan_launches(w, ~0ull, 1);
    CHECK(L.size() == w.size());
    CHECK(plan_launches({}, 100).empty());

    // the jobs of a launch: both orientations of every item, the longest windows first, the scratch laid out without overlap
    const std::vector<uint64_t> len = {10000, 300};
    const mimeo_interval iv[] = {{0, 100, 120}, {0, 0, 10000}, {1, 0, 300}, {1, 7, 7}, {0, 9000, 9801}, {1, 0, 299}};
    std::vector<Job> jobs;
    uint64_t tw = 0, nb = 0;
    plan_jobs(iv, len, 256, 1, 6, jobs, &tw, &nb);
    CHECK(jobs.size() == 10);
    uint64_t t = 0, b = 0;
    std::set<uint32_t> slots;
    for (size_t k = 0; k < jobs.size(); k++) {
        const Job &j = jobs[k];
        CHECK(!k || jobs[k - 1].w >= j.w);
        CHECK(j.trace_off == t && j.blk_off == b);
        t += trace_words(j.w);
        b += j.w;
        CHECK(slots.insert(j.slot).second && j.slot < 10 && j.strand == (j.slot & 1u));
        const mimeo_interval &x = iv[1 + j.slot / 2];
        const Windows W = windows(x, len[x.chrom], 256);
        CHECK(j.chrom == x.chrom && j.w == W.w && j.a0 == W.head && j.b0 == (j.strand ? W.inverted : W.direct));
    }
    CHECK(tw == t && nb == b);
    CHECK(jobs[0].w == 256 && jobs[0].slot == 0 && jobs[1].slot == 1 && jobs[2].w == 256 && jobs[2].slot == 6);   // equal windows keep their order
    CHECK(jobs[8].w == 0 && jobs[9].w == 0 && jobs[9].trace_off == tw);
    plan_jobs(iv, len, 256, 3, 4, jobs, &tw, &nb);   // a launch of one item without a window
    CHECK(jobs.size() == 2 && tw == 0 && nb == 0);
    plan_jobs(iv, len, 256, 2, 2, jobs, &tw, &nb);
    CHECK(jobs.empty() && tw == 0 && nb == 0);
}

int main() {
    params();
    items();
    the_windows();
    scratch();
    launches();
    printf("terminal_check: ok\n");
    return 0;
}
