// The host side of mimeo_path_text (mimeo_amd/csrc/path_text_host.h: validate, columns_of, row_first_of, block_columns,
// plan_slices, plan_jobs) under the CPU sanitizers: every refusal carries the new entry point's name, the column counts do not
// wrap beyond 2^32, and the slices and jobs cover every column of every alignment exactly once, with the cuts on multiples of
// 16 output columns.  Built and run by tests/test_host_path_text.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/path_text_host.h"

using namespace mimeo::path_text_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "path_text_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{1000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    bool ok(std::string *msg) const { return validate(len_t, len_q, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), msg); }
};

static Call valid() {
    Call c;
    c.add(0, 0, 0, {{100, 50, 20}, {120, 73, 15}, {140, 88, 20}});   // an insertion, then a deletion
    c.add(1, 0, 1, {{0, 0, 1}});                                       // starts at base 0
    c.add(0, 0, 1, {{990, 790, 10}});                                  // ends on the last base of both scaffolds
    c.add(1, 1, 0, {});                                                // no blocks: no columns
    c.add(1, 0, 0, {{10, 10, 5}, {15, 20, 5}, {30, 25, 5}});           // touching in t, then in q
    return c;
}

static void refused(const Call &c, const char *record, const char *block, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.rfind("mimeo_path_text: ", 0) != 0 || msg.find(record) == std::string::npos || (block && msg.find(block) == std::string::npos) ||
        msg.find(why) == std::string::npos) {
        fprintf(stderr, "path_text_check: line %d: expected a refusal 'mimeo_path_text: ...' naming '%s' '%s' '%s', got '%s'\n", line, record,
                block ? block : "", why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, record, block, why) refused(c, record, block, why, __LINE__)

// the shapes of tests/test_gpu_path_text.py: paths only (t and q), no sequences
struct Shapes {
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    void add(const std::vector<mimeo_path_block> &b) { blk.insert(blk.end(), b.begin(), b.end()); first.push_back(blk.size()); }
    uint64_t n() const { return first.size() - 1; }
};
static Shapes shapes() {
    Shapes s;
    std::mt19937 rng(5);
    const uint32_t mods[] = {0, 1, 31, 32, 33, 63}, lens[] = {1, 15, 16, 17, 31, 32, 33, 63, 64, 65, 127, 128, 129}, gaps[] = {0, 1, 15, 16, 17, 63, 64, 65};
    for (uint32_t tm : mods)
        for (uint32_t qm : mods) {
            std::vector<mimeo_path_block> b;
            uint32_t t = 192 + tm, q = 320 + qm;
            for (uint32_t len : lens) { b.push_back({t, q, len}); const uint32_t step = 64 * ((len + 1 + 63) / 64); t += step; q += step; }
            s.add(b);
        }
    for (uint32_t dq : gaps)
        for (uint32_t dt : gaps) {
            if (!dq && !dt) continue;
            s.add({{100, 200, 40}, {140 + dt, 240 + dq, 33}, {173 + 2 * dt, 273 + 2 * dq, 1}});
        }
    {   // one-column blocks with one-base gaps between them
        std::vector<mimeo_path_block> b;
        uint32_t t = 50, q = 70;
        for (int k = 0; k < 120; k++) { b.push_back({t, q, 1}); t += 1 + (k % 3 != 1); q += 1 + (k % 3 != 0); }
        s.add(b);
    }
    for (uint32_t nb : {1u, 64u, 65u, 200u}) {
        std::vector<mimeo_path_block> b;
        uint32_t t = 3, q = 17;
        for (uint32_t k = 0; k < nb; k++) { const uint32_t len = 1 + rng() % 90, kind = rng() % 3; b.push_back({t, q, len}); t += len + (kind != 0 ? 1 + rng() % 3 : 0); q += len + (kind != 1 ? 1 + rng() % 3 : 0); }
        s.add(b);
    }
    s.add({{33, 1, 10000}});
    s.add({{64, 127, 9000}, {9070, 9127, 10000}});
    s.add({});
    for (int i = 0; i < 3000; i++) {
        std::vector<mimeo_path_block> b;
        uint32_t t = rng() % 5000, q = rng() % 5000;
        const uint32_t nb = 1 + rng() % 4;
        for (uint32_t k = 0; k < nb; k++) { const uint32_t len = 1 + rng() % 200, kind = rng() % 3; b.push_back({t, q, len}); t += len + (kind != 0 ? 1 + rng() % 3 : 0); q += len + (kind != 1 ? 1 + rng() % 3 : 0); }
        s.add(b);
    }
    return s;
}

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    CHECK(validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, &msg));   // n == 0: nothing is looked at
    // every refusal of path_stats_host::validate, under the new name
    {
        std::string m2;
        CHECK(!validate(c.len_t, c.len_q, nullptr, 1, c.first.data(), c.blk.data(), c.blk.size(), &m2) && m2 == "mimeo_path_text: null argument");
        // ... and the old entry point keeps its own
        CHECK(!mimeo::path_stats_host::validate(c.len_t, c.len_q, nullptr, 1, c.first.data(), c.blk.data(), c.blk.size(), &m2) && m2 == "mimeo_path_stats: null argument");
        Call d = valid(); d.blk[1].len = 0;
        CHECK(!mimeo::path_stats_host::validate(d.len_t, d.len_q, d.aln.data(), d.aln.size(), d.first.data(), d.blk.data(), d.blk.size(), &m2) &&
              m2 == "mimeo_path_stats: record 0, block 1 (t 120, q 73, len 0): len is 0");
        CHECK(!d.ok(&m2) && m2 == "mimeo_path_text: record 0, block 1 (t 120, q 73, len 0): len is 0");
    }
    c = valid(); c.first[2] = 2;
    REFUSED(c, "record 1:", nullptr, "path_first decreases");
    c = valid(); c.first.back() += 1;
    REFUSED(c, "record 4:", nullptr, "path_first[n] is not nblocks");
    c = valid(); c.first[0] = 1;
    REFUSED(c, "record 0:", nullptr, "path_first[0] is not 0");
    c = valid(); c.blk[1].len = 0;
    REFUSED(c, "record 0,", "block 1 ", "len is 0");
    c = valid(); c.blk[4].t = 991;
    REFUSED(c, "record 2,", "block 4 ", "beyond the target scaffold");
    c = valid(); c.blk[4].q = 791;
    REFUSED(c, "record 2,", "block 4 ", "beyond the query scaffold");
    c = valid(); c.blk[3].t = 0xFFFFFFF0u; c.blk[3].len = 0x20u;
    REFUSED(c, "record 1,", "block 3 ", "beyond the target scaffold");
    c = valid(); c.add(1, 1, 0, {{0, 0xFFFFFFF0u, 0x20u}});
    REFUSED(c, "record 5,", "block 8 ", "beyond the query scaffold");
    c = valid(); c.blk[1].t = 119;
    REFUSED(c, "record 0,", "block 1 ", "overlaps");
    c = valid(); c.blk[2].q = 87;
    REFUSED(c, "record 0,", "block 2 ", "overlaps");
    c = valid(); std::swap(c.blk[0], c.blk[1]);
    REFUSED(c, "record 0,", "block 1 ", "overlaps");
    c = valid(); c.aln[2].qstrand = 2;
    REFUSED(c, "record 2:", nullptr, "qstrand");
    c = valid(); c.aln[3].tid = 2;
    REFUSED(c, "record 3:", nullptr, "tid");
    c = valid(); c.aln[3].qid = 0xFFFFFFFFu;
    REFUSED(c, "record 3:", nullptr, "qid");

    // column counts by hand: 20 + 3 I + 15 + 5 D + 20 = 63; 1; 10; 0; 5 + 5 I + 5 + 10 D + 5 = 30
    c = valid();
    std::vector<uint64_t> rf(c.aln.size() + 1);
    row_first_of(c.first.data(), c.blk.data(), c.aln.size(), rf.data());
    CHECK((rf == std::vector<uint64_t>{0, 63, 64, 74, 74, 104}));
    std::vector<uint64_t> bcol;
    block_columns(c.first.data(), c.blk.data(), 0, c.aln.size(), bcol);
    CHECK((bcol == std::vector<uint64_t>{0, 20, 38, 0, 0, 0, 5, 15}));
    block_columns(c.first.data(), c.blk.data(), 4, 5, bcol);
    CHECK((bcol == std::vector<uint64_t>{0, 5, 15}));
    // spans just below 2^31 on both sides: two one-base blocks at the ends of a target and a query of 2^31 - 1 bases, twice:
    // 2 * (2^31 - 1) - 2 = 2^32 - 4 columns each, and row_first beyond 2^32
    {
        const uint32_t L = 0x7FFFFFFFu;
        Call big;
        big.len_t = {L}; big.len_q = {L};
        big.add(0, 0, 0, {{0, 0, 1}, {L - 1, L - 1, 1}});
        big.add(0, 0, 1, {{0, 0, 1}, {L - 1, L - 1, 1}});
        big.add(0, 0, 0, {{5, 7, 3}});
        CHECK(big.ok(&msg));
        CHECK(columns_of(big.first.data(), big.blk.data(), 0) == 0xFFFFFFFCull);
        std::vector<uint64_t> r(4);
        row_first_of(big.first.data(), big.blk.data(), 3, r.data());
        CHECK(r[1] == 0xFFFFFFFCull && r[2] == 0x1FFFFFFF8ull && r[3] == 0x1FFFFFFFBull);
        block_columns(big.first.data(), big.blk.data(), 0, 3, bcol);
        CHECK(bcol[1] == 1 && bcol[3] == 1 && bcol[4] == 0);
        // the over-long alignments are slices of their own, and their jobs tile them
        const auto sl = plan_slices(r.data(), big.first.data(), 3, SLICE_RECORDS, SLICE_BLOCKS, DEFAULT_SLICE_COLUMNS);
        CHECK(sl.size() == 3 && sl[0].second == 1 && sl[1].second == 2);
        std::vector<Job> jobs;
        plan_jobs(r.data(), 1, 2, 1ull << 30, jobs);
        CHECK(jobs.size() >= 4 && jobs[0].c0 == 0 && jobs.back().c1 == 0xFFFFFFFCull);
        for (size_t j = 0; j + 1 < jobs.size(); j++) CHECK(jobs[j].c1 == jobs[j + 1].c0 && (r[1] + jobs[j].c1) % 16 == 0 && jobs[j].c1 - jobs[j].c0 <= (1ull << 30));
    }

    // the slice and job plans over the shapes of the GPU test: every column of every alignment exactly once
    const Shapes s = shapes();
    const uint64_t n = s.n();
    std::vector<uint64_t> row_first(n + 1);
    row_first_of(s.first.data(), s.blk.data(), n, row_first.data());
    for (uint64_t i = 0; i < n; i++) {   // the count against a walk of the blocks
        uint64_t cols = 0;
        for (uint64_t k = s.first[i]; k < s.first[i + 1]; k++) {
            if (k > s.first[i]) cols += (s.blk[k].t - (s.blk[k - 1].t + s.blk[k - 1].len)) + (s.blk[k].q - (s.blk[k - 1].q + s.blk[k - 1].len));
            cols += s.blk[k].len;
        }
        CHECK(row_first[i + 1] - row_first[i] == cols);
    }
    size_t total_jobs = 0, cut_rows = 0, lone_slices = 0;
    for (uint64_t budget : {(uint64_t)1, (uint64_t)17, (uint64_t)4096, DEFAULT_SLICE_COLUMNS})
        for (uint64_t split : {(uint64_t)16, (uint64_t)48, (uint64_t)0, DEFAULT_SPLIT_COLUMNS}) {
            const auto slices = plan_slices(row_first.data(), s.first.data(), n, SLICE_RECORDS, SLICE_BLOCKS, budget);
            uint64_t at = 0;
            std::vector<Job> jobs;
            for (const auto &sl : slices) {
                CHECK(sl.first == at && sl.second > sl.first && sl.second <= n);
                const uint64_t cols = row_first[sl.second] - row_first[sl.first];
                CHECK(cols <= budget || sl.second - sl.first == 1);   // an alignment beyond the budget is a slice of its own
                lone_slices += cols > budget;
                plan_jobs(row_first.data(), sl.first, sl.second, split, jobs);
                block_columns(s.first.data(), s.blk.data(), sl.first, sl.second, bcol);
                CHECK(bcol.size() == s.first[sl.second] - s.first[sl.first]);
                size_t j = 0;
                for (uint64_t i = sl.first; i < sl.second; i++) {
                    const uint64_t c = row_first[i + 1] - row_first[i];
                    if (s.first[i + 1] > s.first[i]) CHECK(bcol[s.first[i] - s.first[sl.first]] == 0 && bcol[s.first[i + 1] - 1 - s.first[sl.first]] + s.blk[s.first[i + 1] - 1].len <= c);
                    uint64_t c0 = 0;
                    const size_t j0 = j;
                    while (c0 < c) {   // an alignment without columns has no job
                        CHECK(j < jobs.size() && jobs[j].aln == i - sl.first && jobs[j].c0 == c0 && jobs[j].c1 > c0 && jobs[j].c1 <= c);
                        if (split) CHECK(c <= split || jobs[j].c1 - jobs[j].c0 <= (split < 16 ? 16 : split));
                        if (jobs[j].c1 < c) CHECK((row_first[i] + jobs[j].c1) % 16 == 0);   // a cut: on a multiple of 16 output columns
                        c0 = jobs[j].c1;
                        j++;
                    }
                    if (!split || c <= split) CHECK(j - j0 == (c ? 1u : 0u));
                    cut_rows += j - j0 > 1;
                }
                CHECK(j == jobs.size());
                total_jobs += j;
                at = sl.second;
            }
            CHECK(at == n);
        }
    CHECK(cut_rows > 0 && lone_slices > 0);
    printf("path_text_check: ok %zu jobs, %zu cut rows, %zu slices of one over-long alignment\n", total_jobs, cut_rows, lone_slices);
    return 0;
}
