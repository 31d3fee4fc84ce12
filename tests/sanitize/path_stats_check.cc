// The host side of mimeo_path_stats (mimeo_amd/csrc/path_stats_host.h: validate, plan_slices, plan_jobs) under the CPU
// sanitizers: valid paths are accepted, every kind of bad path is refused with the record (and the block) named, and the
// slices and jobs cover a call exactly once.  Built and run by tests/test_host_divergence.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/path_stats_host.h"

using namespace mimeo::path_stats_host;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "path_stats_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

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
    c.add(1, 1, 0, {});                                                // no blocks: counts nothing
    c.add(1, 0, 0, {{10, 10, 5}, {15, 20, 5}, {30, 25, 5}});           // touching in t, then in q
    return c;
}

static void refused(const Call &c, const char *record, const char *block, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find(record) == std::string::npos || (block && msg.find(block) == std::string::npos) || msg.find(why) == std::string::npos) {
        fprintf(stderr, "path_stats_check: line %d: expected a refusal naming '%s' '%s' '%s', got '%s'\n", line, record, block ? block : "", why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, record, block, why) refused(c, record, block, why, __LINE__)

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    CHECK(validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, &msg));   // n == 0: nothing is looked at
    // a non-monotone first
    c = valid(); c.first[2] = 2;
    REFUSED(c, "record 1:", nullptr, "path_first decreases");
    // first[n] != nblocks (also one block too many: nothing beyond blocks[nblocks) is read)
    c = valid(); c.first.back() += 1;
    REFUSED(c, "record 4:", nullptr, "path_first[n] is not nblocks");
    c = valid(); c.first[0] = 1;
    REFUSED(c, "record 0:", nullptr, "path_first[0] is not 0");
    // a block with len == 0
    c = valid(); c.blk[1].len = 0;
    REFUSED(c, "record 0,", "block 1 ", "len is 0");
    // t + len == Lt + 1
    c = valid(); c.blk[4].t = 991;
    REFUSED(c, "record 2,", "block 4 ", "beyond the target scaffold");
    c = valid(); c.blk[4].q = 791;
    REFUSED(c, "record 2,", "block 4 ", "beyond the query scaffold");
    // 32-bit wrap: t = 0xFFFFFFF0 with len = 0x20 is base 0x10 in 32 bits
    c = valid(); c.blk[3].t = 0xFFFFFFF0u; c.blk[3].len = 0x20u;
    REFUSED(c, "record 1,", "block 3 ", "beyond the target scaffold");
    // ... and on the query side, against a scaffold of 2^32 - 1 bases
    c = valid(); c.add(1, 1, 0, {{0, 0xFFFFFFF0u, 0x20u}});
    REFUSED(c, "record 5,", "block 8 ", "beyond the query scaffold");
    // overlapping blocks, and blocks in the wrong order
    c = valid(); c.blk[1].t = 119;
    REFUSED(c, "record 0,", "block 1 ", "overlaps");
    c = valid(); c.blk[2].q = 87;
    REFUSED(c, "record 0,", "block 2 ", "overlaps");
    c = valid(); std::swap(c.blk[0], c.blk[1]);
    REFUSED(c, "record 0,", "block 1 ", "overlaps");
    // qstrand == 2, tid and qid out of range
    c = valid(); c.aln[2].qstrand = 2;
    REFUSED(c, "record 2:", nullptr, "qstrand");
    c = valid(); c.aln[3].tid = 2;
    REFUSED(c, "record 3:", nullptr, "tid");
    c = valid(); c.aln[3].qid = 0xFFFFFFFFu;
    REFUSED(c, "record 3:", nullptr, "qid");

    // slices and jobs on random calls: every alignment in exactly one slice, within the caps unless it is alone; the jobs of an
    // alignment tile its chunks, and only a cut alignment is marked split
    std::mt19937 rng(11);
    size_t total_jobs = 0;
    for (int rep = 0; rep < 300; rep++) {
        const uint64_t n = rng() % 40;
        std::vector<uint64_t> first{0};
        std::vector<mimeo_path_block> blk;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t nb = rng() % 6;
            uint32_t t = 0;
            for (uint32_t k = 0; k < nb; k++) { const uint32_t len = 1 + rng() % 700; blk.push_back(mimeo_path_block{t, t, len}); t += len + rng() % 3; }
            first.push_back(blk.size());
        }
        const uint64_t max_rec = 1 + rng() % 8, max_blk = rep % 5 == 0 ? 1 : 1 + rng() % 12, split = rep % 4 == 0 ? 0 : 1 + rng() % 9;
        const auto slices = plan_slices(first.data(), n, max_rec, max_blk);
        uint64_t at = 0;
        std::vector<Job> jobs;
        for (const auto &s : slices) {
            CHECK(s.first == at && s.second > s.first && s.second <= n);
            CHECK(s.second - s.first <= max_rec);
            CHECK(s.second - s.first == 1 || first[s.second] - first[s.first] <= max_blk);
            plan_jobs(first.data(), blk.data(), s.first, s.second, split, jobs);
            size_t j = 0;
            for (uint64_t i = s.first; i < s.second; i++) {
                const uint64_t c = chunks_of(first.data(), blk.data(), i);
                uint64_t c0 = 0;
                const size_t j0 = j;
                do {
                    CHECK(j < jobs.size() && jobs[j].aln == i - s.first && jobs[j].c0 == c0 && jobs[j].c1 >= c0 && jobs[j].c1 <= c);
                    CHECK(!split || jobs[j].c1 - jobs[j].c0 <= split);
                    c0 = jobs[j].c1;
                    j++;
                } while (c0 < c);
                for (size_t k = j0; k < j; k++) CHECK(jobs[k].split == (j - j0 > 1 ? 1u : 0u));
            }
            CHECK(j == jobs.size());
            total_jobs += j;
            at = s.second;
        }
        CHECK(at == n);
    }
    printf("path_stats_check: ok %zu jobs\n", total_jobs);
    return 0;
}
