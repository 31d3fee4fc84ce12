// The job list of the tandem scorer beyond 64 periods (mimeo_amd/csrc/host_plan.h: tandem_jobs) under the CPU sanitizers:
// checked against a plain restatement of "which lanes have work" over random lists of slice lengths.
// Built and run by tests/test_tandem_plan.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <utility>
#include <vector>

#include "../../mimeo_amd/csrc/host_plan.h"

using namespace mimeo;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } } while (0)

// the kernel's own test, lane by lane: period p of a slice of L bases has work when L > p - b
static bool lane_live(uint32_t L, uint32_t p, int maxperiod, int delta) {
    if ((int)p > maxperiod) return false;
    const uint32_t b = delta > 0 ? (p == 1 ? 0u : (p < 5 ? 1u : 2u)) : 0u;
    return L > p - b;
}
static bool block_live(uint32_t L, uint32_t block, int maxperiod, int delta) {
    for (uint32_t lane = 0; lane < 64; lane++)
        if (lane_live(L, block * 64 + lane + 1, maxperiod, delta)) return true;
    return false;
}

// the chunks tandem_masked_device uploads: each within the stated device bytes, together the whole list
static void check_chunks(uint64_t njobs) {
    uint64_t covered = 0;
    for (uint64_t j0 = 0; j0 < njobs; j0 += host_plan::TANDEM_CHUNK_JOBS) {
        const uint64_t nj = std::min<uint64_t>(njobs - j0, host_plan::TANDEM_CHUNK_JOBS);
        CHECK(nj >= 1 && nj * sizeof(host_plan::TandemJob) <= host_plan::TANDEM_CHUNK_BYTES);
        covered += nj;
    }
    CHECK(covered == njobs);
}

static size_t check_list(const std::vector<uint32_t> &lengths, int maxperiod, int delta) {
    const std::vector<host_plan::TandemJob> jobs = host_plan::tandem_jobs(lengths, maxperiod, delta);
    std::map<std::pair<uint32_t, uint32_t>, int> seen;
    for (size_t i = 0; i < jobs.size(); i++) {
        CHECK(jobs[i].slice < lengths.size());
        CHECK(block_live(lengths[jobs[i].slice], jobs[i].block, maxperiod, delta));   // no job without a live lane
        CHECK(++seen[std::make_pair(jobs[i].slice, jobs[i].block)] == 1);              // none twice
        if (i) CHECK(lengths[jobs[i].slice] <= lengths[jobs[i - 1].slice]);            // longest slices first
    }
    size_t expect = 0;
    for (size_t s = 0; s < lengths.size(); s++)
        for (uint32_t k = 0; k * 64 < 2048; k++)   // beyond every block that maxperiod <= 2000 can name
            if (block_live(lengths[s], k, maxperiod, delta)) {
                expect++;
                CHECK(seen.count(std::make_pair((uint32_t)s, k)) == 1);               // every live (slice, block) is there
            }
    CHECK(expect == jobs.size());
    check_chunks(jobs.size());
    return jobs.size();
}

int main() {
    static_assert(host_plan::TANDEM_CHUNK_BYTES <= (256ull << 20), "the job list stays under 256 MiB of device memory");
    static_assert(host_plan::TANDEM_CHUNK_JOBS * sizeof(host_plan::TandemJob) <= host_plan::TANDEM_CHUNK_BYTES, "chunk size");
    std::mt19937 rng(12345);
    const uint32_t edge[] = {0, 1, 2, 3, 4, 5, 62, 63, 64, 65, 66, 67, 126, 127, 128, 129, 130, 131, 1919, 1920, 1921, 1983, 1984,
                             1985, 1999, 2000, 2001, 2002, 1000000};
    const int periods[] = {65, 128, 129, 2000, 64, 1, 191, 193, 1999};
    size_t total = 0;
    for (int maxperiod : periods)
        for (int delta : {7, 0, -1})
            for (int rep = 0; rep < 6; rep++) {
                std::vector<uint32_t> lengths;
                const size_t n = rep == 0 ? 0 : 1 + rng() % 200;
                for (size_t i = 0; i < n; i++) {
                    const uint32_t r = rng() % 4;
                    lengths.push_back(r == 0 ? edge[rng() % (sizeof edge / sizeof edge[0])] : r == 1 ? rng() % 200 : r == 2 ? rng() % 2300 : rng() % 50000);
                }
                if (rep == 1) lengths.assign(edge, edge + sizeof edge / sizeof edge[0]);
                total += check_list(lengths, maxperiod, delta);
            }
    // spot values: a 300-base slice at maxperiod 2000 takes the blocks 0 .. 4 (smallest diagonals 1, 63, 127, 191, 255; block 5: 319)
    CHECK(host_plan::tandem_jobs({300}, 2000, 7).size() == 5);
    CHECK(host_plan::tandem_jobs({63}, 2000, 7).size() == 1 && host_plan::tandem_jobs({64}, 2000, 7).size() == 2);
    CHECK(host_plan::tandem_jobs({65}, 2000, 0).size() == 1 && host_plan::tandem_jobs({66}, 2000, 0).size() == 2);
    CHECK(host_plan::tandem_jobs({1000000}, 2000, 7).size() == 32 && host_plan::tandem_jobs({1000000}, 65, 7).size() == 2);
    CHECK(host_plan::tandem_jobs({0, 1}, 2000, 7).empty());
    // more jobs than one chunk holds: 300 000 slices x 32 blocks (too many for the restatement above: counted, and the order checked)
    {
        std::vector<uint32_t> lengths(300000, 2100);
        lengths[7] = 0;
        lengths[299999] = 5000;
        const std::vector<host_plan::TandemJob> jobs = host_plan::tandem_jobs(lengths, 2000, 7);
        CHECK(jobs.size() == 299999ull * 32 && jobs.size() > host_plan::TANDEM_CHUNK_JOBS);
        CHECK(jobs[0].slice == 299999 && jobs[31].block == 31 && jobs[32].slice == 0 && jobs.back().slice == 299998);
        check_chunks(jobs.size());
        total += jobs.size();
    }
    printf("tandem_plan: ok %zu jobs\n", total);
    return 0;
}
