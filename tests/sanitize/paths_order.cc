// How a pair's rows and their paths are put plus strand first (mimeo_amd/csrc/host_plan.h: plus_strand_first, what
// mimeo_align_units_paths assembles its three arrays with) under the CPU sanitizers, against a plain restatement.
// Built and run by tests/test_host_paths.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "../../mimeo_amd/csrc/host_plan.h"

using namespace mimeo::host_plan;

struct Row { uint32_t id, qstrand; };
struct Blk { uint32_t t, q, len; };

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "paths_order: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

int main() {
    std::mt19937 rng(7);
    size_t total = 0;
    for (int rep = 0; rep < 400; rep++) {
        const size_t n = rng() % 9;   // also no rows at all
        std::vector<Row> rows;
        std::vector<uint32_t> cnt;
        std::vector<Blk> blk;
        for (size_t i = 0; i < n; i++) {
            rows.push_back(Row{(uint32_t)i, rep % 3 == 0 ? 0u : (uint32_t)(rng() & 1u)});
            cnt.push_back(rng() % 4);   // also alignments without blocks
            for (uint32_t k = 0; k < cnt.back(); k++) blk.push_back(Blk{(uint32_t)i, k, 1u + (uint32_t)(rng() % 50)});
        }
        // restatement: plus rows in their order, then minus rows in theirs, each with the blocks tagged with its id
        std::vector<Row> erows;
        for (uint32_t s = 0; s < 2; s++)
            for (const Row &r : rows) if (r.qstrand == s) erows.push_back(r);
        std::vector<Row> plain = rows;
        plus_strand_first<Row, Blk>(plain, nullptr, nullptr);
        const std::vector<uint32_t> cnt0 = cnt;
        plus_strand_first(rows, &cnt, &blk);
        CHECK(rows.size() == erows.size() && plain.size() == erows.size() && cnt.size() == rows.size());
        size_t at = 0;
        for (size_t i = 0; i < rows.size(); i++) {
            CHECK(rows[i].id == erows[i].id && plain[i].id == erows[i].id);
            CHECK(cnt[i] == cnt0[rows[i].id]);
            for (uint32_t k = 0; k < cnt[i]; k++, at++) CHECK(at < blk.size() && blk[at].t == rows[i].id && blk[at].q == k);
        }
        CHECK(at == blk.size());
        total += at;
    }
    printf("paths_order: ok %zu blocks\n", total);
    return 0;
}
