// The host side of mimeo_path_window_stats (mimeo_amd/csrc/window_stats_host.h: validate, bucket_items, plan_jobs) under the
// CPU sanitizers: valid calls are accepted, every kind of bad item is refused with the item named (and a bad path with its
// record, before any item is looked at), the items land in the slice of their alignment, and the jobs of an item tile its
// clipped window exactly, whatever split_bases.  Built and run by tests/test_host_window_stats.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/window_stats_host.h"

using namespace mimeo::window_stats_host;
using mimeo::path_stats_host::plan_slices;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "window_stats_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{1000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_window_item> items;
    uint64_t ngroups = 4;
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    bool ok(std::string *msg) const {
        return validate(len_t, len_q, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), items.data(), items.size(), ngroups, msg);
    }
};

static Call valid() {
    Call c;
    c.add(0, 0, 0, {{100, 50, 20}, {120, 73, 15}, {140, 88, 20}});   // an insertion, then a deletion: [100, 160) on scaffold 0 (1000 bases)
    c.add(1, 0, 1, {{0, 0, 1}});                                       // starts at base 0 of scaffold 1 (5000 bases)
    c.add(0, 0, 1, {{990, 790, 10}});                                  // ends on the last base of both scaffolds
    c.add(1, 1, 0, {});                                                // no blocks: counts nothing
    c.items = {{0, 0, 100, 160}, {0, 3, 0, 1000}, {1, 1, 0, 5000}, {2, 2, 995, 1000}, {3, 0, 10, 20},
               {0, 1, 130, 130},    // an empty window is legal
               {0, 1, 0, 0}, {2, 1, 1000, 1000},   // ... also at either end of the scaffold
               {0, 2, 500, 700}};   // a window that misses its alignment
    return c;
}

static void refused(const Call &c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "window_stats_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    // nitems == 0: no item is looked at (and with n == 0 nothing at all)
    CHECK(validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), nullptr, 0, 0, &msg));
    CHECK(validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, 0, &msg));
    // items without an array
    CHECK(!validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), nullptr, 3, 4, &msg) &&
          msg.find("null argument") != std::string::npos);
    // aln == n, and far beyond
    c = valid(); c.items[2].aln = 4;
    REFUSED(c, "item 2 (aln 4,", "aln is not a record");
    c = valid(); c.items[8].aln = 0xFFFFFFFFu;
    REFUSED(c, "item 8 (aln 4294967295,", "aln is not a record");
    // an item when the call has no record at all
    CHECK(!validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, c.items.data(), 1, 4, &msg) && msg.find("item 0 ") != std::string::npos &&
          msg.find("aln is not a record") != std::string::npos);
    // group == ngroups; ngroups == 0
    c = valid(); c.items[3].group = 4;
    REFUSED(c, "item 3 (aln 2, group 4,", "group is not below ngroups");
    c = valid(); c.ngroups = 0;
    REFUSED(c, "item 0 ", "group is not below ngroups");
    // w0 > w1
    c = valid(); c.items[5].w0 = 131;
    REFUSED(c, "item 5 (aln 0, group 1, window [131, 130))", "w0 is beyond w1");
    // w1 == Lt + 1, on either scaffold: the length is that of the RECORD's target scaffold
    c = valid(); c.items[1].w1 = 1001;
    REFUSED(c, "item 1 ", "w1 is beyond the target scaffold");
    c = valid(); c.items[2].w1 = 5001;
    REFUSED(c, "item 2 ", "w1 is beyond the target scaffold");
    c = valid(); c.items[0].w1 = 5000;   // fine on scaffold 1, not on scaffold 0
    REFUSED(c, "item 0 ", "w1 is beyond the target scaffold");
    c = valid(); c.items[4].w0 = 0xFFFFFFFEu; c.items[4].w1 = 0xFFFFFFFFu;
    REFUSED(c, "item 4 ", "w1 is beyond the target scaffold");
    // the first bad item is the one named
    c = valid(); c.items[6].group = 9; c.items[7].w0 = 2000;
    REFUSED(c, "item 6 ", "group");
    // a bad path is refused as mimeo_path_stats refuses it, before any item is looked at (item 0 is bad as well here)
    c = valid(); c.blk[1].len = 0; c.items[0].aln = 77;
    REFUSED(c, "record 0, block 1 ", "len is 0");
    c = valid(); c.aln[2].tid = 2;   // no item would be safe to check against this record's scaffold
    REFUSED(c, "record 2:", "tid");
    c = valid(); c.first.back() += 1;
    REFUSED(c, "record 3:", "path_first[n] is not nblocks");

    // the valid call, one alignment per slice: every item in the slice of its alignment, in the order of the call; windows that
    // miss their alignment, empty windows and items of an alignment without blocks make no job
    {
        c = valid();
        const auto slices = plan_slices(c.first.data(), c.aln.size(), 1, 1u << 24);
        CHECK(slices.size() == c.aln.size());
        std::vector<uint64_t> order, start;
        bucket_items(slices, c.items.data(), c.items.size(), order, start);
        CHECK(start.size() == 5 && start[0] == 0 && start[4] == c.items.size());
        const std::vector<uint64_t> want{0, 1, 5, 6, 8, 2, 3, 7, 4};
        CHECK(order == want);
        std::vector<Job> jobs;
        plan_jobs(c.first.data(), c.blk.data(), 0, c.items.data(), order.data(), start[0], start[1], 1u << 20, jobs);
        CHECK(jobs.size() == 2);   // [100, 160) as it is, [0, 1000) clipped to it; the empty and the missing windows make none
        CHECK(jobs[0].aln == 0 && jobs[0].group == 0 && jobs[0].w0 == 100 && jobs[0].w1 == 160);
        CHECK(jobs[1].aln == 0 && jobs[1].group == 3 && jobs[1].w0 == 100 && jobs[1].w1 == 160);
        plan_jobs(c.first.data(), c.blk.data(), 1, c.items.data(), order.data(), start[1], start[2], 1u << 20, jobs);
        CHECK(jobs.size() == 1 && jobs[0].aln == 0 && jobs[0].group == 1 && jobs[0].w0 == 0 && jobs[0].w1 == 1);
        plan_jobs(c.first.data(), c.blk.data(), 2, c.items.data(), order.data(), start[2], start[3], 2, jobs);
        CHECK(jobs.size() == 3 && jobs[0].w0 == 995 && jobs[0].w1 == 997 && jobs[2].w0 == 999 && jobs[2].w1 == 1000 && jobs[2].aln == 0 && jobs[2].group == 2);
        plan_jobs(c.first.data(), c.blk.data(), 3, c.items.data(), order.data(), start[3], start[4], 1u << 20, jobs);
        CHECK(jobs.empty());
    }

    // random calls: the items over random slices, and the jobs of every item against its clipped window, for every split_bases
    std::mt19937 rng(12);
    size_t total_jobs = 0, cut_items = 0, empty_items = 0;
    const uint64_t splits[] = {1, 64, 1000, 1ull << 20, 0};
    for (int rep = 0; rep < 200; rep++) {
        const uint64_t n = 1 + rng() % 30;
        std::vector<uint64_t> first{0};
        std::vector<mimeo_path_block> blk;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t nb = rng() % 6;
            uint32_t t = rng() % 500;
            // rep % 20 == 0: blocks of megabases, so that the default split cuts as well
            for (uint32_t k = 0; k < nb; k++) { const uint32_t len = 1 + rng() % (rep % 20 == 0 ? 3000000 : 700); blk.push_back(mimeo_path_block{t, t, len}); t += len + rng() % 3; }
            first.push_back(blk.size());
        }
        const uint32_t Lt = 20000000;
        std::vector<mimeo_window_item> items(rng() % 60);
        for (auto &it : items) {
            it.aln = rng() % n;
            it.group = rng() % 7;
            const uint64_t b0 = first[it.aln], b1 = first[it.aln + 1];
            const uint32_t lo = b0 < b1 ? blk[b0].t : 0, hi = b0 < b1 ? blk[b1 - 1].t + blk[b1 - 1].len : 100;
            switch (rng() % 5) {
                case 0: it.w0 = 0; it.w1 = Lt; break;                                            // the whole scaffold
                case 1: it.w0 = lo + rng() % (hi - lo + 1); it.w1 = it.w0; break;                // empty
                case 2: it.w0 = hi + rng() % 3; it.w1 = it.w0 + 1 + rng() % 50; break;           // behind the alignment (abutting it or not)
                case 3: it.w1 = lo - std::min<uint32_t>(lo, rng() % 3); it.w0 = it.w1 - std::min<uint32_t>(it.w1, rng() % 50); break;   // in front of it
                default: it.w0 = lo - std::min<uint32_t>(lo, rng() % 5) + rng() % (hi - lo + 1); it.w1 = std::min<uint32_t>(it.w0 + rng() % (hi - lo + 10), Lt); break;
            }
            CHECK(it.w0 <= it.w1 && it.w1 <= Lt);
        }
        const uint64_t max_rec = rep % 3 == 0 ? 1 : 1 + rng() % 8, max_blk = 1 + rng() % 12;
        const auto slices = plan_slices(first.data(), n, max_rec, max_blk);
        std::vector<uint64_t> order, start;
        bucket_items(slices, items.data(), items.size(), order, start);
        CHECK(start.size() == slices.size() + 1 && start[0] == 0 && start.back() == items.size() && order.size() == items.size());
        std::vector<char> seen(items.size(), 0);
        for (size_t s = 0; s < slices.size(); s++) {
            CHECK(start[s] <= start[s + 1]);
            if (rep % 3 == 0) CHECK(slices[s].second - slices[s].first == 1);   // one alignment each
            for (uint64_t k = start[s]; k < start[s + 1]; k++) {
                const uint64_t i = order[k];
                CHECK(i < items.size() && !seen[i]);
                seen[i] = 1;
                CHECK(items[i].aln >= slices[s].first && items[i].aln < slices[s].second);
                CHECK(k == start[s] || order[k - 1] < i);   // the order of the call
            }
            for (const uint64_t split : splits) {
                if (rep % 20 == 0 && split && split < 1000) continue;   // megabase blocks base by base: millions of jobs that show nothing new
                std::vector<Job> jobs;
                plan_jobs(first.data(), blk.data(), slices[s].first, items.data(), order.data(), start[s], start[s + 1], split, jobs);
                size_t j = 0;
                for (uint64_t k = start[s]; k < start[s + 1]; k++) {
                    const mimeo_window_item &it = items[order[k]];
                    const uint64_t b0 = first[it.aln], b1 = first[it.aln + 1];
                    uint64_t w0 = 0, w1 = 0;   // the clipped window, restated
                    if (b0 < b1) {
                        w0 = std::max<uint64_t>(it.w0, blk[b0].t);
                        w1 = std::min<uint64_t>(it.w1, (uint64_t)blk[b1 - 1].t + blk[b1 - 1].len);
                    }
                    if (w0 >= w1) { empty_items++; continue; }   // no job; the next job must belong to a later item (checked there)
                    const size_t j0 = j;
                    uint64_t at = w0;
                    do {
                        CHECK(j < jobs.size());
                        const Job &jb = jobs[j];
                        CHECK(jb.aln == it.aln - slices[s].first && jb.group == it.group && jb.w0 == at && jb.w1 > jb.w0 && jb.w1 <= w1);
                        CHECK(!split || jb.w1 - jb.w0 <= split);
                        CHECK(jb.w1 == w1 || (split && jb.w1 - jb.w0 == split));   // only the last piece is short
                        at = jb.w1;
                        j++;
                    } while (at < w1);
                    if (j - j0 > 1) cut_items++;
                }
                CHECK(j == jobs.size());
                total_jobs += j;
            }
        }
        for (char s : seen) CHECK(s);
    }
    CHECK(cut_items > 100 && empty_items > 100);
    printf("window_stats_check: ok %zu jobs, %zu cut items, %zu items without a job\n", total_jobs, cut_items, empty_items);
    return 0;
}
