// The host side of mimeo_link_regions (mimeo_amd/csrc/link_regions_host.h: validate, chrom_offsets, plan_jobs) under the CPU
// sanitizers: a valid call is accepted, every check the header promises refuses its own kind of bad input with the item, the
// region or the record and block named, the per-chromosome offsets cut the region table, and the jobs are the items that pass
// rule A, in the slice of their alignment.  Built and run by tests/test_host_families.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/link_regions_host.h"

using namespace mimeo::link_regions_host;
using mimeo::path_stats_host::plan_slices;
using mimeo::window_stats_host::bucket_items;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "link_regions_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{1000, 5000, 300};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_interval> regions;
    std::vector<uint32_t> chrom_of_scaf{2, 0, 1};   // FASTA order is not the sorted order: scaffold 1 (5000 bases) is chromosome 0
    bool identity = false;
    std::vector<mimeo_window_item> items;
    uint32_t pct = 80;
    std::vector<uint32_t> chrom;
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    bool ok(std::string *msg) {
        return validate(len_t, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), regions.data(), regions.size(),
                        identity ? nullptr : chrom_of_scaf.data(), items.data(), items.size(), pct, chrom, msg);
    }
};

static Call valid() {
    Call c;
    // chromosome 0 = scaffold 1 (5000), chromosome 1 = scaffold 2 (300), chromosome 2 = scaffold 0 (1000)
    c.regions = {{0, 100, 200}, {0, 200, 260}, {0, 4900, 5000}, {1, 0, 300}, {2, 10, 110}, {2, 900, 1000}};
    c.add(0, 1, 0, {{10, 100, 40}, {52, 142, 58}});   // scaffold 0 [10, 110) onto scaffold 1 [100, 200), a deletion of 2
    c.add(1, 0, 1, {{4900, 0, 100}});                 // the last bases of scaffold 1 onto the minus strand of scaffold 0
    c.add(2, 2, 0, {{0, 0, 300}});                    // a whole scaffold
    c.add(1, 1, 0, {});                               // no blocks: links nothing
    c.items = {{0, 4, 10, 110}, {1, 2, 4900, 5000}, {2, 3, 0, 300}, {3, 0, 100, 200},
               {0, 4, 30, 109},     // 79 of 100: fails rule A, legal
               {0, 4, 50, 50},      // an empty window is legal
               {1, 2, 4920, 5000}}; // 80 of 100: passes
    return c;
}

static void refused(Call c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.rfind("mimeo_link_regions:", 0) != 0 || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "link_regions_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    CHECK((c.chrom == std::vector<uint32_t>{2, 0, 1}));
    // nitems == 0, and nothing at all
    CHECK(validate(c.len_t, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), c.regions.data(), c.regions.size(), c.chrom_of_scaf.data(), nullptr, 0, 80, c.chrom, &msg));
    CHECK(validate(c.len_t, nullptr, 0, nullptr, nullptr, 0, nullptr, 0, nullptr, nullptr, 0, 1, c.chrom, &msg));
    CHECK((c.chrom == std::vector<uint32_t>{0, 1, 2}));   // NULL: identity
    // pct 1 and 100 are in range, 0 and 101 are not
    c = valid(); c.pct = 1; CHECK(c.ok(&msg));
    c = valid(); c.pct = 100; CHECK(c.ok(&msg));
    c = valid(); c.pct = 0; REFUSED(c, "min_cover_pct 0", "not in 1 .. 100");
    c = valid(); c.pct = 101; REFUSED(c, "min_cover_pct 101", "not in 1 .. 100");
    // everything mimeo_path_stats checks, under this entry point's name
    c = valid(); c.blk[1].len = 0; REFUSED(c, "record 0, block 1 ", "len is 0");
    c = valid(); c.blk[1].t = 49; REFUSED(c, "record 0, block 1 ", "overlaps the block before it");
    c = valid(); c.blk[2].len = 101; REFUSED(c, "record 1, block 2 ", "t + len is beyond the target scaffold");
    c = valid(); c.blk[2].q = 901; REFUSED(c, "record 1, block 2 ", "q + len is beyond the query scaffold");   // a self job: the query's length is scaffold 0's
    c = valid(); c.aln[2].tid = 3; REFUSED(c, "record 2:", "tid");
    c = valid(); c.aln[2].qid = 3; REFUSED(c, "record 2:", "qid");
    c = valid(); c.aln[1].qstrand = 2; REFUSED(c, "record 1:", "qstrand");
    c = valid(); c.first[0] = 1; REFUSED(c, "record 0:", "path_first[0] is not 0");
    c = valid(); c.first[2] = 1; REFUSED(c, "record 1:", "path_first decreases");
    c = valid(); c.first.back() += 1; REFUSED(c, "record 3:", "path_first[n] is not nblocks");
    // chrom_of_scaf: out of range, and a chromosome twice
    c = valid(); c.chrom_of_scaf[1] = 3; REFUSED(c, "chrom_of_scaf[1] = 3", "not below the number of scaffolds");
    c = valid(); c.chrom_of_scaf[2] = 2; REFUSED(c, "chrom_of_scaf[2] = 2", "also the chromosome of scaffold 0");
    // regions: sorted, disjoint, inside their scaffolds
    c = valid(); c.regions[3].chrom = 3; REFUSED(c, "region 3 (chrom 3,", "chrom is not a chromosome");
    c = valid(); std::swap(c.regions[0], c.regions[1]); REFUSED(c, "region 1 (chrom 0, [100, 200))", "in front of the region before it");
    c = valid(); c.regions[4].chrom = 0; REFUSED(c, "region 4 ", "in front of the region before it");   // chrom goes down
    c = valid(); c.regions[1].start = 199; REFUSED(c, "region 1 (chrom 0, [199, 260))", "overlaps it");
    c = valid(); c.regions[1].end = 200; REFUSED(c, "region 1 ", "start is not below end");
    c = valid(); c.regions[2].end = 5001; REFUSED(c, "region 2 (chrom 0, [4900, 5001))", "end is beyond its scaffold");
    c = valid(); c.regions[3].end = 301; REFUSED(c, "region 3 ", "end is beyond its scaffold");      // chromosome 1 is scaffold 2: 300 bases, not 5000
    c = valid(); c.identity = true; REFUSED(c, "region 2 (chrom 0, [4900, 5000))", "end is beyond its scaffold");   // under the identity chromosome 0 has 1000 bases
    // items
    c = valid(); c.items[2].aln = 4; REFUSED(c, "item 2 (aln 4,", "aln is not a record");
    c = valid(); c.items[6].aln = 0xFFFFFFFFu; REFUSED(c, "item 6 (aln 4294967295,", "aln is not a record");
    c = valid(); c.items[1].group = 6; REFUSED(c, "item 1 (aln 1, region 6,", "region is not below nreg");
    c = valid(); c.items[0].group = 0; c.items[0].w0 = 100; c.items[0].w1 = 200;   // region 0 has these coordinates, on another scaffold
    REFUSED(c, "item 0 (aln 0, region 0,", "does not lie on the record's target scaffold");
    c = valid(); c.items[5].w0 = 51; REFUSED(c, "item 5 (aln 0, region 4, window [51, 50))", "w0 is beyond w1");
    c = valid(); c.items[0].w0 = 9; REFUSED(c, "item 0 ", "the window does not lie inside the region");
    c = valid(); c.items[0].w1 = 111; REFUSED(c, "item 0 ", "the window does not lie inside the region");
    c = valid(); c.items[3].w0 = 0xFFFFFFFEu; c.items[3].w1 = 0xFFFFFFFFu; REFUSED(c, "item 3 ", "the window does not lie inside the region");
    // the first bad item is the one named; a bad region is refused before any item is looked at, a bad path before any region
    c = valid(); c.items[4].group = 9; c.items[5].aln = 77; REFUSED(c, "item 4 ", "region is not below nreg");
    c = valid(); c.regions[5].end = 2000; c.items[0].aln = 77; REFUSED(c, "region 5 ", "end is beyond its scaffold");
    c = valid(); c.blk[0].len = 0; c.regions[5].end = 2000; REFUSED(c, "record 0, block 0 ", "len is 0");
    // items without an array, regions without an array
    c = valid();
    CHECK(!validate(c.len_t, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), c.regions.data(), c.regions.size(), nullptr, nullptr, 3, 80, c.chrom, &msg));
    c = valid();
    CHECK(!validate(c.len_t, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), nullptr, 3, c.chrom_of_scaf.data(), c.items.data(), 1, 80, c.chrom, &msg) &&
          msg.find("null argument") != std::string::npos);

    // the per-chromosome offsets
    c = valid();
    CHECK(c.ok(&msg));
    CHECK((chrom_offsets(c.regions.data(), c.regions.size(), 3) == std::vector<uint32_t>{0, 3, 4, 6}));
    CHECK((chrom_offsets(c.regions.data(), 3, 3) == std::vector<uint32_t>{0, 3, 3, 3}));
    CHECK((chrom_offsets(nullptr, 0, 2) == std::vector<uint32_t>{0, 0, 0}));
    // rule A at its boundary, in 64 bits
    CHECK(covers(0, 80, 0, 100, 80) && !covers(0, 79, 0, 100, 80) && covers(5, 6, 0, 100, 1) && !covers(5, 5, 0, 100, 1));
    CHECK(covers(0, 100, 0, 100, 100) && !covers(0, 99, 0, 100, 100));
    CHECK(covers(0, 0xFFFFFFFFull, 0, 0xFFFFFFFFull, 100) && !covers(1, 0xFFFFFFFFull, 0, 0xFFFFFFFFull, 100));   // 100 * 2^32 does not fit 32 bits
    // the jobs of the valid call, one alignment per slice: the items that pass rule A, in the slice of their alignment, in the
    // order of the call; the alignment without blocks makes none
    {
        const auto slices = plan_slices(c.first.data(), c.aln.size(), 1, 1u << 24);
        CHECK(slices.size() == 4);
        std::vector<uint64_t> order, start;
        bucket_items(slices, c.items.data(), c.items.size(), order, start);
        CHECK((order == std::vector<uint64_t>{0, 4, 5, 1, 6, 2, 3}));
        std::vector<Job> jobs;
        plan_jobs(c.first.data(), 0, c.regions.data(), c.items.data(), order.data(), start[0], start[1], 80, jobs);
        CHECK(jobs.size() == 1 && jobs[0].aln == 0 && jobs[0].region == 4 && jobs[0].w0 == 10 && jobs[0].w1 == 110);
        plan_jobs(c.first.data(), 0, c.regions.data(), c.items.data(), order.data(), start[0], start[1], 79, jobs);
        CHECK(jobs.size() == 2 && jobs[1].w0 == 30 && jobs[1].w1 == 109);
        plan_jobs(c.first.data(), 1, c.regions.data(), c.items.data(), order.data(), start[1], start[2], 80, jobs);
        CHECK(jobs.size() == 2 && jobs[0].aln == 0 && jobs[0].region == 2 && jobs[1].w0 == 4920);
        plan_jobs(c.first.data(), 2, c.regions.data(), c.items.data(), order.data(), start[2], start[3], 100, jobs);
        CHECK(jobs.size() == 1 && jobs[0].aln == 0 && jobs[0].region == 3);
        plan_jobs(c.first.data(), 3, c.regions.data(), c.items.data(), order.data(), start[3], start[4], 1, jobs);
        CHECK(jobs.empty());
    }
    // random calls over random slices: every job belongs to an item that passes rule A, none is lost, windows are never empty
    std::mt19937 rng(12);
    size_t total_jobs = 0, dropped = 0;
    for (int rep = 0; rep < 200; rep++) {
        const uint64_t n = 1 + rng() % 30;
        std::vector<uint64_t> first{0};
        std::vector<mimeo_path_block> blk;
        for (uint64_t i = 0; i < n; i++) {
            const uint32_t nb = rng() % 4;
            uint32_t t = rng() % 500;
            for (uint32_t k = 0; k < nb; k++) { const uint32_t len = 1 + rng() % 300; blk.push_back(mimeo_path_block{t, t, len}); t += len + rng() % 3; }
            first.push_back(blk.size());
        }
        std::vector<mimeo_interval> regions;
        for (uint32_t s = rng() % 50; regions.size() < 20; s += rng() % 40) { const uint32_t len = 1 + rng() % 200; regions.push_back(mimeo_interval{0, s, s + len}); s += len; }
        std::vector<mimeo_window_item> items(rng() % 60);
        for (auto &it : items) {
            it.aln = rng() % n;
            it.group = rng() % regions.size();
            const mimeo_interval &r = regions[it.group];
            it.w0 = r.start + rng() % (r.end - r.start + 1);
            it.w1 = it.w0 + rng() % (r.end - it.w0 + 1);
            if (rng() % 3 == 0) { it.w0 = r.start; it.w1 = r.end; }
        }
        const uint32_t pct = 1 + rng() % 100;
        const auto slices = plan_slices(first.data(), n, 1 + rng() % 8, 1 + rng() % 12);
        std::vector<uint64_t> order, start;
        bucket_items(slices, items.data(), items.size(), order, start);
        for (size_t s = 0; s < slices.size(); s++) {
            std::vector<Job> jobs;
            plan_jobs(first.data(), slices[s].first, regions.data(), items.data(), order.data(), start[s], start[s + 1], pct, jobs);
            size_t j = 0;
            for (uint64_t k = start[s]; k < start[s + 1]; k++) {
                const mimeo_window_item &it = items[order[k]];
                const mimeo_interval &r = regions[it.group];
                const bool pass = first[it.aln] < first[it.aln + 1] && 100ull * (it.w1 - it.w0) >= (uint64_t)pct * (r.end - r.start);
                if (!pass) { dropped++; continue; }
                CHECK(j < jobs.size());
                CHECK(jobs[j].aln == it.aln - slices[s].first && jobs[j].region == it.group && jobs[j].w0 == it.w0 && jobs[j].w1 == it.w1 && jobs[j].w0 < jobs[j].w1);
                j++;
            }
            CHECK(j == jobs.size());
            total_jobs += j;
        }
    }
    CHECK(total_jobs > 100 && dropped > 100);
    printf("link_regions_check: ok %zu jobs, %zu items without a job\n", total_jobs, dropped);
    return 0;
}
