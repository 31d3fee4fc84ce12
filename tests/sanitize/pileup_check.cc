// The host side of mimeo_path_pileup (mimeo_amd/csrc/pileup_host.h: validate, plan_tiles, plan_batch, bucket_tiles, plan_jobs)
// under the CPU sanitizers: a valid call is accepted, every kind of bad window and bad item is refused with its name (and a bad
// path with its record, before any window is looked at), and the jobs of a call cover every (item, column) exactly once, whatever
// the tile, the batch size, the entries per run and the items per job.  Built and run by tests/test_host_pileup.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "../../mimeo_amd/csrc/pileup_host.h"

using namespace mimeo::pileup_host;
using mimeo::path_stats_host::plan_slices;
using mimeo::window_stats_host::bucket_items;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "pileup_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{10000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_pileup_window> win;
    std::vector<mimeo_window_item> items;
    uint64_t max_window_items = MAX_WINDOW_ITEMS;
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    bool ok(std::string *msg) const {
        return validate(len_t, len_q, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), win.data(), win.size(), items.data(), items.size(), msg,
                        max_window_items);
    }
};

static Call valid() {
    Call c;
    c.add(0, 0, 0, {{100, 50, 20}, {120, 73, 15}, {140, 88, 20}});   // an insertion, then a deletion: [100, 160) on scaffold 0
    c.add(1, 0, 1, {{0, 0, 1}});                                       // starts at base 0 of scaffold 1 (5000 bases)
    c.add(0, 0, 1, {{9990, 790, 10}});                                 // ends on the last base of both scaffolds
    c.add(1, 1, 0, {});                                                // no blocks: counts nothing
    c.win = {{0, 50, 300}, {1, 0, 5000}, {0, 9000, 10000}, {0, 50, 300} /* a window twice */, {1, 70, 70} /* empty */, {0, 0, 10000}};
    c.items = {{0, 0, 100, 160}, {0, 3, 50, 300}, {1, 1, 0, 5000}, {2, 2, 9995, 10000}, {3, 1, 10, 20}, {0, 0, 130, 130} /* an empty item */,
               {3, 4, 70, 70}, {0, 5, 0, 10000}, {2, 5, 0, 10000}, {0, 0, 200, 300} /* misses its alignment */};
    return c;
}

static void refused(const Call &c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find("mimeo_path_pileup: ") != 0 || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "pileup_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

// Every job of the call, for the given layout: per (item, target base) the number of jobs that hold it.  Checked against the
// clipped windows of the items.
static void cover(const Call &c, uint32_t tile, uint64_t batch_columns, uint64_t max_rec, uint64_t max_blk, uint64_t run_entries, uint64_t job_items,
                  size_t *njobs, size_t *nbatches, size_t *max_tile_jobs) {
    const Tiles t = plan_tiles(c.win.data(), c.win.size(), tile);
    CHECK(t.col_first.size() == c.win.size() + 1 && t.tile_first.size() == c.win.size() + 1);
    for (size_t g = 0; g < c.win.size(); g++) {
        const uint64_t len = c.win[g].end - c.win[g].start;
        CHECK(t.col_first[g + 1] - t.col_first[g] == len && t.tile_first[g + 1] - t.tile_first[g] == (len + tile - 1) / tile);
    }
    const auto slices = plan_slices(c.first.data(), c.aln.size(), max_rec, max_blk);
    std::vector<uint64_t> order, start;
    bucket_items(slices, c.items.data(), c.items.size(), order, start);
    std::map<std::pair<uint64_t, uint64_t>, int> seen;   // (item's alignment and window, call column) -> times; items that repeat share a key
    std::vector<char> col_in_batch(t.ncols(), 0);
    uint64_t win = 0;
    Batch b;
    for (uint64_t tile0 = 0; tile0 < t.ntiles(); tile0 = b.tile1) {
        while (t.tile_first[win + 1] <= tile0) win++;
        b = plan_batch(t, c.win.data(), c.win.size(), win, tile0, batch_columns);
        (*nbatches)++;
        CHECK(b.tile1 > b.tile0 && b.desc.size() == b.tile1 - b.tile0 && b.ncols <= std::max<uint64_t>(batch_columns, tile));
        CHECK(b.desc.size() == 1 || b.ncols <= batch_columns);
        uint64_t at = 0;
        for (const TileDesc &d : b.desc) {   // consecutive tiles are consecutive columns
            CHECK(d.col0 == at && d.ncols >= 1 && d.ncols <= tile);
            at += d.ncols;
        }
        CHECK(at == b.ncols && b.col0 + b.ncols <= t.ncols());
        for (uint64_t k = 0; k < b.ncols; k++) { CHECK(!col_in_batch[b.col0 + k]); col_in_batch[b.col0 + k] = 1; }
        std::vector<size_t> tile_jobs(b.desc.size(), 0);
        for (size_t s = 0; s < slices.size(); s++) {
            for (uint64_t i0 = start[s]; i0 < start[s + 1];) {
                TileItems ti;
                const uint64_t i1 = bucket_tiles(t, b, c.first.data(), c.blk.data(), slices[s].first, c.win.data(), c.items.data(), order.data(), i0, start[s + 1],
                                                 run_entries, ti);
                CHECK(i1 > i0 && i1 <= start[s + 1] && ti.start.size() == b.desc.size() + 1 && ti.start.back() == ti.entries.size());
                std::vector<Job> jobs;
                plan_jobs(b, ti, job_items, jobs);
                const uint64_t per = job_items >= 1 && job_items <= 0xFFFF ? job_items : JOB_ITEMS;
                uint64_t entries_in_jobs = 0;
                for (const Job &j : jobs) {
                    CHECK(j.nitems >= 1 && j.nitems <= per && (uint64_t)j.item0 + j.nitems <= ti.entries.size());
                    // the job's tile, found again from its first column
                    size_t k = 0;
                    while (k < b.desc.size() && b.desc[k].col0 != j.col0) k++;
                    CHECK(k < b.desc.size() && b.desc[k].t0 == j.t0 && b.desc[k].ncols == j.ncols);
                    CHECK(j.item0 >= ti.start[k] && (uint64_t)j.item0 + j.nitems <= ti.start[k + 1]);
                    tile_jobs[k]++;
                    entries_in_jobs += j.nitems;
                    for (uint32_t e = j.item0; e < j.item0 + j.nitems; e++) {
                        const Entry &en = ti.entries[e];
                        CHECK(en.w0 < en.w1 && en.w0 >= j.t0 && en.w1 <= j.t0 + j.ncols);
                        const uint64_t a = slices[s].first + en.aln;
                        CHECK(a < slices[s].second && c.first[a] < c.first[a + 1]);
                        CHECK(en.w0 >= c.blk[c.first[a]].t && en.w1 <= c.blk[c.first[a + 1] - 1].t + c.blk[c.first[a + 1] - 1].len);
                        CHECK(c.aln[a].tid == b.desc[k].tid);
                        for (uint32_t x = en.w0; x < en.w1; x++) seen[{a << 32 | (b.col0 + j.col0 + (x - j.t0)), 0}]++;
                    }
                }
                CHECK(entries_in_jobs == ti.entries.size());
                *njobs += jobs.size();
                i0 = i1;
            }
        }
        for (size_t k : tile_jobs) *max_tile_jobs = std::max(*max_tile_jobs, k);
    }
    for (char x : col_in_batch) CHECK(x);
    // what the items ask for, restated: per item the window clipped to the alignment, column by column
    std::map<std::pair<uint64_t, uint64_t>, int> want;
    for (const mimeo_window_item &it : c.items) {
        const uint64_t b0 = c.first[it.aln], b1 = c.first[it.aln + 1];
        if (b0 == b1) continue;
        const uint64_t lo = std::max<uint64_t>(it.w0, c.blk[b0].t), hi = std::min<uint64_t>(it.w1, (uint64_t)c.blk[b1 - 1].t + c.blk[b1 - 1].len);
        for (uint64_t x = lo; x < hi; x++) want[{(uint64_t)it.aln << 32 | (t.col_first[it.group] + (x - c.win[it.group].start)), 0}]++;
    }
    CHECK(seen == want);
}

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    // no items, no records; no windows
    CHECK(validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, c.win.data(), c.win.size(), nullptr, 0, &msg));
    CHECK(validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), nullptr, 0, nullptr, 0, &msg));
    // windows or items without an array
    CHECK(!validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, nullptr, 2, nullptr, 0, &msg) && msg == "mimeo_path_pileup: null argument");
    CHECK(!validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), c.win.data(), c.win.size(), nullptr, 3, &msg) &&
          msg == "mimeo_path_pileup: null argument");
    // windows: tid inside T, start <= end, end <= the scaffold's length
    c = valid(); c.win[2].tid = 2;
    REFUSED(c, "window 2 (tid 2, [9000, 10000))", "tid is not a scaffold");
    c = valid(); c.win[4].start = 71;
    REFUSED(c, "window 4 (tid 1, [71, 70))", "start is beyond end");
    c = valid(); c.win[1].end = 5001;
    REFUSED(c, "window 1 (tid 1, [0, 5001))", "end is beyond its scaffold");
    c = valid(); c.win[0].start = 0xFFFFFFF0u; c.win[0].end = 0xFFFFFFFFu;
    REFUSED(c, "window 0 ", "end is beyond its scaffold");
    // items: aln < n, group < nwin, the same scaffold, start <= w0 <= w1 <= end
    c = valid(); c.items[2].aln = 4;
    REFUSED(c, "item 2 (aln 4, window 1, [0, 5000))", "aln is not a record");
    c = valid(); c.items[3].group = 6;
    REFUSED(c, "item 3 (aln 2, window 6,", "window is not below nwin");
    c = valid(); c.items[0].group = 1;   // record 0 lies on scaffold 0, window 1 on scaffold 1
    REFUSED(c, "item 0 (aln 0, window 1,", "does not lie on the record's target scaffold");
    c = valid(); c.items[5].w0 = 131;
    REFUSED(c, "item 5 (aln 0, window 0, [131, 130))", "w0 is beyond w1");
    c = valid(); c.items[0].w0 = 49;
    REFUSED(c, "item 0 ", "does not lie inside the window");
    c = valid(); c.items[1].w1 = 301;
    REFUSED(c, "item 1 ", "does not lie inside the window");
    c = valid(); c.items[6].w0 = 69; c.items[6].w1 = 70;   // nothing lies inside an empty window but the empty item at its place
    REFUSED(c, "item 6 ", "does not lie inside the window");
    // the first bad item is the one named; a bad window comes before every item, a bad path before every window
    c = valid(); c.items[6].group = 9; c.items[7].w0 = 20000;
    REFUSED(c, "item 6 ", "window is not below nwin");
    c = valid(); c.items[0].aln = 77; c.win[5].end = 10001;
    REFUSED(c, "window 5 ", "end is beyond its scaffold");
    c = valid(); c.blk[1].len = 0; c.win[0].tid = 9;
    REFUSED(c, "record 0, block 1 ", "len is 0");
    c = valid(); c.first.back() += 1;
    REFUSED(c, "record 3:", "path_first[n] is not nblocks");
    // more items on one window than its counters hold: the limit is a parameter, so that it can be reached here
    c = valid(); c.max_window_items = 2;   // items 0, 5 and 9 name window 0
    REFUSED(c, "window 0 (tid 0, [50, 300))", "more than 2 items name it (item 9)");
    c = valid(); c.max_window_items = 3;
    CHECK(c.ok(&msg));

    // the tiles and the jobs, by hand, TILE = 1024: a window of 2500 columns is tiles of 1024, 1024 and 452
    {
        Call h;
        h.add(0, 0, 0, {{1000, 0, 300}, {1400, 300, 400}});   // [1000, 1800) with a deletion of 100
        h.add(0, 0, 0, {{100, 0, 700}});                       // [100, 800)
        h.win = {{0, 100, 2600}, {0, 0, 0}, {0, 1124, 1125}};
        // an item that spans three tiles ([100, 1124), [1124, 2148), [2148, 2600)); one that ends exactly on a tile's edge; one
        // that starts on it; the one-column window
        h.items = {{0, 0, 100, 2600}, {1, 0, 100, 1124}, {0, 0, 1124, 1500}, {0, 2, 1124, 1125}};
        CHECK(h.ok(&msg));
        const Tiles t = plan_tiles(h.win.data(), h.win.size());
        CHECK(t.tile == 1024 && t.ncols() == 2501 && t.ntiles() == 4);
        CHECK((t.col_first == std::vector<uint64_t>{0, 2500, 2500, 2501}) && (t.tile_first == std::vector<uint64_t>{0, 3, 3, 4}));
        const Batch b = plan_batch(t, h.win.data(), h.win.size(), 0, 0, 1ull << 22);
        CHECK(b.tile0 == 0 && b.tile1 == 4 && b.win0 == 0 && b.win1 == 3 && b.col0 == 0 && b.ncols == 2501 && b.desc.size() == 4);
        CHECK(b.desc[0].t0 == 100 && b.desc[0].ncols == 1024 && b.desc[1].t0 == 1124 && b.desc[1].col0 == 1024 && b.desc[2].t0 == 2148 &&
              b.desc[2].ncols == 452 && b.desc[2].col0 == 2048 && b.desc[3].t0 == 1124 && b.desc[3].ncols == 1 && b.desc[3].col0 == 2500);
        const std::vector<uint64_t> order{0, 1, 2, 3};
        TileItems ti;
        CHECK(bucket_tiles(t, b, h.first.data(), h.blk.data(), 0, h.win.data(), h.items.data(), order.data(), 0, 4, 1ull << 22, ti) == 4);
        // item 0 is clipped to its alignment [1000, 1800): tiles 0 and 1, not 2; item 1 to [100, 800): tile 0 only
        CHECK((ti.start == std::vector<uint64_t>{0, 2, 4, 4, 5}));
        auto is = [&](size_t e, uint32_t a, uint32_t w0, uint32_t w1) { return ti.entries[e].aln == a && ti.entries[e].w0 == w0 && ti.entries[e].w1 == w1; };
        CHECK(is(0, 0, 1000, 1124) && is(1, 1, 100, 800) && is(2, 0, 1124, 1800) && is(3, 0, 1124, 1500) && is(4, 0, 1124, 1125));
        std::vector<Job> jobs;
        plan_jobs(b, ti, 1, jobs);
        CHECK(jobs.size() == 5 && jobs[1].item0 == 1 && jobs[1].nitems == 1 && jobs[1].t0 == 100 && jobs[4].col0 == 2500 && jobs[4].ncols == 1);
        plan_jobs(b, ti, 0, jobs);   // 0: the default
        CHECK(jobs.size() == 3 && jobs[0].nitems == 2 && jobs[1].nitems == 2 && jobs[1].t0 == 1124 && jobs[2].nitems == 1);
        // a batch of at most 1476 columns from tile 1 on: tiles 1 and 2 (1024 + 452) fill it, the one-column tile 3 is the next batch's
        const Batch b1 = plan_batch(t, h.win.data(), h.win.size(), 0, 1, 1476);
        CHECK(b1.tile0 == 1 && b1.tile1 == 3 && b1.col0 == 1024 && b1.ncols == 1476 && b1.win0 == 0 && b1.win1 == 1);
        CHECK(bucket_tiles(t, b1, h.first.data(), h.blk.data(), 0, h.win.data(), h.items.data(), order.data(), 0, 4, 1ull << 22, ti) == 4);
        CHECK((ti.start == std::vector<uint64_t>{0, 2, 2}) && is(0, 0, 1124, 1800) && is(1, 0, 1124, 1500));
        // a run of at most one entry at a time: every item that makes entries goes alone, whatever it makes
        CHECK(bucket_tiles(t, b, h.first.data(), h.blk.data(), 0, h.win.data(), h.items.data(), order.data(), 0, 4, 1, ti) == 1 && ti.entries.size() == 2);
        CHECK(bucket_tiles(t, b, h.first.data(), h.blk.data(), 0, h.win.data(), h.items.data(), order.data(), 1, 4, 1, ti) == 2 && ti.entries.size() == 1);
    }

    // every (item, column) in exactly one job, under every layout: the valid call (a window that is no multiple of the tile, a
    // window twice, an empty one, items over the whole scaffold), and a tile with more items than a job takes
    size_t njobs = 0, nbatches = 0, max_tile_jobs = 0;
    c = valid();
    for (int k = 0; k < 70; k++) c.items.push_back({0, 0, 100u + k % 7, 160u - k % 5});   // 70 more items on one tile of window 0
    for (const uint32_t tile : {1024u, 64u, 100u})
        for (const uint64_t batch : {1ull << 22, 1500ull, 1ull})
            for (const uint64_t run : {1ull << 22, 3ull})
                for (const uint64_t per : {64ull, 7ull, 1ull})
                    cover(c, tile, batch, batch == 1 ? 1 : 1u << 22, run == 3 ? 1 : 1u << 24, run, per, &njobs, &nbatches, &max_tile_jobs);
    CHECK(max_tile_jobs >= 71 && nbatches > 100);   // items 0 and the 70: a job each where a job takes one
    // random calls
    std::mt19937 rng(13);
    for (int rep = 0; rep < 60; rep++) {
        Call r;
        r.len_t = {20000, 3000};
        r.len_q = {1u << 30, 1u << 30};
        const uint32_t n = 1 + rng() % 12;
        for (uint32_t i = 0; i < n; i++) {
            const uint32_t tid = rng() % 2, nb = rng() % 6, L = (uint32_t)r.len_t[tid];
            std::vector<mimeo_path_block> b;
            uint32_t t = rng() % (L / 2), q = rng() % 1000;
            for (uint32_t k = 0; k < nb; k++) {
                const uint32_t len = 1 + rng() % 900;
                if (t + len > L) break;
                b.push_back({t, q, len});
                t += len + rng() % 40; q += len + rng() % 3;
            }
            r.add(tid, rng() % 2, rng() % 2, b);
        }
        const uint32_t nwin = 1 + rng() % 6;
        for (uint32_t g = 0; g < nwin; g++) {
            const uint32_t tid = rng() % 2, L = (uint32_t)r.len_t[tid], s = rng() % L, e = s + rng() % std::min<uint32_t>(L - s + 1, 4000);
            r.win.push_back({tid, s, e});
        }
        const uint32_t nitems = rng() % 40;
        for (uint32_t i = 0; i < nitems; i++) {
            const uint32_t a = rng() % n;
            std::vector<uint32_t> on;   // the windows of the record's scaffold
            for (uint32_t g = 0; g < nwin; g++) if (r.win[g].tid == r.aln[a].tid) on.push_back(g);
            if (on.empty()) continue;
            const uint32_t g = on[rng() % on.size()], len = r.win[g].end - r.win[g].start;
            const uint32_t w0 = r.win[g].start + rng() % (len + 1), w1 = w0 + rng() % (r.win[g].end - w0 + 1);
            r.items.push_back({a, g, w0, w1});
        }
        CHECK(r.ok(&msg));
        const uint32_t tiles[] = {1024, 64, 257};
        const uint64_t batches[] = {1ull << 22, 1500, 300};
        cover(r, tiles[rep % 3], batches[(rep / 3) % 3], 1 + rng() % 5, 1 + rng() % 9, rep % 2 ? 1ull << 22 : 5, 1 + rng() % 9, &njobs, &nbatches, &max_tile_jobs);
    }
    printf("pileup_check: ok %zu jobs, %zu batches, at most %zu jobs on a tile\n", njobs, nbatches, max_tile_jobs);
    return 0;
}
