// The host side of mimeo_path_insertions (mimeo_amd/csrc/insert_host.h: validate, plan_sites, plan_batch, batch_sites,
// bucket_tiles, plan_jobs) under the CPU sanitizers: a valid call is accepted; every kind of bad site is refused with its name,
// and a bad path, window or item under this entry point's name before any site is looked at; the site tiles close where the
// summed columns would pass 1024 and never split a site; and the jobs of a call hold every (item, site) that a brute-force
// restatement asks for exactly once, whatever the tile, the batch size, the entries per run and the entries per job.  Built and
// run by tests/test_host_insertions.py with -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "../../mimeo_amd/csrc/insert_host.h"

using namespace mimeo::insert_host;
using mimeo::path_stats_host::plan_slices;
using mimeo::window_stats_host::bucket_items;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "insert_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{10000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_pileup_window> win;
    std::vector<mimeo_window_item> items;
    std::vector<mimeo_insert_site> sites;
    uint64_t max_window_items = mimeo::pileup_host::MAX_WINDOW_ITEMS;
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    bool ok(std::string *msg) const {
        return validate(len_t, len_q, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), win.data(), win.size(), items.data(), items.size(),
                        sites.data(), sites.size(), msg, max_window_items);
    }
};

static Call valid() {
    Call c;
    c.add(0, 0, 0, {{100, 50, 20}, {120, 73, 15}, {140, 88, 20}});   // 3 inserted bases in front of 120, a deletion [135, 140): [100, 160) on scaffold 0
    c.add(1, 0, 1, {{0, 0, 1}});                                       // starts at base 0 of scaffold 1 (5000 bases)
    c.add(0, 0, 1, {{9990, 790, 10}});                                 // ends on the last base of both scaffolds
    c.add(1, 1, 0, {});                                                // no blocks: counts nothing
    c.win = {{0, 50, 300}, {1, 0, 5000}, {0, 9000, 10000}, {0, 50, 300} /* a window twice */, {1, 70, 70} /* empty */, {0, 0, 10000}};
    c.items = {{0, 0, 100, 160}, {0, 3, 50, 300}, {1, 1, 0, 5000}, {2, 2, 9995, 10000}, {3, 1, 10, 20}, {0, 0, 130, 130} /* an empty item */,
               {3, 4, 70, 70}, {0, 5, 0, 10000}, {2, 5, 0, 10000}, {0, 0, 200, 300} /* misses its alignment */};
    // the first and the last base of a window, a site inside a deletion, the same x in two windows, a window without sites (1, 2, 4)
    c.sites = {{0, 50, 1, 3}, {0, 120, 3, 3}, {0, 137, 1024, 0}, {0, 299, 7, 1}, {3, 120, 5, 2}, {5, 0, 1, 9}, {5, 120, 2, 9}, {5, 9999, 1, 0xFFFFFFFFu}};
    return c;
}

static void refused(const Call &c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find("mimeo_path_insertions: ") != 0 || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "insert_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

// Every job of the call, for the given layout: per (item's alignment and window, site) the number of job entries that hold it,
// against the brute-force restatement: an item holds the sites of its window whose x lies in its window clipped to its alignment.
static void cover(const Call &c, uint32_t tile_cols, uint64_t batch_columns, uint64_t max_rec, uint64_t max_blk, uint64_t run_entries, uint64_t job_items,
                  size_t *njobs, size_t *nbatches, size_t *max_tile_jobs) {
    const Sites p = plan_sites(c.sites.data(), c.sites.size(), c.win.size(), tile_cols);
    CHECK(p.icol_first.size() == c.sites.size() + 1 && p.win_first.size() == c.win.size() + 1 && p.win_first.back() == c.sites.size());
    // the tiles: consecutive, of one window, never over tile_cols, and as long as they can be
    uint64_t s_at = 0;
    for (size_t k = 0; k < p.tiles.size(); k++) {
        const SiteTile &t = p.tiles[k];
        CHECK(t.site0 == s_at && t.nsites >= 1 && t.icol0 == p.icol_first[t.site0] && t.ncols <= tile_cols);
        uint64_t sum = 0;
        for (uint64_t s = t.site0; s < t.site0 + t.nsites; s++) { CHECK(c.sites[s].window == t.window); sum += c.sites[s].ncols; }
        CHECK(sum == t.ncols);
        s_at += t.nsites;
        if (s_at < c.sites.size() && c.sites[s_at].window == t.window) CHECK(t.ncols + c.sites[s_at].ncols > tile_cols);
    }
    CHECK(s_at == c.sites.size());
    const auto slices = plan_slices(c.first.data(), c.aln.size(), max_rec, max_blk);
    std::vector<uint64_t> order, start;
    bucket_items(slices, c.items.data(), c.items.size(), order, start);
    std::map<std::pair<uint64_t, uint64_t>, int> seen, want;   // (alignment, site) -> times; items that repeat share a key
    std::vector<char> site_in_batch(c.sites.size(), 0);
    Batch b;
    std::vector<SiteDesc> desc;
    for (uint64_t tile0 = 0; tile0 < p.tiles.size(); tile0 = b.tile1) {
        b = plan_batch(p, tile0, batch_columns);
        (*nbatches)++;
        CHECK(b.tile1 > b.tile0 && b.site0 == p.tiles[tile0].site0 && b.icol0 == p.tiles[tile0].icol0);
        CHECK(b.tile1 == b.tile0 + 1 || b.ncols <= batch_columns);
        CHECK(b.tile1 == p.tiles.size() || b.ncols + p.tiles[b.tile1].ncols > batch_columns);
        batch_sites(p, b, c.sites.data(), desc);
        CHECK(desc.size() == b.nsites && (desc.empty() || desc[0].off == 0));
        for (uint64_t s = 0; s < b.nsites; s++) {
            CHECK(!site_in_batch[b.site0 + s]);
            site_in_batch[b.site0 + s] = 1;
            CHECK(desc[s].x == c.sites[b.site0 + s].x && desc[s].ncols == c.sites[b.site0 + s].ncols && desc[s].voters == c.sites[b.site0 + s].voters);
            CHECK(desc[s].off + b.icol0 == p.icol_first[b.site0 + s] && (uint64_t)desc[s].off + desc[s].ncols <= b.ncols);
        }
        std::vector<size_t> tile_jobs(b.tile1 - b.tile0, 0);
        for (size_t s = 0; s < slices.size(); s++) {
            for (uint64_t i0 = start[s]; i0 < start[s + 1];) {
                TileItems ti;
                const uint64_t i1 = bucket_tiles(p, b, c.first.data(), c.blk.data(), slices[s].first, c.sites.data(), c.items.data(), order.data(), i0, start[s + 1],
                                                 run_entries, ti);
                CHECK(i1 > i0 && i1 <= start[s + 1] && ti.start.size() == b.tile1 - b.tile0 + 1 && ti.start.back() == ti.entries.size());
                std::vector<Job> jobs;
                plan_jobs(p, b, ti, job_items, jobs);
                const uint64_t per = job_items >= 1 && job_items <= 0xFFFF ? job_items : JOB_ITEMS;
                uint64_t entries_in_jobs = 0;
                for (const Job &j : jobs) {
                    CHECK(j.nitems >= 1 && j.nitems <= per && (uint64_t)j.item0 + j.nitems <= ti.entries.size());
                    size_t k = 0;   // the job's tile, found again from its first site
                    while (k < b.tile1 - b.tile0 && p.tiles[b.tile0 + k].site0 - b.site0 != j.site0) k++;
                    CHECK(k < b.tile1 - b.tile0);
                    const SiteTile &t = p.tiles[b.tile0 + k];
                    CHECK(j.nsites == t.nsites && j.ncols == t.ncols && j.icol0 == t.icol0 - b.icol0 && j.ncols <= tile_cols);
                    CHECK(j.item0 >= ti.start[k] && (uint64_t)j.item0 + j.nitems <= ti.start[k + 1]);
                    tile_jobs[k]++;
                    entries_in_jobs += j.nitems;
                    for (uint32_t e = j.item0; e < j.item0 + j.nitems; e++) {
                        const Entry &en = ti.entries[e];
                        CHECK(en.s0 < en.s1 && en.s0 >= j.site0 && en.s1 <= (uint32_t)j.site0 + j.nsites);
                        const uint64_t a = slices[s].first + en.aln;
                        CHECK(a < slices[s].second && c.first[a] < c.first[a + 1]);
                        for (uint32_t q = en.s0; q < en.s1; q++) {
                            const SiteDesc &d = desc[q];
                            // what the kernel relies on: x inside the alignment, the columns inside the tile's
                            CHECK(d.x >= c.blk[c.first[a]].t && d.x < c.blk[c.first[a + 1] - 1].t + c.blk[c.first[a + 1] - 1].len);
                            CHECK(d.off >= j.icol0 && d.off - j.icol0 + d.ncols <= j.ncols);
                            CHECK(c.aln[a].tid == c.win[c.sites[b.site0 + q].window].tid);
                            seen[{a, b.site0 + q}]++;
                        }
                    }
                }
                CHECK(entries_in_jobs == ti.entries.size());
                *njobs += jobs.size();
                i0 = i1;
            }
        }
        for (size_t k : tile_jobs) *max_tile_jobs = std::max(*max_tile_jobs, k);
    }
    for (char x : site_in_batch) CHECK(x);
    for (const mimeo_window_item &it : c.items) {
        const uint64_t b0 = c.first[it.aln], b1 = c.first[it.aln + 1];
        if (b0 == b1) continue;
        const uint64_t lo = std::max<uint64_t>(it.w0, c.blk[b0].t), hi = std::min<uint64_t>(it.w1, (uint64_t)c.blk[b1 - 1].t + c.blk[b1 - 1].len);
        for (uint64_t s = 0; s < c.sites.size(); s++)
            if (c.sites[s].window == it.group && c.sites[s].x >= lo && c.sites[s].x < hi) want[{it.aln, s}]++;
    }
    CHECK(seen == want);
}

int main() {
    std::string msg;
    Call c = valid();
    CHECK(c.ok(&msg) && msg.empty());
    // no sites; sites without an array; no items
    CHECK(validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), c.win.data(), c.win.size(), c.items.data(), c.items.size(),
                   nullptr, 0, &msg));
    CHECK(!validate(c.len_t, c.len_q, c.aln.data(), c.aln.size(), c.first.data(), c.blk.data(), c.blk.size(), c.win.data(), c.win.size(), c.items.data(), c.items.size(),
                    nullptr, 2, &msg) && msg == "mimeo_path_insertions: null argument");
    CHECK(validate(c.len_t, c.len_q, nullptr, 0, nullptr, nullptr, 0, c.win.data(), c.win.size(), nullptr, 0, c.sites.data(), c.sites.size(), &msg));
    // sites: window < nwin, start <= x < end, 1 <= ncols <= 1024, strictly increasing by (window, x)
    c = valid(); c.sites[7].window = 6;
    REFUSED(c, "site 7 (window 6, x 9999, ncols 1)", "window is not below nwin");
    c = valid(); c.sites[0].x = 49;
    REFUSED(c, "site 0 (window 0, x 49, ncols 1)", "x does not lie inside the window");
    c = valid(); c.sites[3].x = 300;
    REFUSED(c, "site 3 (window 0, x 300, ncols 7)", "x does not lie inside the window");
    c = valid(); c.sites[4].window = 4; c.sites[4].x = 70;   // nothing lies inside an empty window
    REFUSED(c, "site 4 (window 4, x 70, ncols 5)", "x does not lie inside the window");
    c = valid(); c.sites[1].ncols = 0;
    REFUSED(c, "site 1 (window 0, x 120, ncols 0)", "ncols is not in 1 .. 1024");
    c = valid(); c.sites[2].ncols = 1025;
    REFUSED(c, "site 2 (window 0, x 137, ncols 1025)", "ncols is not in 1 .. 1024");
    c = valid(); c.sites[2].x = 120;   // the same site twice
    REFUSED(c, "site 2 (window 0, x 120,", "not strictly increasing by (window, x)");
    c = valid(); c.sites[3].x = 130;   // x falls inside a window
    REFUSED(c, "site 3 (window 0, x 130,", "not strictly increasing by (window, x)");
    c = valid(); std::swap(c.sites[4], c.sites[5]);   // the window falls
    REFUSED(c, "site 5 (window 3, x 120,", "not strictly increasing by (window, x)");
    // the first bad site is the one named; a bad item comes before every site, a bad window before every item, a bad path first,
    // all under this entry point's name
    c = valid(); c.sites[1].ncols = 2000; c.sites[6].window = 77;
    REFUSED(c, "site 1 ", "ncols is not in 1 .. 1024");
    c = valid(); c.sites[0].window = 9; c.items[2].aln = 4;
    REFUSED(c, "item 2 (aln 4, window 1, [0, 5000))", "aln is not a record");
    c = valid(); c.items[3].group = 6;
    REFUSED(c, "item 3 (aln 2, window 6,", "window is not below nwin");
    c = valid(); c.items[0].group = 1;
    REFUSED(c, "item 0 (aln 0, window 1,", "does not lie on the record's target scaffold");
    c = valid(); c.items[5].w0 = 131;
    REFUSED(c, "item 5 (aln 0, window 0, [131, 130))", "w0 is beyond w1");
    c = valid(); c.items[1].w1 = 301;
    REFUSED(c, "item 1 ", "does not lie inside the window");
    c = valid(); c.items[0].aln = 77; c.win[5].end = 10001;
    REFUSED(c, "window 5 (tid 0, [0, 10001))", "end is beyond its scaffold");
    c = valid(); c.win[2].tid = 2;
    REFUSED(c, "window 2 (tid 2, [9000, 10000))", "tid is not a scaffold");
    c = valid(); c.win[4].start = 71;
    REFUSED(c, "window 4 (tid 1, [71, 70))", "start is beyond end");
    c = valid(); c.blk[1].len = 0; c.win[0].tid = 9; c.sites[0].ncols = 0;
    REFUSED(c, "record 0, block 1 ", "len is 0");
    c = valid(); c.first.back() += 1;
    REFUSED(c, "record 3:", "path_first[n] is not nblocks");
    c = valid(); c.max_window_items = 2;   // items 0, 5 and 9 name window 0
    REFUSED(c, "window 0 (tid 0, [50, 300))", "more than 2 items name it (item 9)");

    // the site tiles by hand, TILE_COLS = 1024: where the summed ncols reach 1023 and 1024 the next site still joins or the tile
    // is full; at 1025 it starts a tile of its own; a site of 1024 columns is a tile alone; a new window starts a tile
    {
        auto tiles_of = [](std::vector<mimeo_insert_site> s, uint64_t nwin) { return plan_sites(s.data(), s.size(), nwin); };
        Sites p = tiles_of({{0, 10, 1000, 0}, {0, 20, 23, 0}, {0, 30, 1, 0}}, 1);   // 1023, then 1024: one tile
        CHECK(p.tiles.size() == 1 && p.tiles[0].nsites == 3 && p.tiles[0].ncols == 1024 && p.nicols() == 1024);
        p = tiles_of({{0, 10, 1000, 0}, {0, 20, 23, 0}, {0, 30, 2, 0}}, 1);          // 1023, then 1025: the third site starts a tile
        CHECK(p.tiles.size() == 2 && p.tiles[0].nsites == 2 && p.tiles[0].ncols == 1023 && p.tiles[1].site0 == 2 && p.tiles[1].icol0 == 1023 && p.tiles[1].ncols == 2);
        p = tiles_of({{0, 10, 1000, 0}, {0, 20, 24, 0}, {0, 30, 1, 0}}, 1);          // 1024 exactly, then one more column: a new tile
        CHECK(p.tiles.size() == 2 && p.tiles[0].ncols == 1024 && p.tiles[1].nsites == 1 && p.tiles[1].icol0 == 1024);
        p = tiles_of({{0, 10, 1, 0}, {0, 20, 1024, 0}, {0, 30, 1, 0}}, 1);           // a site of 1024 columns alone
        CHECK(p.tiles.size() == 3 && p.tiles[1].nsites == 1 && p.tiles[1].ncols == 1024 && p.tiles[1].icol0 == 1 && p.tiles[2].icol0 == 1025);
        CHECK((p.icol_first == std::vector<uint64_t>{0, 1, 1025, 1026}));
        p = tiles_of({{0, 10, 1, 0}, {2, 10, 1, 0}, {2, 11, 1, 0}}, 4);              // a window of its own tile; windows 1 and 3 have no site
        CHECK(p.tiles.size() == 2 && p.tiles[1].window == 2 && p.tiles[1].nsites == 2 && (p.win_first == std::vector<uint64_t>{0, 1, 1, 3, 3}));
        // batches: tiles of 1024, 1, 1 columns under a bound of 1025: the first two, then the third; under 1: every tile alone
        p = tiles_of({{0, 10, 1024, 0}, {1, 20, 1, 0}, {2, 30, 1, 0}}, 3);
        Batch b = plan_batch(p, 0, 1025);
        CHECK(b.tile0 == 0 && b.tile1 == 2 && b.nsites == 2 && b.ncols == 1025 && b.site0 == 0 && b.icol0 == 0);
        b = plan_batch(p, 2, 1025);
        CHECK(b.tile1 == 3 && b.nsites == 1 && b.ncols == 1 && b.site0 == 2 && b.icol0 == 1025);
        b = plan_batch(p, 0, 1);
        CHECK(b.tile1 == 1 && b.ncols == 1024);
    }
    // bucketing by hand: the valid call's items on its sites, all in one batch
    {
        c = valid();
        const Sites p = plan_sites(c.sites.data(), c.sites.size(), c.win.size());
        // window 0: 1 + 3 + 1024 columns pass 1024: tiles {50, 120}, {137}, {299}; window 3: {120}; window 5: {0, 120, 9999}
        CHECK(p.tiles.size() == 5 && p.tiles[0].nsites == 2 && p.tiles[1].ncols == 1024 && p.tiles[2].ncols == 7 && p.tiles[3].window == 3 && p.tiles[4].window == 5);
        CHECK(p.tiles[4].ncols == 4 && p.tiles[4].nsites == 3);
        const Batch b = plan_batch(p, 0, 1ull << 22);
        CHECK(b.tile1 == 5 && b.nsites == 8 && b.ncols == p.nicols());
        std::vector<uint64_t> order(c.items.size());
        for (size_t i = 0; i < order.size(); i++) order[i] = i;
        TileItems ti;
        CHECK(bucket_tiles(p, b, c.first.data(), c.blk.data(), 0, c.sites.data(), c.items.data(), order.data(), 0, order.size(), 1ull << 22, ti) == order.size());
        // item 0 (record 0 over [100, 160) of window 0): sites 120 and 137, on tiles 0 and 1; item 1 the same of window 3: site 4;
        // item 7 (window 5, clipped to [100, 160)): site 120 = site 6, tile 4; item 8 (record 2 over [9990, 10000)): site 9999 = site
        // 7, tile 4 too; the empty item, the item that misses its alignment, the record without blocks and windows 1, 2: none
        CHECK((ti.start == std::vector<uint64_t>{0, 1, 2, 2, 3, 5}));
        auto is = [&](size_t e, uint32_t a, uint32_t s0, uint32_t s1) { return ti.entries[e].aln == a && ti.entries[e].s0 == s0 && ti.entries[e].s1 == s1; };
        CHECK(is(0, 0, 1, 2) && is(1, 0, 2, 3) && is(2, 0, 4, 5) && is(3, 0, 6, 7) && is(4, 2, 7, 8));
        std::vector<Job> jobs;
        plan_jobs(p, b, ti, 1, jobs);
        CHECK(jobs.size() == 5 && jobs[1].site0 == 2 && jobs[1].icol0 == 4 && jobs[1].ncols == 1024 && jobs[1].nsites == 1 && jobs[4].site0 == 5 && jobs[4].nsites == 3 &&
              jobs[4].item0 == 4);
        // an item that touches no site makes nothing: only the one that misses its alignment and the empty one
        const std::vector<uint64_t> none{5, 9};
        CHECK(bucket_tiles(p, b, c.first.data(), c.blk.data(), 0, c.sites.data(), c.items.data(), none.data(), 0, 2, 1ull << 22, ti) == 2 && ti.entries.empty());
        plan_jobs(p, b, ti, 64, jobs);
        CHECK(jobs.empty());
        // a run of at most one entry at a time: item 0 makes two and goes alone, whatever it makes
        CHECK(bucket_tiles(p, b, c.first.data(), c.blk.data(), 0, c.sites.data(), c.items.data(), order.data(), 0, order.size(), 1, ti) == 1 && ti.entries.size() == 2);
    }

    // every (item, site) in exactly one job entry, under every layout, job cuts of 1 and 7 among them
    size_t njobs = 0, nbatches = 0, max_tile_jobs = 0;
    c = valid();
    for (int k = 0; k < 70; k++) c.items.push_back({0, 0, 100u + k % 7, 160u - k % 5});   // 70 more items on the first tiles of window 0
    for (const uint32_t tile : {1024u, 2048u})
        for (const uint64_t batch : {1ull << 22, 1030ull, 1ull})
            for (const uint64_t run : {1ull << 22, 3ull})
                for (const uint64_t per : {64ull, 7ull, 1ull, 0ull})
                    cover(c, tile, batch, batch == 1 ? 1 : 1u << 22, run == 3 ? 1 : 1u << 24, run, per, &njobs, &nbatches, &max_tile_jobs);
    CHECK(max_tile_jobs >= 71 && nbatches > 50);
    // random small calls against the brute-force restatement
    std::mt19937 rng(14);
    for (int rep = 0; rep < 80; rep++) {
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
        // sites: a few per window, some at block junctions, with columns that make tiles of every size
        for (uint32_t g = 0; g < nwin; g++) {
            std::vector<uint32_t> xs;
            const uint32_t len = r.win[g].end - r.win[g].start;
            if (!len) continue;
            for (uint32_t k = rng() % 12; k > 0; k--) xs.push_back(r.win[g].start + rng() % len);
            for (const mimeo_path_block &b : r.blk)
                if (rng() % 3 == 0 && b.t >= r.win[g].start && b.t < r.win[g].end) xs.push_back(b.t);
            std::sort(xs.begin(), xs.end());
            xs.erase(std::unique(xs.begin(), xs.end()), xs.end());
            for (uint32_t x : xs) r.sites.push_back({g, x, (uint32_t)(rng() % 4 == 0 ? 1 + rng() % 1024 : 1 + rng() % 40), (uint32_t)(rng() % 9)});
        }
        CHECK(r.ok(&msg));
        const uint32_t tiles[] = {1024, 1500, 4096};
        const uint64_t batches[] = {1ull << 22, 1500, 300};
        cover(r, tiles[rep % 3], batches[(rep / 3) % 3], 1 + rng() % 5, 1 + rng() % 9, rep % 2 ? 1ull << 22 : 5, rep % 4 == 0 ? 7 : 1 + rng() % 9, &njobs, &nbatches,
              &max_tile_jobs);
    }
    printf("insert_check: ok %zu jobs, %zu batches, at most %zu jobs on a tile\n", njobs, nbatches, max_tile_jobs);
    return 0;
}
