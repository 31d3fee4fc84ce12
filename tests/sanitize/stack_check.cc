// The host side of mimeo_path_stack (mimeo_amd/csrc/stack_host.h: validate, plan_layout, row_first_of, query_stretch,
// plan_batch) under the CPU sanitizers: a valid call is accepted; a bad path, window, item or site is refused under this entry
// point's name; the column of every target base and of every insertion column is the one the contract's sums give; the query
// stretch of an item is the one a base-by-base restatement finds; and the batches and jobs of a call hold every column of every
// row exactly once, whatever the slices, the batch bytes and the job columns.  Built and run by tests/test_host_stack.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/stack_host.h"

using namespace mimeo::stack_host;
using mimeo::path_stats_host::plan_slices;
using mimeo::window_stats_host::bucket_items;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "stack_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{10000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_pileup_window> win;
    std::vector<mimeo_window_item> items;
    std::vector<mimeo_insert_site> sites;
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
                        sites.data(), sites.size(), msg);
    }
};

static Call valid() {
    Call c;
    // 3 inserted bases in front of 120, a deletion [135, 140), both sequences jump at 160 (2 bases, then [160, 164)): [100, 180)
    c.add(0, 0, 0, {{100, 50, 20}, {120, 73, 15}, {140, 88, 20}, {164, 110, 16}});
    c.add(1, 0, 1, {{0, 0, 1}});         // starts at base 0 of scaffold 1
    c.add(0, 0, 1, {{9990, 790, 10}});   // ends on the last base of both scaffolds
    c.add(1, 1, 0, {});                  // no blocks
    c.win = {{0, 50, 300}, {1, 0, 5000}, {0, 9000, 10000}, {0, 50, 300} /* a window twice */, {1, 70, 70} /* empty */, {0, 0, 10000}, {0, 136, 139}};
    c.items = {{0, 0, 100, 180}, {0, 3, 50, 300}, {1, 1, 0, 5000}, {2, 2, 9995, 10000}, {3, 1, 10, 20}, {0, 0, 130, 130} /* an empty item */,
               {3, 4, 70, 70}, {0, 5, 0, 10000}, {2, 5, 0, 10000}, {0, 0, 200, 300} /* misses its alignment */, {0, 0, 100, 180} /* twice */,
               {0, 6, 136, 139} /* inside the deletion */, {0, 0, 120, 135} /* w0 == p_k */, {0, 0, 110, 137} /* w1 inside the deletion */,
               {0, 0, 135, 140} /* the deletion, from its first base */, {0, 0, 160, 161} /* one column where both jump */};
    c.sites = {{0, 50, 1, 3}, {0, 120, 3, 3}, {0, 137, 1024, 0}, {0, 160, 1, 0}, {0, 299, 7, 1}, {3, 120, 5, 2}, {3, 121, 16, 2}, {5, 0, 1, 9}, {5, 120, 2, 9},
               {5, 9999, 1, 0xFFFFFFFFu}};
    return c;
}

static void refused(const Call &c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find("mimeo_path_stack: ") != 0 || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "stack_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

// the contract's sums, base by base
static void layout(const Call &c) {
    const Layout L = plan_layout(c.win.data(), c.win.size(), c.sites.data(), c.sites.size());
    CHECK(L.win.size() == c.win.size() && L.site.size() == c.sites.size() && L.width.size() == c.win.size());
    uint64_t seen = 0;
    for (size_t g = 0; g < c.win.size(); g++) {
        uint64_t w = c.win[g].end - c.win[g].start;
        CHECK(L.win[g].start == c.win[g].start && L.win[g].end == c.win[g].end && L.win[g].site0 == seen);
        for (size_t s = 0; s < c.sites.size(); s++) {
            if (c.sites[s].window != g) continue;
            CHECK(s >= L.win[g].site0 && s < L.win[g].site1);
            seen++;
            w += c.sites[s].ncols;
            uint64_t tcol = c.sites[s].x - c.win[g].start;   // the column of x_s: the sites with x_i <= x_s, itself among them
            for (size_t i = 0; i < c.sites.size(); i++)
                if (c.sites[i].window == g && c.sites[i].x <= c.sites[s].x) tcol += c.sites[i].ncols;
            CHECK(L.site[s].x == c.sites[s].x && L.site[s].ncols == c.sites[s].ncols && L.site[s].col == tcol - c.sites[s].ncols);
        }
        CHECK(L.win[g].site1 == seen && L.width[g] == w);
    }
    CHECK(seen == c.sites.size());
    std::vector<uint64_t> rf(c.items.size() + 1, 7);
    row_first_of(L, c.items.data(), c.items.size(), rf.data());
    CHECK(rf[0] == 0);
    for (size_t k = 0; k < c.items.size(); k++) CHECK(rf[k + 1] - rf[k] == L.width[c.items[k].group]);
}

// the query stretch of an item, base by base: the bases under its target columns and its runs with w0 <= p_k < w1
static void stretch(const Call &c, const mimeo_window_item &it) {
    uint64_t lo = ~0ull, hi = 0;
    auto take = [&](uint64_t a, uint64_t b) { if (a < b) { lo = std::min(lo, a); hi = std::max(hi, b); } };
    for (uint64_t k = c.first[it.aln]; k < c.first[it.aln + 1]; k++) {
        const mimeo_path_block &b = c.blk[k];
        const uint64_t x0 = std::max<uint64_t>(it.w0, b.t), x1 = std::min<uint64_t>(it.w1, (uint64_t)b.t + b.len);
        if (x0 < x1) take(b.q + (x0 - b.t), b.q + (x1 - b.t));
        if (k > c.first[it.aln]) {
            const mimeo_path_block &pb = c.blk[k - 1];
            const uint64_t p = (uint64_t)pb.t + pb.len;
            if (it.w0 <= p && p < it.w1) take((uint64_t)pb.q + pb.len, b.q);
        }
    }
    uint32_t ql = 9, qh = 9;
    const bool any = query_stretch(c.first.data(), c.blk.data(), it, &ql, &qh);
    if (hi == 0) CHECK(!any && ql == 0 && qh == 0);
    else CHECK(any && ql == lo && qh == hi);
}

// every column of every row exactly once, in batches of bounded bytes and jobs of bounded columns
static void cover(const Call &c, uint64_t max_rec, uint64_t max_blk, uint64_t max_bytes, uint64_t job_columns, size_t *nbatches, size_t *njobs) {
    const Layout L = plan_layout(c.win.data(), c.win.size(), c.sites.data(), c.sites.size());
    const auto slices = plan_slices(c.first.data(), c.aln.size(), max_rec, max_blk);
    std::vector<uint64_t> order, start;
    bucket_items(slices, c.items.data(), c.items.size(), order, start);
    std::vector<std::vector<char>> hit(c.items.size());
    for (size_t k = 0; k < c.items.size(); k++) hit[k].assign(L.width[c.items[k].group], 0);
    std::vector<char> item_seen(c.items.size(), 0);
    Batch b;
    for (size_t s = 0; s < slices.size(); s++)
        for (uint64_t i0 = start[s]; i0 < start[s + 1]; i0 = b.i1) {
            plan_batch(L, c.items.data(), order.data(), slices[s].first, i0, start[s + 1], max_bytes, job_columns, b);
            (*nbatches)++;
            CHECK(b.i0 == i0 && b.i1 > i0 && b.i1 <= start[s + 1] && b.rows.size() == b.i1 - b.i0);
            CHECK(b.rows.size() == 1 || b.bytes <= max_bytes);
            if (b.i1 < start[s + 1]) CHECK(b.bytes + L.width[c.items[order[b.i1]].group] > max_bytes);
            uint64_t at = 0;
            for (size_t r = 0; r < b.rows.size(); r++) {
                const uint64_t k = order[b.i0 + r];
                const mimeo_window_item &it = c.items[k];
                CHECK(!item_seen[k]);
                item_seen[k] = 1;
                CHECK(b.rows[r].off == at && b.rows[r].aln + slices[s].first == it.aln && it.aln >= slices[s].first && it.aln < slices[s].second);
                CHECK(b.rows[r].window == it.group && b.rows[r].w0 == it.w0 && b.rows[r].w1 == it.w1);
                at += L.width[it.group];
            }
            CHECK(at == b.bytes);
            for (const Job &j : b.jobs) {
                (*njobs)++;
                CHECK(j.row < b.rows.size() && j.c0 < j.c1 && j.c1 - j.c0 <= (job_columns ? job_columns : DEFAULT_JOB_COLUMNS));
                std::vector<char> &h = hit[order[b.i0 + j.row]];
                CHECK(j.c1 <= h.size());
                for (uint64_t x = j.c0; x < j.c1; x++) { CHECK(!h[x]); h[x] = 1; }
            }
        }
    for (size_t k = 0; k < c.items.size(); k++) {
        CHECK(item_seen[k]);
        for (char v : hit[k]) CHECK(v);
    }
}

int main() {
    std::string msg;
    const Call v = valid();
    if (!v.ok(&msg)) { fprintf(stderr, "stack_check: the valid call was refused: %s\n", msg.c_str()); return 1; }
    { Call c = valid(); c.sites.clear(); CHECK(c.ok(&msg)); }   // no site at all is legal
    { Call c = valid(); c.items.clear(); CHECK(c.ok(&msg)); }
    // the checks of mimeo_path_insertions, in their order, under this entry point's name
    { Call c = valid(); c.blk[1].t = 110; REFUSED(c, "record 0, block 1", "overlaps the block before it"); }
    { Call c = valid(); c.win[2].end = 10001; c.items[0].aln = 99; REFUSED(c, "window 2", "end is beyond its scaffold"); }
    { Call c = valid(); c.items[3].w1 = 10001; c.sites[0].ncols = 0; REFUSED(c, "item 3", "does not lie inside the window"); }
    { Call c = valid(); c.items[2].group = 0; REFUSED(c, "item 2", "does not lie on the record's target scaffold"); }
    { Call c = valid(); c.sites[1].window = 7; REFUSED(c, "site 1", "window is not below nwin"); }
    { Call c = valid(); c.sites[4].x = 300; REFUSED(c, "site 4", "x does not lie inside the window"); }
    { Call c = valid(); c.sites[2].ncols = 1025; REFUSED(c, "site 2", "ncols is not in 1 .. 1024"); }
    { Call c = valid(); c.sites[2].ncols = 0; REFUSED(c, "site 2", "ncols is not in 1 .. 1024"); }
    { Call c = valid(); c.sites[6].x = 120; REFUSED(c, "site 6", "not strictly increasing"); }
    { Call c = valid(); std::swap(c.sites[4], c.sites[5]); REFUSED(c, "site 5", "not strictly increasing"); }
    { Call c = valid(); for (auto &s : c.sites) s.voters = 0; CHECK(c.ok(&msg)); }   // voters is not read

    layout(v);
    for (const mimeo_window_item &it : v.items) stretch(v, it);
    // every window over the first record, base by base: all the edges of blocks, runs and deletions
    for (uint32_t w0 = 95; w0 <= 185; w0++)
        for (uint32_t w1 = w0; w1 <= 185; w1++) stretch(v, mimeo_window_item{0, 5, w0, w1});
    // random paths
    std::mt19937 rng(15);
    for (int round = 0; round < 200; round++) {
        Call c;
        std::vector<mimeo_path_block> b;
        uint32_t t = 10 + rng() % 20, q = rng() % 20;
        const int nb = 1 + rng() % 6;
        for (int k = 0; k < nb; k++) {
            const uint32_t len = 1 + rng() % 5;
            b.push_back({t, q, len});
            t += len + (rng() % 3 ? 0 : rng() % 4);
            q += len + (rng() % 3 ? 0 : rng() % 4);
        }
        c.add(0, 0, 0, b);
        c.win = {{0, 0, 100}};
        for (uint32_t w0 = 5; w0 <= t + 3; w0++)
            for (uint32_t w1 = w0; w1 <= t + 3; w1++) stretch(c, mimeo_window_item{0, 0, w0, w1});
    }

    size_t nbatches = 0, njobs = 0, nb1 = 0, nj1 = 0;
    cover(v, 1ull << 22, 1ull << 24, DEFAULT_BATCH_BYTES, DEFAULT_JOB_COLUMNS, &nb1, &nj1);
    CHECK(nb1 == 1);
    cover(v, 1ull << 22, 1ull << 24, DEFAULT_BATCH_BYTES, 0, &nbatches, &njobs);
    for (uint64_t max_blk : {1ull, 3ull, 1ull << 24})
        for (uint64_t max_bytes : {1ull, 16ull, 250ull, 1300ull, 20000ull})
            for (uint64_t jc : {1ull, 15ull, 16ull, 17ull, 1000ull}) {
                if (jc == 1 && max_bytes > 16) continue;   // one job per column of ten thousand: once is enough
                cover(v, 1ull << 22, max_blk, max_bytes, jc, &nbatches, &njobs);
            }
    cover(v, 1, 1, 1, 16, &nbatches, &njobs);
    CHECK(nbatches > 50 && njobs > nj1);
    printf("stack_check: ok (%zu batches, %zu jobs)\n", nbatches, njobs);
    return 0;
}
