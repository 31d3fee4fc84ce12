// The host side of mimeo_path_call_stats (mimeo_amd/csrc/call_stats_host.h: validate, validate_calls, plan_call, plan_jobs)
// under the CPU sanitizers: a valid call is accepted; a bad path, window, item, site or byte of either call is refused under
// this entry point's name; the offsets and iletters are the contract's sums; the jobs of a call cut every item's [lo, hi) into
// pieces of bounded size that hold every base once, with the sites and the letter columns the rules give; and the kernel's
// arithmetic over the jobs (the walk of the blocks of a piece, del_bases = gaps + site_letters - met, ins_bases = '-' under
// blocks + runs - met), restated here on the host, gives what the header's rules give column by column, over designed and
// random paths, whatever the slices and the job columns.  Built and run by tests/test_host_call_stats.py with
// -fsanitize=address,undefined.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>

#include "../../mimeo_amd/csrc/call_stats_host.h"

using namespace mimeo::call_stats_host;
using mimeo::path_stats_host::plan_slices;
using mimeo::window_stats_host::bucket_items;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "call_stats_check: %s failed at line %d\n", #c, __LINE__); exit(1); } } while (0)

struct Call {
    std::vector<uint64_t> len_t{10000, 5000}, len_q{800, 0xFFFFFFFFull};
    std::vector<mimeo_alignment> aln;
    std::vector<uint64_t> first{0};
    std::vector<mimeo_path_block> blk;
    std::vector<mimeo_pileup_window> win;
    std::vector<mimeo_window_item> items;
    std::vector<mimeo_insert_site> sites;
    std::vector<uint8_t> call, icall, query;   // query: the letters of the one aligned strand the counting reads
    void add(uint32_t tid, uint32_t qid, uint32_t qstrand, std::vector<mimeo_path_block> b) {
        mimeo_alignment a;
        memset(&a, 0, sizeof a);
        a.tid = tid; a.qid = qid; a.qstrand = qstrand;
        aln.push_back(a);
        blk.insert(blk.end(), b.begin(), b.end());
        first.push_back(blk.size());
    }
    // the two calls and the query from a generator: every byte one of the six (the query: A C G T N)
    void letters(std::mt19937 &rng, size_t nquery) {
        size_t nc = 0, ni = 0;
        for (const auto &w : win) nc += w.end - w.start;
        for (const auto &s : sites) ni += s.ncols;
        call.resize(nc); icall.resize(ni); query.resize(nquery);
        for (auto &b : call) b = "ACGTACGTACGTN-"[rng() % 14];
        for (auto &b : icall) b = "ACGTACGTN--"[rng() % 11];
        for (auto &b : query) b = "ACGTACGTACGTN"[rng() % 13];
    }
    bool ok(std::string *msg) const {
        return validate(len_t, len_q, aln.data(), aln.size(), first.data(), blk.data(), blk.size(), win.data(), win.size(), items.data(), items.size(),
                        sites.data(), sites.size(), msg) &&
               validate_calls(win.data(), win.size(), sites.data(), sites.size(), call.empty() ? nullptr : call.data(), icall.empty() ? nullptr : icall.data(), msg);
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
               {0, 0, 135, 140} /* the deletion, from its first base */, {0, 0, 160, 161} /* one column where both jump */, {0, 0, 100, 120} /* w1 == p_k */};
    // a site at the first block's t (100: not spanned), at a run (120, fewer columns than bases; 160), inside the deletion (137), off
    // the alignment (50, 299), at x and x + 1 (3: 120, 121)
    c.sites = {{0, 50, 1, 3}, {0, 100, 2, 0}, {0, 120, 2, 3}, {0, 137, 1024, 0}, {0, 160, 5, 0}, {0, 299, 7, 1}, {3, 120, 5, 2}, {3, 121, 16, 2}, {5, 0, 1, 9},
               {5, 120, 3, 9}, {5, 9999, 1, 0xFFFFFFFFu}};
    std::mt19937 rng(16);
    c.letters(rng, 800);
    return c;
}

static void refused(const Call &c, const char *who, const char *why, int line) {
    std::string msg;
    if (c.ok(&msg) || msg.find("mimeo_path_call_stats: ") != 0 || msg.find(who) == std::string::npos || msg.find(why) == std::string::npos) {
        fprintf(stderr, "call_stats_check: line %d: expected a refusal naming '%s' '%s', got '%s'\n", line, who, why, msg.c_str());
        exit(1);
    }
}
#define REFUSED(c, who, why) refused(c, who, why, __LINE__)

struct Counts {
    uint64_t v[6] = {0, 0, 0, 0, 0, 0};   // matches, transitions, transversions, ambiguous, ins_bases, del_bases
    bool operator==(const Counts &o) const { return !memcmp(v, o.v, sizeof v); }
};
static int code(uint8_t b) { return b == 'A' ? 0 : b == 'C' ? 1 : b == 'G' ? 2 : b == 'T' ? 3 : 4; }
static void classify(Counts &n, uint8_t c, uint8_t y) {
    const int a = code(c), b = code(y);
    if (a == 4 || b == 4) n.v[3]++;
    else if (a == b) n.v[0]++;
    else if ((a ^ b) == 2) n.v[1]++;
    else n.v[2]++;
}

// the header's rules, column by column, for one item (all records of the check read the one `query`)
static Counts by_rule(const Call &c, const Plan &p, const mimeo_window_item &it) {
    Counts n;
    const uint64_t b0 = c.first[it.aln], b1 = c.first[it.aln + 1];
    if (b0 == b1) return n;
    const uint64_t ft = c.blk[b0].t, le = (uint64_t)c.blk[b1 - 1].t + c.blk[b1 - 1].len;
    const uint64_t lo = std::max<uint64_t>(it.w0, ft), hi = std::min<uint64_t>(it.w1, le);
    if (lo >= hi) return n;
    const uint64_t col0 = p.col_first[it.group] - c.win[it.group].start;
    std::map<uint64_t, std::pair<uint64_t, uint64_t>> runs;   // p_k -> (first inserted base, dq_k)
    for (uint64_t k = b0; k < b1; k++) {
        const mimeo_path_block &b = c.blk[k];
        for (uint64_t x = std::max<uint64_t>(lo, b.t); x < std::min<uint64_t>(hi, (uint64_t)b.t + b.len); x++) {
            const uint8_t cb = c.call[col0 + x];
            if (cb == '-') n.v[4]++; else classify(n, cb, c.query[b.q + (x - b.t)]);
        }
        if (k == b0) continue;
        const mimeo_path_block &pb = c.blk[k - 1];
        const uint64_t pk = (uint64_t)pb.t + pb.len, qs = (uint64_t)pb.q + pb.len;
        for (uint64_t x = std::max(lo, pk); x < std::min<uint64_t>(hi, b.t); x++) n.v[5] += c.call[col0 + x] != '-';
        if (b.q > qs && it.w0 <= pk && pk < it.w1) runs[pk] = {qs, b.q - qs};
    }
    std::map<uint64_t, bool> sited;
    for (size_t s = 0; s < c.sites.size(); s++) {
        if (c.sites[s].window != it.group) continue;
        const uint64_t x = c.sites[s].x;
        const auto r = runs.find(x);
        const uint64_t dq = r == runs.end() ? 0 : r->second.second;
        if (dq) sited[x] = true;
        for (uint64_t j = 0; j < c.sites[s].ncols; j++) {
            const uint8_t ib = c.icall[p.site[s].icol + j];
            if (j < dq) { if (ib == '-') n.v[4]++; else classify(n, ib, c.query[r->second.first + j]); }
            else if (ib != '-' && it.w0 <= x && x < it.w1 && ft < x && x < le) n.v[5]++;
        }
        if (dq > c.sites[s].ncols) n.v[4] += dq - c.sites[s].ncols;
    }
    for (const auto &r : runs) if (!sited.count(r.first)) n.v[4] += r.second.second;
    return n;
}

// the kernel's arithmetic for one job, lane by lane turned block by block
static Counts by_job(const Call &c, const Plan &p, const Job &j, uint64_t a0) {
    Counts n;
    const uint64_t aln = a0 + j.aln, b0 = c.first[aln], b1 = c.first[aln + 1];
    uint64_t met = 0;
    for (uint64_t k = b0; k < b1; k++) {
        const mimeo_path_block &b = c.blk[k];
        uint64_t pend = b.t, pq = 0, dq = 0;
        if (k > b0) { pend = (uint64_t)c.blk[k - 1].t + c.blk[k - 1].len; pq = (uint64_t)c.blk[k - 1].q + c.blk[k - 1].len; dq = b.q - pq; }
        if ((uint64_t)b.t + b.len <= j.w0 || pend >= j.w1) continue;
        for (uint64_t x = std::max<uint64_t>(pend, j.w0); x < std::min<uint64_t>(b.t, j.w1); x++) n.v[5] += c.call[j.col + (x - j.w0)] != '-';
        if (pend >= j.w0 && dq) {
            n.v[4] += dq;
            for (uint32_t s = j.site0; s < j.site1; s++)
                if (p.site[s].x == pend)
                    for (uint64_t i = 0; i < std::min<uint64_t>(dq, p.site[s].ncols); i++) {
                        const uint8_t ib = c.icall[j.icol0 + (p.site[s].icol - p.site[j.site0].icol) + i];
                        if (ib != '-') { met++; classify(n, ib, c.query[pq + i]); }
                    }
        }
        for (uint64_t x = std::max<uint64_t>(b.t, j.w0); x < std::min<uint64_t>((uint64_t)b.t + b.len, j.w1); x++) {
            const uint8_t cb = c.call[j.col + (x - j.w0)];
            if (cb == '-') n.v[4]++; else classify(n, cb, c.query[b.q + (x - b.t)]);
        }
    }
    CHECK(met <= n.v[4] && met <= j.site_letters);
    n.v[4] -= met;
    n.v[5] += j.site_letters - met;
    return n;
}

// every base of every item's [lo, hi) in exactly one job; the sums of the jobs are the rules' counts
static void cover(const Call &c, uint64_t max_rec, uint64_t max_blk, uint64_t job_columns, size_t *njobs) {
    const Plan p = plan_call(c.win.data(), c.win.size(), c.sites.data(), c.sites.size(), c.icall.empty() ? nullptr : c.icall.data());
    CHECK(p.ncols() == c.call.size() && p.nicols() == c.icall.size());
    for (size_t s = 0; s < c.sites.size(); s++) {
        uint64_t letters = 0;
        for (uint32_t jj = 0; jj < c.sites[s].ncols; jj++) letters += c.icall[p.site[s].icol + jj] != '-';
        CHECK(p.iletters[s + 1] - p.iletters[s] == letters && p.site[s].x == c.sites[s].x && p.site[s].ncols == c.sites[s].ncols);
        CHECK(s >= p.win_first[c.sites[s].window] && s < p.win_first[c.sites[s].window + 1]);
        if (s) CHECK(p.site[s].icol == p.site[s - 1].icol + c.sites[s - 1].ncols);
    }
    const auto slices = plan_slices(c.first.data(), c.aln.size(), max_rec, max_blk);
    std::vector<uint64_t> order, start;
    bucket_items(slices, c.items.data(), c.items.size(), order, start);
    std::vector<Counts> sum(c.items.size());
    std::vector<std::map<uint64_t, int>> hit(c.items.size());
    const uint64_t jc = job_columns && job_columns <= MAX_JOB_COLUMNS ? job_columns : DEFAULT_JOB_COLUMNS;
    std::vector<Job> jobs;
    for (size_t s = 0; s < slices.size(); s++) {
        plan_jobs(p, c.win.data(), c.first.data(), c.blk.data(), slices[s].first, c.items.data(), order.data(), start[s], start[s + 1], job_columns, jobs);
        for (const Job &j : jobs) {
            (*njobs)++;
            CHECK(j.item < c.items.size() && j.w0 < j.w1 && j.w1 - j.w0 <= jc && j.site0 <= j.site1 && j.site1 <= c.sites.size());
            const mimeo_window_item &it = c.items[j.item];
            CHECK(j.aln + slices[s].first == it.aln && it.aln < slices[s].second);
            const uint64_t b0 = c.first[it.aln], b1 = c.first[it.aln + 1];
            CHECK(b1 > b0 && j.w0 >= std::max(it.w0, c.blk[b0].t) && j.w1 <= std::min<uint64_t>(it.w1, (uint64_t)c.blk[b1 - 1].t + c.blk[b1 - 1].len));
            CHECK(j.col == p.col_first[it.group] + (j.w0 - c.win[it.group].start) && j.col + (j.w1 - j.w0) <= c.call.size());
            for (uint64_t x = j.w0; x < j.w1; x++) CHECK(hit[j.item][x]++ == 0);
            uint64_t letters = 0;
            for (size_t k = 0; k < c.sites.size(); k++) {   // the sites of the piece that the alignment spans, by the rule
                const bool mine = c.sites[k].window == it.group && c.sites[k].x >= j.w0 && c.sites[k].x < j.w1 && c.sites[k].x > c.blk[b0].t;
                CHECK(mine == (k >= j.site0 && k < j.site1));
                if (mine) letters += p.iletters[k + 1] - p.iletters[k];
            }
            CHECK(letters == j.site_letters && (j.site0 == j.site1 || j.icol0 == p.site[j.site0].icol));
            const Counts n = by_job(c, p, j, slices[s].first);
            for (int k = 0; k < 6; k++) sum[j.item].v[k] += n.v[k];
        }
    }
    for (size_t k = 0; k < c.items.size(); k++) {
        const mimeo_window_item &it = c.items[k];
        const uint64_t b0 = c.first[it.aln], b1 = c.first[it.aln + 1];
        uint64_t want = 0;
        if (b1 > b0) {
            const uint64_t lo = std::max(it.w0, c.blk[b0].t), hi = std::min<uint64_t>(it.w1, (uint64_t)c.blk[b1 - 1].t + c.blk[b1 - 1].len);
            want = hi > lo ? hi - lo : 0;
        }
        CHECK(hit[k].size() == want);
        const Counts r = by_rule(c, p, it);
        if (!(sum[k] == r)) {
            fprintf(stderr, "call_stats_check: item %zu (aln %u, window %u, [%u, %u)), job columns %llu: jobs", k, it.aln, it.group, it.w0, it.w1, (unsigned long long)jc);
            for (int i = 0; i < 6; i++) fprintf(stderr, " %llu", (unsigned long long)sum[k].v[i]);
            fprintf(stderr, ", rules");
            for (int i = 0; i < 6; i++) fprintf(stderr, " %llu", (unsigned long long)r.v[i]);
            fprintf(stderr, "\n");
            exit(1);
        }
        // the guarantee of the header: the classified columns and ins_bases are the bases of the stretch
        uint32_t ql, qh;
        mimeo::stack_host::query_stretch(c.first.data(), c.blk.data(), it, &ql, &qh);
        CHECK(r.v[0] + r.v[1] + r.v[2] + r.v[3] + r.v[4] == qh - ql);
    }
}

int main() {
    std::string msg;
    const Call v = valid();
    if (!v.ok(&msg)) { fprintf(stderr, "call_stats_check: the valid call was refused: %s\n", msg.c_str()); return 1; }
    { Call c = valid(); c.sites.clear(); c.icall.clear(); CHECK(c.ok(&msg)); }   // no site at all is legal, icall is then NULL
    { Call c = valid(); c.items.clear(); CHECK(c.ok(&msg)); }
    // the checks of mimeo_path_stack, in their order, under this entry point's name
    { Call c = valid(); c.blk[1].t = 110; REFUSED(c, "record 0, block 1", "overlaps the block before it"); }
    { Call c = valid(); c.win[2].end = 10001; c.items[0].aln = 99; REFUSED(c, "window 2", "end is beyond its scaffold"); }
    { Call c = valid(); c.items[3].w1 = 10001; c.sites[0].ncols = 0; REFUSED(c, "item 3", "does not lie inside the window"); }
    { Call c = valid(); c.items[2].group = 0; REFUSED(c, "item 2", "does not lie on the record's target scaffold"); }
    { Call c = valid(); c.sites[1].window = 7; REFUSED(c, "site 1", "window is not below nwin"); }
    { Call c = valid(); c.sites[5].x = 300; REFUSED(c, "site 5", "x does not lie inside the window"); }
    { Call c = valid(); c.sites[3].ncols = 1025; REFUSED(c, "site 3", "ncols is not in 1 .. 1024"); }
    { Call c = valid(); c.sites[7].x = 120; REFUSED(c, "site 7", "not strictly increasing"); }
    { Call c = valid(); for (auto &s : c.sites) s.voters = 0; CHECK(c.ok(&msg)); }   // voters is not read
    // the bytes of the two calls, checked last: the first and the last byte, lower case, '.', NUL
    { Call c = valid(); c.call[0] = 'a'; REFUSED(c, "column 0 of call (window 0, x 50)", "byte 0x61 is not one of A C G T N -"); }
    { Call c = valid(); c.call[250 + 5000 + 999] = '.'; REFUSED(c, "column 6249 of call (window 2, x 9999)", "byte 0x2e"); }
    { Call c = valid(); c.call.back() = 0; REFUSED(c, "of call (window 6, x 138)", "byte 0x00"); }
    { Call c = valid(); c.icall[0] = 'n'; REFUSED(c, "insertion column 0 of icall (site 0, column 0)", "byte 0x6e"); }
    { Call c = valid(); c.icall.back() = 'R'; REFUSED(c, "of icall (site 10, column 0)", "byte 0x52"); }
    { Call c = valid(); c.icall[1 + 2 + 1] = '*'; REFUSED(c, "insertion column 4 of icall (site 2, column 1)", "byte 0x2a"); }
    { Call c = valid(); c.call[3] = 'x'; c.sites[3].ncols = 0; REFUSED(c, "site 3", "ncols is not in 1 .. 1024"); }   // a bad site is named before a bad byte
    { Call c = valid(); c.call[3] = 'x'; c.icall[0] = 'x'; REFUSED(c, "column 3 of call", "byte 0x78"); }            // call before icall
    { Call c = valid(); c.icall.clear(); REFUSED(c, "null argument", ""); }   // icall == NULL with nicols > 0
    { Call c = valid(); c.call.clear(); REFUSED(c, "null argument", ""); }
    { Call c = valid(); c.items.clear(); c.call[7] = '?'; REFUSED(c, "column 7 of call", "byte 0x3f"); }   // the checks run for a call without items too

    size_t njobs = 0, nj1 = 0;
    cover(v, 1ull << 22, 1ull << 24, 0, &nj1);
    CHECK(nj1 == 13);   // one per item that reaches its alignment
    for (uint64_t max_blk : {1ull, 3ull, 1ull << 24})
        for (uint64_t jc : std::vector<uint64_t>{1, 2, 7, 64, 100, MAX_JOB_COLUMNS, MAX_JOB_COLUMNS + 1}) cover(v, 1ull << 22, max_blk, jc, &njobs);
    cover(v, 1, 1, 1, &njobs);
    // every window over the first record, base by base: all the edges of blocks, runs, deletions and sites
    {
        Call c = valid();
        c.items.clear();
        for (uint32_t w0 = 95; w0 <= 185; w0 += 1)
            for (uint32_t w1 = w0; w1 <= 185; w1 += 1) c.items.push_back({0, 0, w0, w1});
        cover(c, 1ull << 22, 1ull << 24, 0, &njobs);
        cover(c, 1ull << 22, 1ull << 24, 3, &njobs);
    }
    // random paths, sites and letters
    std::mt19937 rng(16);
    for (int round = 0; round < 300; round++) {
        Call c;
        c.len_t = {200}; c.len_q = {400};
        for (int a = 0; a < 3; a++) {
            std::vector<mimeo_path_block> b;
            uint32_t t = 10 + rng() % 20, q = rng() % 20;
            const int nb = rng() % 8;
            for (int k = 0; k < nb; k++) {
                const uint32_t len = 1 + rng() % 5;
                b.push_back({t, q, len});
                t += len + (rng() % 3 ? 0 : rng() % 4);
                q += len + (rng() % 3 ? 0 : rng() % 6);
            }
            c.add(0, 0, 0, b);
        }
        c.win = {{0, 0, 100}, {0, 5, 80}};
        for (uint32_t g = 0; g < 2; g++)
            for (uint32_t x = c.win[g].start + rng() % 3; x < c.win[g].end; x += 1 + rng() % 4) c.sites.push_back({g, x, 1 + (uint32_t)(rng() % 4), 0});
        for (int k = 0; k < 40; k++) {
            const uint32_t g = rng() % 2, w0 = c.win[g].start + rng() % 70;
            c.items.push_back({(uint32_t)(rng() % 3), g, w0, std::min(c.win[g].end, w0 + (uint32_t)(rng() % 60))});
        }
        c.letters(rng, 400);
        CHECK(c.ok(&msg));
        cover(c, 1ull << 22, round % 2 ? 1 : 1ull << 24, round % 3 ? 1 + rng() % 9 : 0, &njobs);
    }
    CHECK(njobs > 10000);
    printf("call_stats_check: ok (%zu jobs)\n", njobs);
    return 0;
}
