// Host-side logic of the library under the CPU sanitizers (GPU AddressSanitizer is not available on the pool):
//   * the threaded FASTA ingest (mimeo_amd/csrc/ingest_host.h: parser thread, two staging slots, hand-over, abort)
//     with malloc in the place of pinned memory and a consumer that keeps the bytes;
//   * the planning code of the pipeline (mimeo_amd/csrc/host_plan.h: super-scaffold plan, cross-product test, index
//     blocks, mirror pairing, batch cut).
// Built and run by tests/test_host_sanitize.py with -fsanitize=address,undefined and with -fsanitize=thread.
#include <cassert>
#include <cstdio>
#include <cstdlib>
#include <limits>
#include <random>
#include <set>
#include <string>
#include <vector>

#include "../../mimeo_amd/csrc/host_plan.h"
#include "../../mimeo_amd/csrc/ingest_host.h"

using namespace mimeo;

struct MallocMem {
    static void *alloc(size_t n) { return malloc(n); }
    static void release(void *p) { free(p); }
    static void thread_init(int) {}
};

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "CHECK failed: %s (%s:%d)\n", #c, __FILE__, __LINE__); exit(1); } } while (0)

struct Rec { std::string name, header, seq; };

// the plain restatement the ingest is checked against (Biopython SimpleFastaParser semantics: text before the first header
// ignored, blanks and line ends inside a record dropped, id = first word of the header)
static std::vector<Rec> reference_parse(const std::vector<std::string> &texts) {
    std::vector<Rec> out;
    for (const std::string &t : texts) {
        bool open = false;
        size_t p = 0;
        while (p <= t.size()) {
            size_t nl = t.find('\n', p);
            if (nl == std::string::npos) nl = t.size();
            std::string line = t.substr(p, nl - p);
            p = nl + 1;
            if (!line.empty() && line[0] == '>') {
                std::string h = line.substr(1);
                while (!h.empty() && h.back() == '\r') h.pop_back();
                Rec r;
                r.header = h;
                size_t a = 0;
                while (a < h.size() && (h[a] == ' ' || h[a] == '\t')) a++;
                size_t b = a;
                while (b < h.size() && h[b] != ' ' && h[b] != '\t') b++;
                r.name = h.substr(a, b - a);
                out.push_back(r);
                open = true;
            } else if (open) {
                for (char c : line) if (c != ' ' && c != '\t' && c != '\r') out.back().seq.push_back(c);
            }
            if (nl == t.size()) break;
        }
    }
    return out;
}

static std::string random_fasta(std::mt19937 &rng, int nrec, bool crlf, bool trailing_newline) {
    std::string t;
    if (rng() % 2) t += "this text precedes the first header\n";
    const char *alpha = "ACGTacgtNn";
    for (int r = 0; r < nrec; r++) {
        t += ">rec" + std::to_string(rng() % 100000) + "_" + std::to_string(r) + (rng() % 2 ? " some description" : "") + (crlf ? "\r\n" : "\n");
        size_t len = (rng() % 8 == 0) ? 0 : rng() % 5000;
        if (rng() % 16 == 0) len = 300000 + rng() % 50000;   // longer than the chunk and the first staging capacity of the test
        size_t col = 0, width = 1 + rng() % 120;
        for (size_t i = 0; i < len; i++) {
            t.push_back(alpha[rng() % 10]);
            if (rng() % 997 == 0) t.push_back(' ');
            if (++col == width) { t += crlf ? "\r\n" : "\n"; col = 0; if (rng() % 50 == 0) t += "\n"; }
        }
        if (col && (r + 1 < nrec || trailing_newline)) t += crlf ? "\r\n" : "\n";
    }
    return t;
}

static void write_file(const std::string &path, const std::string &text) {
    FILE *f = fopen(path.c_str(), "wb");
    CHECK(f);
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
}

static void test_ingest(const std::string &dir) {
    std::mt19937 rng(12345);
    for (int round = 0; round < 12; round++) {
        std::vector<std::string> texts, paths;
        const int nfiles = 1 + rng() % 3;
        for (int f = 0; f < nfiles; f++) {
            texts.push_back(random_fasta(rng, 1 + rng() % 12, rng() % 3 == 0, rng() % 2));
            paths.push_back(dir + "/in_" + std::to_string(round) + "_" + std::to_string(f) + ".fa");
            write_file(paths.back(), texts.back());
        }
        const std::vector<Rec> want = reference_parse(texts);
        ingest_host::Ingest<MallocMem> in;
        in.chunk_bytes = 1 + rng() % 70000;   // lines straddle chunks
        in.first_cap = 64;                    // the staging buffers grow many times
        std::vector<Rec> got;
        int rc = in.run(paths, [&](ingest_host::Slot &s) -> int {
            got.push_back(Rec{s.name, s.header, std::string((const char *)s.buf, s.len)});
            return 0;
        });
        CHECK(rc == 0);
        CHECK(got.size() == want.size());
        for (size_t i = 0; i < got.size(); i++) {
            CHECK(got[i].name == want[i].name);
            CHECK(got[i].header == want[i].header);
            CHECK(got[i].seq == want[i].seq);
        }
        // the consumer gives up half way: the parser thread must come home
        if (want.size() >= 2) {
            ingest_host::Ingest<MallocMem> in2;
            in2.chunk_bytes = 4096;
            in2.first_cap = 64;
            size_t seen = 0;
            rc = in2.run(paths, [&](ingest_host::Slot &) -> int { return ++seen == want.size() / 2 + 1 ? -7 : 0; });
            CHECK(rc == -7);
        }
    }
    {   // a file that does not exist: the parser's error comes back
        ingest_host::Ingest<MallocMem> in;
        int rc = in.run({dir + "/no_such_file.fa"}, [&](ingest_host::Slot &) -> int { return 0; });
        CHECK(rc == ingest_host::ERR_ARG);
        CHECK(in.err.find("cannot open") != std::string::npos);
    }
    {   // split files as a side effect (60 columns per line)
        const std::string t = ">a first\nACGTACGTAC\nGT\n>b\n" + std::string(130, 'C') + "\n";
        write_file(dir + "/split_in.fa", t);
        ingest_host::Ingest<MallocMem> in;
        in.split_dir = dir;
        int n = 0;
        CHECK(in.run({dir + "/split_in.fa"}, [&](ingest_host::Slot &) -> int { n++; return 0; }) == 0);
        CHECK(n == 2);
        FILE *f = fopen((dir + "/b.fa").c_str(), "rb");
        CHECK(f);
        char buf[512];
        size_t got = fread(buf, 1, sizeof buf, f);
        fclose(f);
        CHECK(std::string(buf, got) == ">b\n" + std::string(60, 'C') + "\n" + std::string(60, 'C') + "\n" + std::string(10, 'C') + "\n");
    }
}


// ---- index blocks, mirror pairing, batch cut (the batch driver of pipeline.hip) ----------------------------------------------
struct PUnit { uint32_t t, q, minus; size_t id; };   // id: position before the cut

// plain restatement: blocks in (target block, query block) order; inside a block the targets ascending, and the units of a
// target in the order they came in
static std::vector<PUnit> blocks_restated(const std::vector<PUnit> &u, const std::vector<uint64_t> &tb, const std::vector<uint64_t> &qb, uint64_t budget,
                                          std::vector<size_t> *block_end, uint64_t *Bt_out, uint64_t *Bq_out) {
    std::set<uint32_t> ts, qs;
    for (auto &x : u) { ts.insert(x.t); qs.insert(x.q); }
    uint64_t need = 0, tmax = 1, qmax = 1;
    for (uint32_t t : ts) { need += tb[t]; tmax = std::max(tmax, tb[t]); }
    for (uint32_t q : qs) { need += qb[q]; qmax = std::max(qmax, qb[q]); }
    *Bt_out = *Bq_out = std::numeric_limits<uint64_t>::max();
    block_end->clear();
    if (need <= budget || u.empty()) { block_end->push_back(u.size()); return u; }
    const uint64_t Bt = std::max<uint64_t>(1, budget / 2 / tmax), Bq = std::max<uint64_t>(1, budget / 2 / qmax);
    *Bt_out = Bt; *Bq_out = Bq;
    const std::vector<uint32_t> tv(ts.begin(), ts.end()), qv(qs.begin(), qs.end());
    std::vector<PUnit> out;
    for (size_t t0 = 0; t0 < tv.size(); t0 += Bt)
        for (size_t q0 = 0; q0 < qv.size(); q0 += Bq) {
            const size_t before = out.size();
            for (size_t ti = t0; ti < std::min<size_t>(tv.size(), t0 + Bt); ti++)
                for (auto &x : u) {
                    if (x.t != tv[ti]) continue;
                    const size_t qi = std::find(qv.begin(), qv.end(), x.q) - qv.begin();
                    if (qi >= q0 && qi < q0 + Bq) out.push_back(x);
                }
            if (out.size() > before) block_end->push_back(out.size());
        }
    return out;
}

static void check_blocks(const std::vector<PUnit> &in, const std::vector<uint64_t> &tb, const std::vector<uint64_t> &qb, uint64_t budget, int expect_cut) {   // expect_cut: 0 one block, 1 more than one, -1 either
    std::vector<PUnit> got = in;
    const std::vector<size_t> ends = host_plan::index_blocks(got, tb, qb, budget);
    std::vector<size_t> want_ends;
    uint64_t Bt, Bq;
    const std::vector<PUnit> want = blocks_restated(in, tb, qb, budget, &want_ends, &Bt, &Bq);
    CHECK(ends == want_ends && got.size() == want.size());
    for (size_t i = 0; i < got.size(); i++) CHECK(got[i].id == want[i].id);
    // the blocks partition the units
    std::vector<char> seen(in.size(), 0);
    for (auto &x : got) { CHECK(!seen[x.id]); seen[x.id] = 1; CHECK(x.t == in[x.id].t && x.q == in[x.id].q && x.minus == in[x.id].minus); }
    CHECK(!ends.empty() && ends.back() == in.size());
    if (expect_cut == 0) { CHECK(ends.size() == 1); for (size_t i = 0; i < got.size(); i++) CHECK(got[i].id == i); }
    if (expect_cut == 1) CHECK(ends.size() > 1);
    size_t b0 = 0;
    for (size_t e : ends) {
        CHECK(e > b0 || in.empty());
        std::set<uint32_t> ts, qs;
        for (size_t i = b0; i < e; i++) {
            ts.insert(got[i].t); qs.insert(got[i].q);
            if (ends.size() > 1 && i > b0) CHECK(got[i - 1].t < got[i].t || (got[i - 1].t == got[i].t && got[i - 1].id < got[i].id));   // target-major, stable
            // the two strands of a pair came in adjacent and stay so
            if (got[i].minus && got[i].id && in[got[i].id - 1].minus == 0 && in[got[i].id - 1].t == got[i].t && in[got[i].id - 1].q == got[i].q)
                CHECK(i > b0 && got[i - 1].id == got[i].id - 1);
        }
        CHECK(ts.size() <= Bt && qs.size() <= Bq);
        b0 = e;
    }
}

// plain restatement of the mirror rule, pair by pair
static host_plan::MirrorPairs mirrors_restated(const std::vector<uint32_t> &pt, const std::vector<uint32_t> &pq, const std::vector<uint8_t> &strands,
                                               const std::vector<char> &plane) {
    const size_t n = pt.size();
    host_plan::MirrorPairs m{std::vector<uint64_t>(n, host_plan::NO_PAIR), std::vector<char>(n, 0)};
    auto eligible = [&](size_t k) { return pt[k] != pq[k] && (strands[k] & 1) && !plane[pt[k]] && !plane[pq[k]]; };
    auto first_of = [&](uint32_t t, uint32_t q) { for (size_t k = 0; k < n; k++) if (eligible(k) && pt[k] == t && pq[k] == q) return (uint64_t)k; return host_plan::NO_PAIR; };
    for (size_t k = 0; k < n; k++) {
        if (!eligible(k) || pt[k] > pq[k] || first_of(pt[k], pq[k]) != k) continue;
        const uint64_t hi = first_of(pq[k], pt[k]);
        if (hi != host_plan::NO_PAIR) { m.mirror_of[k] = hi; m.served[hi] = 1; }
    }
    return m;
}

// the units of the per-pair path as pipeline.hip makes them: target-major, plus strand then minus strand, a served plus
// strand left out
static std::vector<host_plan::BatchUnit> pair_units(const std::vector<uint32_t> &pt, const std::vector<uint32_t> &pq, const std::vector<uint8_t> &strands,
                                                    const host_plan::MirrorPairs &m) {
    std::vector<size_t> ord(pt.size());
    for (size_t k = 0; k < ord.size(); k++) ord[k] = k;
    std::stable_sort(ord.begin(), ord.end(), [&](size_t a, size_t b) { return pt[a] < pt[b]; });
    std::vector<host_plan::BatchUnit> u;
    for (size_t k : ord)
        for (uint32_t minus = 0; minus < 2; minus++) {
            if (!(strands[k] & (1u << minus)) || (!minus && m.served[k])) continue;
            const bool rider = !minus && m.mirror_of[k] != host_plan::NO_PAIR;
            u.push_back(host_plan::BatchUnit{rider ? 2u : 1u, 1.0, rider ? 2u : 1u});
        }
    return u;
}

// all batches of [0, n): checked against a restatement that sums every candidate batch afresh, and against the properties
static size_t check_batches(const std::vector<host_plan::BatchUnit> &u, const host_plan::BatchLimits &lim) {
    std::vector<char> rider;   // per work slot
    std::vector<size_t> slot0;   // first slot of every unit
    for (auto &x : u) { slot0.push_back(rider.size()); rider.push_back(0); if (x.slots == 2) rider.push_back(1); }
    size_t nb = 0, b0 = 0;
    while (b0 < u.size()) {
        const host_plan::Batch b = host_plan::batch_cut(u, b0, u.size(), lim);
        size_t want = b0 + 1;
        for (; want < u.size(); want++) {
            size_t slots = 0; double hits = 0; uint64_t w = 0;
            for (size_t i = b0; i <= want; i++) { slots += u[i].slots; hits += u[i].hits; w += u[i].weight; }
            if (slots > lim.max_units || hits > lim.max_hits || w > lim.max_weight) break;
        }
        CHECK(b.end == want);
        CHECK(b.end > b0 && b.end <= u.size());   // never empty, in order: the batches concatenated are the units
        size_t slots = 0; double hits = 0; uint64_t w = 0;
        for (size_t i = b0; i < b.end; i++) { slots += u[i].slots; hits += u[i].hits; w += u[i].weight; }
        CHECK(b.slots == slots && b.hits == hits);
        if (b.end - b0 > 1) CHECK(slots <= lim.max_units && hits <= lim.max_hits && w <= lim.max_weight);
        CHECK(!rider[slot0[b0]]);   // a rider is never the first slot of a batch ...
        CHECK(b.end == u.size() || !rider[slot0[b.end]]);   // ... it stays with its source
        b0 = b.end;
        nb++;
    }
    return nb;
}

static void test_batch_plan() {
    std::mt19937 rng(4242);
    const uint64_t none = std::numeric_limits<uint64_t>::max();
    for (int round = 0; round < 300; round++) {
        // ---- index blocks: pairs drawn from nt x nq keys (duplicates and holes), one or both strands, adjacent
        const uint32_t nt = 1 + rng() % 9, nq = 1 + rng() % 9, NK = 40;
        std::vector<uint32_t> tkeys, qkeys;
        while (tkeys.size() < nt) { uint32_t v = rng() % NK; if (std::find(tkeys.begin(), tkeys.end(), v) == tkeys.end()) tkeys.push_back(v); }
        while (qkeys.size() < nq) { uint32_t v = rng() % NK; if (std::find(qkeys.begin(), qkeys.end(), v) == qkeys.end()) qkeys.push_back(v); }
        std::vector<uint64_t> tb(NK), qb(NK);
        for (auto &b : tb) b = (rng() % 5 == 0) ? 0 : 50 + rng() % 100;   // 0: an index kept on the genome
        for (auto &b : qb) b = (rng() % 5 == 0) ? 0 : 100 + rng() % 200;
        std::vector<PUnit> units;
        const size_t npairs = rng() % 60;
        for (size_t k = 0; k < npairs; k++) {
            const uint32_t t = tkeys[rng() % nt], q = qkeys[rng() % nq], strands = 1 + rng() % 3;
            for (uint32_t minus = 0; minus < 2; minus++)
                if (strands & (1u << minus)) units.push_back(PUnit{t, q, minus, units.size()});
        }
        uint64_t need = 0;
        std::set<uint32_t> ts, qs;
        for (auto &x : units) { if (ts.insert(x.t).second) need += tb[x.t]; if (qs.insert(x.q).second) need += qb[x.q]; }
        check_blocks(units, tb, qb, need, 0);                    // the need fits: one block, nothing moves
        check_blocks(units, tb, qb, need + rng() % 1000, 0);
        if (need) check_blocks(units, tb, qb, rng() % need, -1);   // (a single target or query whose index alone exceeds its half stays one block)
        // ---- mirror pairing
        const uint32_t S = 1 + rng() % 6;
        std::vector<uint32_t> pt, pq;
        std::vector<uint8_t> strands;
        std::vector<char> plane(S);
        for (auto &f : plane) f = rng() % 5 == 0;
        const size_t n = rng() % 40;
        for (size_t k = 0; k < n; k++) { pt.push_back(rng() % S); pq.push_back(rng() % S); strands.push_back(rng() % 8 ? 3 : rng() % 4); }
        const host_plan::MirrorPairs got = host_plan::mirror_pairs(pt.data(), pq.data(), strands, plane), want = mirrors_restated(pt, pq, strands, plane);
        CHECK(got.mirror_of == want.mirror_of && got.served == want.served);
        size_t nserved = 0, nmirror = 0;
        for (size_t k = 0; k < n; k++) {
            nserved += got.served[k];
            if (got.mirror_of[k] == host_plan::NO_PAIR) continue;
            const uint64_t j = got.mirror_of[k];
            nmirror++;
            CHECK(got.served[j] && pt[k] < pq[k] && pt[j] == pq[k] && pq[j] == pt[k] && (strands[k] & 1) && (strands[j] & 1) && !plane[pt[k]] && !plane[pq[k]]);
            CHECK(!got.served[k] && got.mirror_of[j] == host_plan::NO_PAIR);
        }
        CHECK(nserved == nmirror);
        // ---- batch cut: the units of that pair list, then units with random costs
        std::vector<host_plan::BatchUnit> bu = pair_units(pt, pq, strands, got);
        check_batches(bu, host_plan::BatchLimits{1 + rng() % 8, 1e30, none});
        for (auto &x : bu) { x.hits = (double)(rng() % 1000) * 1e7; x.weight = rng() % 5000; }
        check_batches(bu, host_plan::BatchLimits{1 + rng() % 12, 1.0 + (double)(rng() % 3000) * 1e7, 1 + rng() % 20000});
    }
    {   // pinned: three scaffolds against themselves, both strands: 15 units, 18 work slots, three of them riders
        std::vector<uint32_t> pt, pq;
        for (uint32_t t = 0; t < 3; t++) for (uint32_t q = 0; q < 3; q++) { pt.push_back(t); pq.push_back(q); }
        const std::vector<uint8_t> strands(9, 3);
        const host_plan::MirrorPairs m = host_plan::mirror_pairs(pt.data(), pq.data(), strands, std::vector<char>(3, 0));
        const std::vector<host_plan::BatchUnit> u = pair_units(pt, pq, strands, m);
        size_t slots = 0, riders = 0;
        for (auto &x : u) { slots += x.slots; riders += x.slots == 2; }
        CHECK(u.size() == 15 && slots == 18 && riders == 3);
        CHECK(check_batches(u, host_plan::BatchLimits{1, 2.5e10, none}) == 15);
        CHECK(check_batches(u, host_plan::BatchLimits{5, 2.5e10, none}) == 4);
        CHECK(check_batches(u, host_plan::BatchLimits{8192, 2.5e10, none}) == 1);
    }
    {   // pinned: 24 x 24 targets x queries, both strands, a budget one byte short of the need: more than one block
        std::vector<PUnit> units;
        for (uint32_t t = 0; t < 24; t++) for (uint32_t q = 0; q < 24; q++) for (uint32_t minus = 0; minus < 2; minus++) units.push_back(PUnit{t, q, minus, units.size()});
        const std::vector<uint64_t> tb(24, 1000), qb(24, 2000);
        check_blocks(units, tb, qb, 24 * 3000, 0);
        check_blocks(units, tb, qb, 24 * 3000 - 1, 1);
    }
}

static void test_plan() {
    test_batch_plan();
    std::mt19937 rng(99);
    for (int round = 0; round < 200; round++) {
        const size_t n = 1 + rng() % 300;
        std::vector<uint64_t> len(n);
        for (auto &l : len) l = (rng() % 10 == 0) ? 0 : (rng() % 7 == 0 ? 3000000 + rng() % 1000000 : 1 + rng() % 200000);
        std::vector<uint32_t> ids;
        for (uint32_t i = 0; i < n; i++) if (rng() % 4) ids.push_back(i);
        const uint32_t spacer = 42 + rng() % 400;
        const uint64_t member_max = 2u << 20, super_len = 100000 + rng() % 8000000;
        auto plan = host_plan::plan_supers(len, ids, spacer, member_max, super_len);
        std::vector<uint32_t> seen;
        for (auto &mem : plan) {
            CHECK(!mem.empty());
            for (size_t i = 0; i < mem.size(); i++) {
                seen.push_back(mem[i].id);
                CHECK(mem[i].len == len[mem[i].id]);
                CHECK(mem[i].start % 32 == 0);
                if (i) CHECK((uint64_t)mem[i].start >= (uint64_t)mem[i - 1].start + mem[i - 1].len + spacer);
                if (mem.size() > 1) { CHECK(mem[i].len <= member_max && mem[i].len > 0); CHECK((uint64_t)mem[i].start + mem[i].len <= super_len || i == 0); }
            }
            CHECK(mem[0].start == 0);
        }
        for (auto &mem : plan) for (size_t i = 1; i < mem.size(); i++) CHECK(mem[i].id > mem[i - 1].id);   // members in scaffold order
        std::sort(seen.begin(), seen.end());
        CHECK(seen == ids);   // every scaffold once
    }
    // cross product
    for (int round = 0; round < 100; round++) {
        const size_t nt = 1 + rng() % 12, nq = 1 + rng() % 12, NA = 40, NQ = 50;
        std::vector<uint32_t> ts, qs;
        while (ts.size() < nt) { uint32_t v = rng() % NA; if (std::find(ts.begin(), ts.end(), v) == ts.end()) ts.push_back(v); }
        while (qs.size() < nq) { uint32_t v = rng() % NQ; if (std::find(qs.begin(), qs.end(), v) == qs.end()) qs.push_back(v); }
        std::vector<uint32_t> pt, pq;
        for (uint32_t t : ts) for (uint32_t q : qs) { pt.push_back(t); pq.push_back(q); }
        std::shuffle(pt.begin(), pt.end(), std::mt19937(round));
        std::shuffle(pq.begin(), pq.end(), std::mt19937(round));   // the same permutation: pairs stay pairs
        auto c = host_plan::cross_product(pt.data(), pq.data(), pt.size(), NA, NQ);
        CHECK(c.full && c.distinct == nt * nq && c.dups.empty());
        for (size_t k = 0; k < pt.size(); k++) CHECK(c.pairidx[(size_t)c.trank[pt[k]] * c.qset.size() + c.qrank[pq[k]]] == k);
        pt.push_back(pt[0]); pq.push_back(pq[0]);   // a duplicate
        c = host_plan::cross_product(pt.data(), pq.data(), pt.size(), NA, NQ);
        CHECK(c.full && c.dups.size() == 1 && c.dups[0].first == pt.size() - 1 && c.dups[0].second == 0);
        if (nt > 1 && nq > 1) {   // one cell missing
            pt.pop_back(); pq.pop_back(); pt.pop_back(); pq.pop_back();
            c = host_plan::cross_product(pt.data(), pq.data(), pt.size(), NA, NQ);
            CHECK(!c.full);
        }
    }
}

int main(int argc, char **argv) {
    CHECK(argc == 2);
    test_plan();
    test_ingest(argv[1]);
    printf("host_sanitize: ok\n");
    return 0;
}
