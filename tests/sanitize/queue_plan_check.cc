// The sizing policy of the extension batch (mimeo_amd/csrc/queue_plan.h) against a frozen restatement of the arithmetic that
// ExtBatch::start, ::finish, ::arena_bytes, ::queue_bytes, queue_budget, ext_batch_max_units and the two arena-growth blocks
// of k4_extend.hip held before the policy had a header of its own (namespace frozen: the expressions as they stood there,
// members as locals; it is the reference and is not to be tidied).  Every value is compared for exact equality (boosts bit
// for bit) over seeded random inputs and the edges named in main(); then the properties that nothing else checks: a batch
// never carves past what it declared, slices are aligned and disjoint, growth makes room for what the counters reported,
// boosts only rise and stop at 4096, and ext_batch_max_units agrees with the key-bits test of start().
// Built and run by tests/test_host_queue_plan.py, plain and with -fsanitize=address,undefined.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>

#include "../../mimeo_amd/csrc/queue_plan.h"

namespace qp = mimeo::queue_plan;

#define CHECK(c) do { if (!(c)) { fprintf(stderr, "queue_plan_check: %s failed at line %d (case %llu)\n", #c, __LINE__, (unsigned long long)g_case); exit(1); } } while (0)
static uint64_t g_case = 0;

namespace frozen {
constexpr int SEED_LEN = 19;
constexpr uint64_t SIZEOF_CAND = 20, SIZEOF_HSP = 32;   // sizeof(Cand), sizeof(mimeo_hsp)

static uint32_t bits_for(uint64_t v) {  // bits needed to hold values 0 .. v
    uint32_t b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}
uint32_t ext_batch_max_units(uint64_t max_tlen, uint64_t max_qlen) {
    const uint32_t ebits = bits_for(max_tlen + SEED_LEN), dbits = bits_for(max_tlen + max_qlen + SEED_LEN);
    const uint32_t ubits = 64 - std::min(63u, ebits + dbits);
    return ubits >= 20 ? (1u << 20) : (1u << ubits);
}

struct Batch {
    double boost_f = 1.0, boost_m = 1.0, boost_l = 1.0, boost_c = 1.0, boost_w = 1.0;
    uint64_t cap_f_ = 0, cap_m_ = 0, cap_l_ = 0, cap_c_ = 0, walk_entries_ = 0;
    std::vector<uint64_t> walk_cap_u_;
    double shrink_ = 1.0;
    uint32_t ebits_ = 0, dbits_ = 0, key_bits_ = 0;
    bool v1_ = false, mirror_ = false, splittable_ = false;

    bool key_bits(uint64_t max_t, uint64_t max_q, uint32_t nunits) {   // false: "batch too large for the follower key"
        ebits_ = bits_for(max_t + SEED_LEN);
        dbits_ = bits_for(max_t + max_q + SEED_LEN);
        if (ebits_ + dbits_ > 63 || (nunits > 1 && bits_for(nunits - 1) + ebits_ + dbits_ > 64)) return false;
        key_bits_ = std::min(64u, ebits_ + dbits_ + (nunits > 1 ? bits_for(nunits - 1) : 0));
        return true;
    }
    // unit_hits[u]: expected_seed_hits of unit u, 0 for a unit without indexes (a mirror rider)
    void start(const std::vector<double> &unit_hits, double shrink) {
        double expect_hits = 0;
        for (double e : unit_hits) expect_hits += e;
        shrink_ = shrink > 0 ? shrink : 1.0;
        cap_f_ = (uint64_t)(expect_hits * 0.02 / 8 * 1.5 * boost_f / shrink) + (uint64_t)(1048576 / shrink) + 64;
        cap_m_ = (uint64_t)(expect_hits * 0.03 / 8 * 1.5 * boost_m / shrink) + (uint64_t)(1048576 / shrink) + 64;
        cap_l_ = (uint64_t)(expect_hits * 0.002 * boost_l / shrink) + (uint64_t)(1048576 / shrink) + 64;
        cap_c_ = (uint64_t)(expect_hits * 0.002 * boost_c / shrink) + (uint64_t)(1048576 / shrink) + 64;
        walk_entries_ = 0;
        walk_cap_u_.assign(unit_hits.size(), 0);
        for (size_t u = 0; u < unit_hits.size(); u++) {
            if (unit_hits[u] == 0) continue;
            const double e = unit_hits[u];
            walk_cap_u_[u] = (uint64_t)(e * 0.08 / 8 * 1.5 * boost_w / shrink) + (uint64_t)(16384 / shrink) + 64;
            walk_entries_ += 8 * walk_cap_u_[u];
        }
    }
    uint64_t arena_bytes() const {
        const uint64_t mf = !mirror_ ? 1 : 2;
        return cap_f_ * 8 * 12 + cap_m_ * 8 * 20 + cap_l_ * 12 + cap_c_ * (SIZEOF_CAND + mf * (SIZEOF_HSP + 4)) + (v1_ ? 8 : walk_entries_ * 8) + 4096;
    }
    uint64_t queue_bytes() const {
        const uint64_t mf = !mirror_ ? 1 : 2;
        return arena_bytes() + cap_f_ * 8 * 41 + cap_c_ * mf * 260;
    }
    void slices(size_t (&sz_out)[10]) const {   // the sz[10] table of enqueue_heavy
        const uint64_t cap_f = cap_f_, cap_m = cap_m_, cap_l = cap_l_, cap_c = cap_c_;
        const bool v1 = v1_;
        const size_t mf = !mirror_ ? 1 : 2;
        const size_t sz[10] = {cap_f * 8 * 8, cap_f * 8 * 4, cap_m * 8 * 16, cap_m * 8 * 4, cap_l * 8, cap_l * 4, cap_c * SIZEOF_CAND,
                               cap_c * SIZEOF_HSP * mf, cap_c * 4 * mf, v1 ? 8 : walk_entries_ * 8 + 8};
        for (int i = 0; i < 10; i++) sz_out[i] = sz[i];
    }
    // the growth block of enqueue_heavy: what arena_q.reserve is first asked for
    size_t want_queue_arena(size_t arena_q_cap, size_t free_b) const {
        size_t sz[10];
        slices(sz);
        size_t total = 0;
        for (size_t z : sz) total += (z + 255) & ~(size_t)255;
        const size_t have = free_b + arena_q_cap;
        size_t want = arena_q_cap ? total + total / 2 : total;
        if (want + (queue_bytes() - arena_bytes()) + (8ull << 30) > have) want = total;
        return want;
    }
    // the overflow branch of finish(): growth, then learning
    void overflow(uint64_t maxf, uint64_t maxm, uint64_t nlong, uint64_t ncand, uint64_t nwalk_total, uint64_t nwalk_over, double expect_hits) {
        uint64_t &cap_f = cap_f_, &cap_m = cap_m_, &cap_l = cap_l_, &cap_c = cap_c_;
        cap_f = std::max<uint64_t>(cap_f, maxf + maxf / 2 + 1024);
        cap_m = std::max<uint64_t>(cap_m, maxm + maxm / 2 + 1024);
        cap_l = std::max<uint64_t>(cap_l, nlong + nlong / 2 + 1024);
        cap_c = std::max<uint64_t>(cap_c, 2 * ncand + 65536);
        if (nwalk_over > 1024) {
            const double grow = 1.25 * (double)nwalk_over / 1024.0;
            walk_entries_ = 0;
            for (auto &w : walk_cap_u_) { if (w) w = (uint64_t)((double)w * grow) + 1024; walk_entries_ += 8 * w; }
        }
        if (expect_hits > 1e6) {
            boost_f = std::min(4096.0, std::max(boost_f, 1.5 * (double)(8 * maxf) / (0.02 * expect_hits)));
            boost_m = std::min(4096.0, std::max(boost_m, 1.5 * (double)(8 * maxm) / (0.03 * expect_hits)));
            boost_l = std::min(4096.0, std::max(boost_l, 1.5 * (double)nlong / (0.002 * expect_hits)));
            boost_c = std::min(4096.0, std::max(boost_c, 1.5 * (double)ncand / (0.002 * expect_hits)));
            boost_w = std::min(4096.0, std::max(boost_w, 1.5 * (double)nwalk_total / (0.08 * expect_hits)));
            boost_w = std::min(4096.0, std::max(boost_w, 1.5 * boost_w * ((double)nwalk_over / 1024.0) / shrink_));
        }
    }
    // the end of finish()
    void learn_at_end(uint64_t nf_total, uint64_t nm_total, uint64_t nlong, uint64_t ncand, uint64_t nwalk_total, uint64_t nwalk_over, double expect_hits) {
        if (expect_hits > 1e6) {
            const double e = expect_hits;
            boost_f = std::min(4096.0, std::max(boost_f, 1.5 * (double)nf_total / (0.02 * e)));
            boost_m = std::min(4096.0, std::max(boost_m, 1.5 * (double)nm_total / (0.03 * e)));
            boost_l = std::min(4096.0, std::max(boost_l, 1.5 * (double)nlong / (0.002 * e)));
            boost_c = std::min(4096.0, std::max(boost_c, 1.5 * (double)ncand / (0.002 * e)));
            boost_w = std::min(4096.0, std::max(boost_w, 1.5 * (double)nwalk_total / (0.08 * e)));
            boost_w = std::min(4096.0, std::max(boost_w, 1.5 * boost_w * ((double)nwalk_over / 1024.0) / shrink_));
        }
    }
    bool split(uint64_t budget) const { return splittable_ && queue_bytes() > budget; }
};
// queue_budget(); budget_mb: the text of MIMEO_QUEUE_BUDGET_MB, or null
uint64_t queue_budget(size_t free_b, uint64_t held_bytes, const char *budget_mb) {
    uint64_t budget;
    const uint64_t have = (uint64_t)free_b + held_bytes, reserve = std::min<uint64_t>(have / 8, 8ull << 30);
    budget = have - reserve;
    if (budget_mb) budget = (uint64_t)atol(budget_mb) << 20;
    return budget;
}
// the growth block of the sort arena in finish(): what arena_s.reserve is first asked for; tmp: max(t1, t2)
size_t want_sort_arena(uint64_t nf, size_t tmp, size_t arena_s_cap, size_t free_b, size_t *total_out) {
    const size_t sz[6] = {nf * 8, nf * 4, nf, nf * 8, nf * 8, tmp + 16};
    size_t total = 0;
    for (size_t z : sz) total += (z + 255) & ~(size_t)255;
    size_t want = arena_s_cap ? total + total / 2 : total + total / 8;
    if (want + (4ull << 30) > free_b + arena_s_cap) want = total;
    *total_out = total;
    return want;
}
}  // namespace frozen

static bool same_bits(double a, double b) { return !memcmp(&a, &b, sizeof a); }

struct Case {
    std::vector<double> unit_hits;   // expected seed hits per unit; 0: a mirror rider
    double boost[5];
    double shrink;
    bool mirror, v1;
    uint64_t maxf, maxm, nf_total, nm_total, nlong, ncand, nwalk_total, nwalk_over;
    uint64_t free_b, held_q, held_s;
    const char *budget_mb;
    uint64_t nf_sort, tmp_sort;
};

static void run_case(const Case &k) {
    g_case++;
    frozen::Batch f;
    f.boost_f = k.boost[0]; f.boost_m = k.boost[1]; f.boost_l = k.boost[2]; f.boost_c = k.boost[3]; f.boost_w = k.boost[4];
    f.mirror_ = k.mirror; f.v1_ = k.v1;
    qp::Boosts b{k.boost[0], k.boost[1], k.boost[2], k.boost[3], k.boost[4]};
    // ---- start(): capacities, walk queue, what the batch declares, the split before allocation
    double expect = 0;
    uint32_t launching = 0;
    std::vector<uint64_t> walk(k.unit_hits.size(), 0);
    for (size_t u = 0; u < k.unit_hits.size(); u++) {
        if (k.unit_hits[u] == 0) continue;
        expect += k.unit_hits[u];
        walk[u] = qp::walk_cap(k.unit_hits[u], b, k.shrink);
        launching++;
    }
    f.splittable_ = launching > 1;
    f.start(k.unit_hits, k.shrink);
    qp::Caps c = qp::initial_caps(expect, b, k.shrink);
    uint64_t entries = qp::walk_entries(walk);
    auto same_state = [&]() {
        CHECK(c.f == f.cap_f_ && c.m == f.cap_m_ && c.l == f.cap_l_ && c.c == f.cap_c_);
        CHECK(walk == f.walk_cap_u_ && entries == f.walk_entries_);
        CHECK(qp::arena_bytes(c, entries, k.mirror, k.v1) == f.arena_bytes());
        CHECK(qp::queue_bytes(c, entries, k.mirror, k.v1) == f.queue_bytes());
        CHECK(same_bits(b.f, f.boost_f) && same_bits(b.m, f.boost_m) && same_bits(b.l, f.boost_l) && same_bits(b.c, f.boost_c) && same_bits(b.w, f.boost_w));
    };
    auto same_layout = [&]() {
        const qp::QueueSizes z = qp::queue_slices(c, entries, k.mirror, k.v1);
        size_t sz[10];
        f.slices(sz);
        static_assert(qp::Q_SLICES == 10, "the frozen table has ten slices");
        // the order in which enqueue_heavy carved them: fkey, fprev, medq, medu, longq, longu, cand, hsps, hsp_unit, walkq
        const int order[10] = {qp::Q_FKEY, qp::Q_FPREV, qp::Q_MEDQ, qp::Q_MEDU, qp::Q_LONGQ, qp::Q_LONGU, qp::Q_CAND, qp::Q_HSPS, qp::Q_HSP_UNIT, qp::Q_WALKQ};
        for (int i = 0; i < 10; i++) CHECK(order[i] == i && z.bytes[i] == sz[i]);
        uint64_t off[qp::Q_SLICES];
        const uint64_t total = qp::place_slices(z.bytes, off);
        // declared >= carved; aligned; disjoint and in order
        CHECK(qp::arena_bytes(c, entries, k.mirror, k.v1) >= total);
        for (int i = 0; i < qp::Q_SLICES; i++) {
            CHECK(off[i] % 256 == 0);
            CHECK(off[i] + z.bytes[i] <= (i + 1 < qp::Q_SLICES ? off[i + 1] : total));
        }
        for (uint64_t held : {(uint64_t)0, k.held_q}) {
            const uint64_t want = qp::arena_want(total, held, k.free_b, qp::queue_bytes(c, entries, k.mirror, k.v1) - qp::arena_bytes(c, entries, k.mirror, k.v1) + qp::QUEUE_ARENA_HEADROOM, 0);
            CHECK(want == f.want_queue_arena(held, k.free_b));
            CHECK(want >= total);
        }
    };
    same_state();
    same_layout();
    const uint64_t budget = qp::queue_budget(k.free_b, k.held_q + k.held_s, k.budget_mb != nullptr, k.budget_mb ? atol(k.budget_mb) : 0);
    CHECK(budget == frozen::queue_budget(k.free_b, k.held_q + k.held_s, k.budget_mb));
    if (!k.budget_mb) CHECK(budget <= k.free_b + k.held_q + k.held_s && k.free_b + k.held_q + k.held_s - budget <= 8 * qp::GiB);
    CHECK(qp::must_split(f.splittable_, qp::queue_bytes(c, entries, k.mirror, k.v1), budget) == f.split(budget));
    if (launching <= 1) CHECK(!qp::must_split(launching > 1, ~0ull, 0));   // one launching unit is tried whatever it asks for
    // ---- the overflow branch of finish(): growth, learning, the split after overflow
    const qp::Boosts before = b;
    const qp::Counts fullest{k.maxf, k.maxm, k.nlong, k.ncand, k.nwalk_total, k.nwalk_over};
    const bool was_over = qp::over(c, fullest);
    CHECK(was_over == (k.maxf > f.cap_f_ || k.maxm > f.cap_m_ || k.nlong > f.cap_l_ || k.ncand > f.cap_c_ || k.nwalk_over > 1024));
    const std::vector<uint64_t> walk_before = walk;
    qp::grow(c, walk, fullest);
    entries = qp::walk_entries(walk);
    qp::Counts batch = fullest;
    batch.followers *= 8; batch.generic *= 8;
    qp::learn(b, batch, expect, k.shrink);
    f.overflow(k.maxf, k.maxm, k.nlong, k.ncand, k.nwalk_total, k.nwalk_over, expect);
    same_state();
    same_layout();
    CHECK(qp::must_split(f.splittable_, qp::queue_bytes(c, entries, k.mirror, k.v1), budget) == f.split(budget));
    // room for everything the counters reported
    CHECK(c.f > k.maxf && c.m > k.maxm && c.l > k.nlong && c.c > k.ncand);
    for (size_t u = 0; u < walk.size(); u++) {
        CHECK((walk[u] == 0) == (walk_before[u] == 0) && walk[u] >= walk_before[u]);
        // the fullest shard held nwalk_over / 1024 of its capacity
        if (walk[u] && k.nwalk_over > 1024) CHECK((long double)walk[u] * 1024 > (long double)walk_before[u] * k.nwalk_over);
    }
    qp::Counts again = fullest;
    again.nwalk_over = 0;   // (the walk queue's fullness is relative to the capacity it had)
    CHECK(!qp::over(c, again));
    // ---- the end of finish()
    qp::learn(b, qp::Counts{k.nf_total, k.nm_total, k.nlong, k.ncand, k.nwalk_total, k.nwalk_over}, expect, k.shrink);
    f.learn_at_end(k.nf_total, k.nm_total, k.nlong, k.ncand, k.nwalk_total, k.nwalk_over, expect);
    same_state();
    const double was[5] = {before.f, before.m, before.l, before.c, before.w}, now[5] = {b.f, b.m, b.l, b.c, b.w};
    for (int i = 0; i < 5; i++) CHECK(now[i] >= was[i] && now[i] <= 4096.0);
    if (!(expect > 1e6)) for (int i = 0; i < 5; i++) CHECK(same_bits(now[i], was[i]));   // below the threshold nothing is learned
    // ---- the sort arena
    const qp::SortSizes s = qp::sort_slices(k.nf_sort, k.tmp_sort);
    uint64_t soff[qp::S_SLICES];
    const uint64_t stotal = qp::place_slices(s.bytes, soff);
    for (uint64_t held : {(uint64_t)0, k.held_s}) {
        size_t ftotal = 0;
        const size_t fwant = frozen::want_sort_arena(k.nf_sort, k.tmp_sort, held, k.free_b, &ftotal);
        CHECK(stotal == ftotal);
        CHECK(qp::arena_want(stotal, held, k.free_b, qp::SORT_ARENA_HEADROOM, stotal / 8) == fwant && fwant >= stotal);
    }
    for (int i = 0; i < qp::S_SLICES; i++) CHECK(soff[i] % 256 == 0 && soff[i] + s.bytes[i] <= (i + 1 < qp::S_SLICES ? soff[i + 1] : stotal));
    CHECK(s.bytes[qp::S_FKEY2] == k.nf_sort * 8 && s.bytes[qp::S_FPREV2] == k.nf_sort * 4 && s.bytes[qp::S_FLAGS] == k.nf_sort &&
          s.bytes[qp::S_SEGS] == k.nf_sort * 8 && s.bytes[qp::S_BIGSEG] == k.nf_sort * 8 && s.bytes[qp::S_TMP] == k.tmp_sort + 16);
}

static void key_case(uint64_t max_t, uint64_t max_q, uint32_t nunits) {
    g_case++;
    frozen::Batch f;
    const bool fits = f.key_bits(max_t, max_q, nunits);
    const qp::KeyBits k = qp::follower_key_bits(max_t, max_q, nunits, frozen::SEED_LEN);
    CHECK(k.fits == fits && k.ebits == f.ebits_ && k.dbits == f.dbits_);
    if (fits) CHECK(k.key_bits == f.key_bits_ && k.key_bits <= 64);
    const uint32_t most = qp::max_units(max_t, max_q, frozen::SEED_LEN);
    CHECK(most == frozen::ext_batch_max_units(max_t, max_q));
    if (k.ebits + k.dbits <= 63) {   // what the pipeline cuts batches by is what start() accepts
        CHECK(most >= 2 && most <= (1u << 20));
        CHECK(qp::follower_key_bits(max_t, max_q, 1, frozen::SEED_LEN).fits && qp::follower_key_bits(max_t, max_q, most, frozen::SEED_LEN).fits);
        if (nunits <= most) CHECK(fits);
        if (most < (1u << 20)) CHECK(!qp::follower_key_bits(max_t, max_q, most + 1, frozen::SEED_LEN).fits);
    } else
        CHECK(!fits);
}

int main() {
    std::mt19937_64 rng(20240607);
    auto uniform = [&](uint64_t lo, uint64_t hi) { return std::uniform_int_distribution<uint64_t>(lo, hi)(rng); };
    auto log_uniform = [&](double lo, double hi) { return lo * std::exp(std::uniform_real_distribution<double>(0.0, std::log(hi / lo))(rng)); };
    auto counter = [&]() -> uint64_t { return uniform(0, 3) ? uniform(0, 1ull << uniform(0, 40)) : 0; };   // 0 .. 2^40, every magnitude
    auto hits = [&]() -> double {   // 0 .. 1e12, every magnitude, and the learning threshold from both sides
        switch (uniform(0, 7)) {
            case 0: return 0.0;
            case 1: return std::nextafter(1e6, uniform(0, 1) ? 0.0 : 2e6);
            case 2: return 1e6;
            default: return log_uniform(1.0, 1e12);
        }
    };
    const double shrinks[3] = {1.0, 3000.0, 4000.0};
    const char *budgets[4] = {nullptr, nullptr, "3072", "0"};
    auto random_case = [&]() {
        Case k;
        const uint64_t nunits = uniform(1, 6);
        double left = hits();   // the batch's expected hits, spread over its units; a unit may be a rider
        for (uint64_t u = 0; u < nunits; u++) {
            const double e = u + 1 == nunits ? left : (uniform(0, 3) ? left * std::uniform_real_distribution<double>(0.0, 1.0)(rng) : 0.0);
            k.unit_hits.push_back(e);
            left = std::max(0.0, left - e);
        }
        for (double &b : k.boost) b = uniform(0, 3) ? log_uniform(1.0, 4096.0) : (uniform(0, 1) ? 1.0 : 4096.0);
        k.shrink = shrinks[uniform(0, 2)];
        k.mirror = uniform(0, 1); k.v1 = uniform(0, 1);
        k.maxf = counter(); k.maxm = counter(); k.nlong = counter(); k.ncand = counter(); k.nwalk_total = counter();
        k.nf_total = counter(); k.nm_total = counter();
        k.nwalk_over = uniform(0, 2) ? uniform(0, 4096) : uniform(1020, 1028);   // the walk queue's fullest shard: both sides of 1024, and the edge
        k.free_b = uniform(0, 3) ? uniform(0, 288 * qp::GiB) : 0;
        k.held_q = uniform(0, 1) ? uniform(0, 288 * qp::GiB) : 0;
        k.held_s = uniform(0, 1) ? uniform(0, 288 * qp::GiB - k.held_q) : 0;
        k.budget_mb = budgets[uniform(0, 3)];
        k.nf_sort = counter() + 1;
        k.tmp_sort = counter();
        return k;
    };
    for (int i = 0; i < 200000; i++) run_case(random_case());
    // ---- edges by hand
    Case k = random_case();
    k.unit_hits = {0.0, 0.0};   // mirror riders only: nothing expected, nothing learned, the floors alone
    run_case(k);
    for (double e : {std::nextafter(1e6, 0.0), 1e6, std::nextafter(1e6, 2e6), 0.0, 1e12}) {
        k = random_case();
        k.unit_hits = {e};   // one unit: never split
        k.maxf = 1ull << 40; k.ncand = 1ull << 40; k.nwalk_over = 1025;
        run_case(k);
        k.unit_hits = {e / 2, 0.0, e / 2};
        k.nwalk_over = 1024;
        run_case(k);
    }
    {
        const qp::Caps c = qp::initial_caps(0.0, qp::Boosts(), 1.0);
        CHECK(c.f == 1048576 + 64 && c.m == c.f && c.l == c.f && c.c == c.f);
        qp::Boosts b;
        qp::learn(b, qp::Counts{1ull << 40, 1ull << 40, 1ull << 40, 1ull << 40, 1ull << 40, 4096}, 1e6, 1.0);
        CHECK(b.f == 1.0 && b.w == 1.0);   // 1e6 itself is below the threshold
        qp::learn(b, qp::Counts{1ull << 40, 1ull << 40, 1ull << 40, 1ull << 40, 1ull << 40, 4096}, std::nextafter(1e6, 2e6), 1.0);
        CHECK(b.f == 4096.0 && b.m == 4096.0 && b.l == 4096.0 && b.c == 4096.0 && b.w == 4096.0);
    }
    // ---- the follower key: random lengths up to 2^31 - 257 and batches of 1 .. 2^20 units, then ebits + dbits of 62, 63 and 64
    for (int i = 0; i < 100000; i++) {
        const uint64_t max_t = uniform(0, 1) ? uniform(0, 0x7FFFFEFFull) : uniform(0, 1ull << uniform(0, 31)) % 0x7FFFFF00ull;
        const uint64_t max_q = uniform(0, 1) ? uniform(0, 0x7FFFFEFFull) : uniform(0, 1ull << uniform(0, 31)) % 0x7FFFFF00ull;
        key_case(max_t, max_q, (uint32_t)(uniform(0, 1) ? uniform(1, 1u << 20) : uniform(1, 1ull << uniform(0, 20))));
    }
    const uint64_t t30 = 1ull << 30, t31 = 1ull << 31;
    for (uint32_t n : {1u, 2u, 3u, 4u, 5u, 1u << 20}) {
        key_case(t30, 0, n);          // 31 + 31 = 62: four units
        key_case(t30, t30, n);        // 31 + 32 = 63: two units
        key_case(0x7FFFFEFFull, 0x7FFFFEFFull, n);   // the longest scaffolds start() admits: 31 + 32
        key_case(t31, 0, n);          // 32 + 32 = 64: no batch fits, not even one unit
    }
    CHECK(qp::follower_key_bits(t30, 0, 1, 19).ebits + qp::follower_key_bits(t30, 0, 1, 19).dbits == 62 && qp::max_units(t30, 0, 19) == 4);
    CHECK(qp::follower_key_bits(t30, t30, 1, 19).ebits + qp::follower_key_bits(t30, t30, 1, 19).dbits == 63 && qp::max_units(t30, t30, 19) == 2);
    CHECK(qp::follower_key_bits(t31, 0, 1, 19).ebits + qp::follower_key_bits(t31, 0, 1, 19).dbits == 64 && !qp::follower_key_bits(t31, 0, 1, 19).fits);
    printf("queue_plan_check: ok (%llu cases)\n", (unsigned long long)g_case);
    return 0;
}
