// The care-position count of the seed filters (mimeo_amd/csrc/seed_window.h: a carry-save network of three-input boolean
// functions) held to the loop it replaced — a serial ones / twos counter over the shifted words, kept here verbatim — on the
// host's instantiation of the header: the truth tables, the grouping and the shift directions are the ones the kernels compile.
//   g++ -std=c++17 -O2 [-fsanitize=address,undefined] tests/sanitize/seed_window_check.cc -o seed_window_check && ./seed_window_check
// Instantiations: the three the kernels use (CARE10 without the transversion plane from frame bit 13: K34's pre-filter; CARE19
// with it from bit 13: the sharp filter at the flush; CARE19 with it from bit 0: the walk kernel's left_masks / filter_left) and
// filter_left's eight high care positions, each in both `transitions` modes.
// Inputs: all-zero and all-ones words; every single set bit of the 64 columns; every pair of set bits at most 19 columns apart
// (across the n0 / n1 word boundary too), in the mismatch plane alone and with each of the two also in the transversion plane;
// 10^6 random word pairs at five bit densities.
#include <cstdint>
#include <cstdio>
#include <cstdlib>

#include "../../mimeo_amd/csrc/seed_window.h"

namespace {

constexpr uint32_t CARE19 = 0x7A997u, CARE10 = 0x1A997u, CARE8_HIGH = 0x7A980u;
constexpr int SEED_LEN = 19;

uint32_t alignbit(uint32_t hi, uint32_t lo, uint32_t sh) { return (uint32_t)((((uint64_t)hi << 32) | lo) >> (sh & 31u)); }

// the loop of seed_starts32 / left_masks / filter_left before the header (BASE = 13 / 0)
template <uint32_t CARE, bool TV, int BASE>
uint32_t old_starts32(uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, int transitions) {
    uint32_t ones = 0, twos = 0, tv = 0;
    for (int c = 0; c < SEED_LEN; c++) {
        if (!((CARE >> c) & 1u)) continue;
        const uint32_t v = alignbit(n1, n0, BASE + c);
        twos |= ones & v;
        ones |= v;
        if (TV) tv |= alignbit(d1, d0, BASE + c);
    }
    return ~(transitions ? (twos | tv) : ones);
}

// the rule itself, one window at a time
template <uint32_t CARE, bool TV, int BASE>
uint32_t plain_starts32(uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, int transitions) {
    const uint64_t n = ((uint64_t)n1 << 32) | n0, d = ((uint64_t)d1 << 32) | d0;
    uint32_t r = 0;
    for (int i = 0; i < 32; i++) {
        int nm = 0, nv = 0;
        for (int c = 0; c < SEED_LEN; c++) {
            if (!((CARE >> c) & 1u)) continue;
            nm += (int)((n >> (BASE + i + c)) & 1u);
            nv += (int)((d >> (BASE + i + c)) & 1u);
        }
        const bool ok = transitions ? (nm <= 1 && (!TV || nv == 0)) : nm == 0;
        r |= (uint32_t)ok << i;
    }
    return r;
}

unsigned long long g_checked = 0;
int g_bad = 0;

template <uint32_t CARE, bool TV, int BASE>
void check(const char *name, uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, bool plain) {
    using namespace mimeo::seed_window;
    for (int transitions = 0; transitions < 2; transitions++) {
        const uint32_t exp = old_starts32<CARE, TV, BASE>(n0, n1, d0, d1, transitions);
        const uint32_t got = starts32<HostOps, CARE, TV, BASE>(n0, n1, d0, d1, transitions);
        g_checked++;
        if (got != exp || (plain && plain_starts32<CARE, TV, BASE>(n0, n1, d0, d1, transitions) != exp)) {
            if (g_bad++ < 10)
                std::printf("MISMATCH %s transitions=%d n=%08x:%08x d=%08x:%08x old=%08x new=%08x\n", name, transitions, n1, n0, d1, d0, exp, got);
        }
    }
}

// d is a subset of n in the kernels (n = dl | dh, d = dl); the header does not rely on it, so the random part also feeds
// independent planes
void check_all(uint32_t n0, uint32_t n1, uint32_t d0, uint32_t d1, bool plain) {
    check<CARE10, false, 13>("CARE10/13", n0, n1, 0u, 0u, plain);
    check<CARE19, true, 13>("CARE19+tv/13", n0, n1, d0, d1, plain);
    check<CARE19, true, 0>("CARE19+tv/0", n0, n1, d0, d1, plain);
    check<CARE8_HIGH, true, 0>("CARE8_HIGH+tv/0", n0, n1, d0, d1, plain);
}

uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint64_t next64() {   // xorshift64*
    g_rng ^= g_rng >> 12; g_rng ^= g_rng << 25; g_rng ^= g_rng >> 27;
    return g_rng * 0x2545F4914F6CDD1Dull;
}
// a word whose bits are set with probability 2^-k
uint64_t sparse64(int k) {
    uint64_t w = next64();
    for (int j = 1; j < k; j++) w &= next64();
    return w;
}

}  // namespace

int main() {
    // the host's primitives against their definitions
    {
        using namespace mimeo::seed_window;
        for (int j = 0; j < 2000; j++) {
            const uint32_t a = (uint32_t)next64(), b = (uint32_t)next64(), c = (uint32_t)next64();
            if (HostOps::bitop3<TT_XOR3>(a, b, c) != (a ^ b ^ c) || HostOps::bitop3<TT_MAJ3>(a, b, c) != ((a & b) | (a & c) | (b & c)) ||
                HostOps::bitop3<TT_OR3>(a, b, c) != (a | b | c) || HostOps::bitop3<TT_A_OR_BC>(a, b, c) != (a | (b & c)) ||
                HostOps::funnel(a, b, j & 31) != alignbit(b, a, j & 31)) {
                std::printf("seed_window_check: a primitive of HostOps is wrong\n");
                return 1;
            }
        }
    }
    const uint64_t one = 1;
    check_all(0u, 0u, 0u, 0u, true);
    check_all(~0u, ~0u, 0u, 0u, true);
    check_all(~0u, ~0u, ~0u, ~0u, true);
    check_all(0u, 0u, ~0u, ~0u, true);
    for (int i = 0; i < 64; i++) {
        const uint64_t n = one << i;
        check_all((uint32_t)n, (uint32_t)(n >> 32), 0u, 0u, true);
        check_all((uint32_t)n, (uint32_t)(n >> 32), (uint32_t)n, (uint32_t)(n >> 32), true);
        check_all(~(uint32_t)n, ~(uint32_t)(n >> 32), 0u, 0u, true);
        for (int j = i + 1; j < 64 && j <= i + SEED_LEN; j++) {
            const uint64_t m = n | (one << j);
            const uint64_t planes[4] = {0, n, one << j, m};
            for (const uint64_t d : planes)
                check_all((uint32_t)m, (uint32_t)(m >> 32), (uint32_t)d, (uint32_t)(d >> 32), true);
        }
    }
    // random word pairs: bit densities 1/2, 1/4, 1/8, 1/16, 1/32 (the last two are where windows pass); the transversion plane a
    // random half of the mismatches, and in every fourth pair independent of them
    for (int k = 1; k <= 5; k++)
        for (int r = 0; r < 200000; r++) {
            const uint64_t n = sparse64(k);
            const uint64_t d = (r & 3) == 3 ? sparse64(k + 1) : (n & next64());
            check_all((uint32_t)n, (uint32_t)(n >> 32), (uint32_t)d, (uint32_t)(d >> 32), r < 2000);
        }
    if (g_bad) {
        std::printf("seed_window_check: %d mismatches in %llu comparisons\n", g_bad, g_checked);
        return 1;
    }
    std::printf("seed_window_check: ok (%llu comparisons)\n", g_checked);
    return 0;
}
