// K18 — flank repeats (mimeo_flank_repeats, include/mimeo_hip.h): the target-site duplication of an element, the short direct
// repeat immediately outside its two ends, with either end free to move by `slack` bases.  The rules, ties included, are in the
// header.
//
// k18_flank: one wavefront per item, four per workgroup.  The left region fwd[start - slack - max_len, start + slack) is at most
// 48 bases: lane i holds base i.  The right region fwd[end - slack, end + slack + max_len) is at most 48 bases: one wave-uniform
// win64 gives its three masks.  Lane i builds eq_i — bit j: left base i equals right base j, both ACGT and inside the scaffold —
// one row of a 48 x 48 dot matrix, and a candidate (dl, dr, k) is the diagonal run of k cells that ends in row
// max_len + slack + dl - 1 and starts in column slack + dr.  Runs of length t with at most e mismatches whose first column
// matches are carried as Wu-Manber planes, bit j of row i = the run that ends in cell (i, j):
//   S0_1[i] = S1_1[i] = S2_1[i] = eq_i
//   S0_t[i] = eq_i & (S0_{t-1}[i-1] << 1)
//   Se_t[i] = (eq_i & (Se_{t-1}[i-1] << 1)) | (S(e-1)_{t-1}[i-1] << 1)
// where [i-1] comes over with DPP wave_shr:1 on both halves (lane 0 takes 0), as k17_dp moves its H and E: max_len steps of a
// handful of VALU instructions.  At every t >= min_len the lanes whose row is a left end inside the slack keep, of the bits of
// Se_t & eq_i (the last column matches too) whose run starts inside the slack, the best packed key (flank_host.h: pack_key puts
// v, |dl| + |dr|, m, dl, dr in the header's order into one word).  A run with fewer than e mismatches is in plane e too, with a
// smaller v than its own: its key loses against the one from its own plane, so the planes need not be made exclusive.  One
// wave reduction per item ends the job.
//
// Bounds.  A left lane reads base start - slack - max_len + i >= -40 and < start + slack <= L + 8 with base_at (one word, inside
// the PLANE_PAD = 8 words on either side), and only lanes whose base lies inside [0, L) count; the right window starts at
// end - slack >= -8 and win64 reads three words from there, at most (L + 8) / 32 + 2: inside the padding; bits outside [0, L)
// are masked.  So what the padding holds never matters, and an admitted run lies inside the scaffold because its two end
// columns match.  Positions are int32_t as everywhere (a scaffold has fewer than 2^31 - 256 bases).  out[jid], jid < n.  Every
// pointer is a kernel argument or a gptr: no flat access.
#include <cstdio>
#include <cstdlib>

#include "flank_host.h"
#include "path_call.h"

namespace mimeo {

struct K18Params { int32_t min_len, max_len, slack, max_mismatch; };

__device__ __forceinline__ uint64_t k18_row_above(uint64_t v) {   // wave_shr:1 on both halves; lane 0 takes 0
    const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)v, 0x138, 0xf, 0xf, false);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(v >> 32), 0x138, 0xf, 0xf, false);
    return ((uint64_t)hi << 32) | lo;
}

__global__ __launch_bounds__(256) void k18_flank(const StrandView *__restrict__ fwd, const mimeo_interval *__restrict__ items, uint32_t n, K18Params P,
                                                 mimeo_flank_repeat *__restrict__ out) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63u;
    if (jid >= n) return;
    const mimeo_interval it = items[jid];
    const GStrandView A(fwd[it.chrom]);
    const int32_t L = (int32_t)A.len, s = P.slack, M = P.max_len, nl = M + 2 * s;
    // the left region: lane i holds base i
    const int32_t lpos = (int32_t)it.start - s - M + (int32_t)lane;
    bool lv = (int32_t)lane < nl && lpos >= 0 && lpos < L;
    Base1 b{0u, 0u, 1u};
    if (lv) b = base_at(A, lpos);
    lv = lv && !b.nm;
    // the right region: bits [jlo, jhi) lie inside the scaffold
    const int32_t rbase = (int32_t)it.end - s;
    const Win64 wr = win64(A, rbase);
    const int32_t jlo = rbase < 0 ? -rbase : 0, jhi = min(64, L - rbase);
    uint64_t rvalid = 0ull;
    if (jhi > jlo) rvalid = (jhi >= 64 ? ~0ull : (1ull << jhi) - 1ull) & ~((1ull << jlo) - 1ull);
    const uint64_t eq = lv ? ~(wr.lo ^ (b.lo ? ~0ull : 0ull)) & ~(wr.hi ^ (b.hi ? ~0ull : 0ull)) & ~wr.nm & rvalid : 0ull;
    // this lane as the last row of a left copy: dl, and the run starts (columns) that keep start + dl <= end + dr
    const int32_t dl = (int32_t)lane - (s + M) + 1;
    const bool end_row = dl >= -s && dl <= s;
    const int64_t ilen = (int64_t)it.end - (int64_t)it.start;
    const int32_t jmin = (int32_t)max((int64_t)0, (int64_t)(s + dl) - ilen);   // dr >= dl - (end - start)
    const uint32_t wmask = end_row && jmin <= 2 * s ? ((2u << (2 * s)) - 1u) & ~((1u << jmin) - 1u) : 0u;
    uint64_t S0 = eq, S1 = eq, S2 = eq;
    uint32_t key = 0u;
    for (int32_t t = 1; t <= M; t++) {
        if (t > 1) {
            const uint64_t p0 = k18_row_above(S0) << 1, p1 = k18_row_above(S1) << 1, p2 = k18_row_above(S2) << 1;
            S0 = eq & p0;
            S1 = (eq & p1) | p0;
            S2 = (eq & p2) | p1;
        }
        if (t < P.min_len) continue;
#pragma unroll
        for (int32_t e = 0; e <= flank_host::MAX_MISMATCH; e++) {
            const int32_t v = t - flank_host::MISMATCH_CHARGE * e;
            if (e > P.max_mismatch || v < P.min_len) break;   // wave-uniform
            const uint64_t Se = e == 0 ? S0 : e == 1 ? S1 : S2;
            const uint32_t w = (uint32_t)((Se & eq) >> (t - 1)) & wmask;
            if (w) key = max(key, flank_host::pack_key((uint32_t)v, dl, flank_host::best_dr(w, s), (uint32_t)e));
        }
    }
    for (int o = 32; o > 0; o >>= 1) key = max(key, (uint32_t)__shfl_xor((int)key, o));
    if (lane == 0) out[jid] = flank_host::unpack_key(key, it.start, it.end);
}

static_assert(sizeof(mimeo_flank_repeat) == 16 && sizeof(mimeo_interval) == 12, "layouts the kernel relies on");

// MIMEO_ELEMENTS_STATS: a line when the checks have passed, before anything touches the device, and at the end what the call
// did and the HIP-event time of its kernel, on stderr.  MIMEO_PATH_LAUNCH_JOBS (tests) cuts the items into launches.  Results
// depend on neither.
int flank_repeats_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, const mimeo_flank_params *p, mimeo_flank_repeat *out) {
    std::string msg;
    int rc = flank_host::check_params(p, &msg);
    const std::vector<uint64_t> len = scaffold_lengths(G);
    if (!rc && !flank_host::validate_items(flank_host::NAME, len, iv, n, &msg)) rc = MIMEO_ERR_ARG;
    if (rc) { set_error(msg); return rc; }
    if (!n) return 0;
    const bool stats = getenv("MIMEO_ELEMENTS_STATS") != nullptr;
    if (stats) fprintf(stderr, "[k18] checked: %llu items go to the device\n", (unsigned long long)n);
    PathCall pc(stats);
    DeviceBuf &ditems = pc.buf(), &dout = pc.buf();
    if ((rc = pc.views(G, G))) return rc;
    const K18Params P{p->min_len, p->max_len, p->slack, p->max_mismatch};
    const uint64_t per = pc.launch_jobs;
    if ((rc = ditems.reserve(std::min(per, n) * sizeof(mimeo_interval))) || (rc = dout.reserve(std::min(per, n) * sizeof(mimeo_flank_repeat)))) return rc;
    for (uint64_t j0 = 0; j0 < n; j0 += per) {
        const uint32_t nj = (uint32_t)std::min(per, n - j0);
        HIP_TRY(hipMemcpyAsync(ditems.p, iv + j0, nj * sizeof(mimeo_interval), hipMemcpyHostToDevice, pc.st));
        if ((rc = pc.timed([&] {
                hipLaunchKernelGGL(k18_flank, dim3((nj + 3u) / 4u), dim3(256), 0, pc.st, pc.t_fwd(), (const mimeo_interval *)ditems.p, nj, P,
                                   (mimeo_flank_repeat *)dout.p);
            })))
            return rc;
        HIP_TRY(hipMemcpyAsync(out + j0, dout.p, nj * sizeof(mimeo_flank_repeat), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));
    }
    if (stats)
        fprintf(stderr, "[k18] flank repeats: %llu items, %llu launches, kernels %.3f ms\n", (unsigned long long)n, (unsigned long long)pc.launches, pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
