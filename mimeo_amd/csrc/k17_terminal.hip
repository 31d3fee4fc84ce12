// K17 — terminal repeats of features (mimeo_terminal_repeats, include/mimeo_hip.h): for every item a full affine-gap local
// alignment of its first w bases against its last w bases, and against the stored reverse complement of the last w bases.
// 2 n independent w x w Gotoh DPs with a stored traceback; the rules, ties included, are in the header.
//
// k17_dp: one wavefront per job, a workgroup of 64.  The matrix is swept in strips of 64 columns of b; inside a strip lane l owns
// column j0 + l and the rows are skewed across the lanes, lane l at row t - l in step t (a systolic anti-diagonal sweep of
// w + 63 steps), so that what a cell needs from its left neighbour — H and E of (i, j - 1) — is what lane l - 1 made one step
// before: two DPP wave shifts (wave_shr:1, as k6.h), no LDS.  H[i-1][j-1] is the H that arrived one step earlier, H and F of
// (i - 1, j) are the lane's own.  Lane 0 takes its left neighbour from LDS, where lane 63 of the strip before left H and E of its
// column row by row (bnd[], read as the `old` operand of the shift, which lane 0 keeps); entry row + 64, so that lane 63's store
// in step t (row t - 63, entry t + 1) lies 63 entries behind lane 0's read (row t, entry t + 64) and one array serves both.
// The bases: a lane turns its column's base of b into three masks once per strip (win64), and once per 64 steps loads the 64
// rows it is about to meet (win64 at a0 + T - l: each lane its own alignment) and folds both into one 64-bit "not a match"
// word, one bit per step; a cell's score is a shift and a select.
// Cells outside the matrix are computed like any other, with every column a mismatch: rows t - l < 0 then hold H = 0 and what
// they pass on (E = F = -gap_open - gap_extend) is what the recurrence gives on the first row anyway; rows >= w and columns
// >= w of the last strip hold values that no cell of the matrix reads (dependencies run up and to the left), each smaller
// than some H of the matrix (every step into them costs a mismatch or a gap), so they never become the best cell.  No cell is
// masked in the inner loop.
// Traceback: four bits per cell — the source of H (0 stop, 1 diagonal, 2 E, 3 F), "E extends", "F extends" ("opened" wins the
// tie, as the header says).  A lane packs the nibbles of eight consecutive steps into a word and all 64 lanes store together,
// 256 contiguous bytes: word (strip, t >> 3, lane) of the job's scratch (terminal_host.h: trace_word).
// Best cell: per lane and strip the first strictly larger H (rows ascend), merged per strip into one 64-bit key — score,
// 0xFFFF - i, 0xFFFF - j — whose maximum is the largest H with the smallest i, then the smallest j; one wave reduction per job.
//
// k17_walk: one lane per job walks back from the best cell through the nibbles, writes the blocks from the end of the job's
// region of w blocks backwards (a path has at most one block per row), counts the matching columns from the bit planes and
// makes the record.  k17_gather copies the blocks to their dense places behind a prefix sum of the counts (rocPRIM, as
// dense_paths_device).
//
// Bounds.  Positions on a strand are int32_t in win64 and base_at, as everywhere: pack_scaffold (k1_pack.hip) refuses a scaffold
// longer than 2^31 - 256 bases, so a0 + w + 132 and b0 + w stay below 2^31.  Strands: b is read from b0 + j0 < b0 + w <= len with
// win64 (three words, inside PLANE_PAD); a from a0 + T - l with
// -63 <= T - l and T < w + 70, so from base -63 on and up to word (len + 68) / 32 + 2: inside the 8 pad words on either side.
// Scratch: every (strip, step group, lane) below strips(w) * step_groups(w) * 64 = trace_words(w) words, which the host laid
// out; the walk reads cells of the matrix only.  LDS: entries 0 .. steps + 63 of steps + 64.  Every pointer is a kernel
// argument or a gptr: no flat access.
#include <cstdio>
#include <cstdlib>
#include <cstring>   // rocPRIM's headers call memset without including it
#include <rocprim/rocprim.hpp>

#include "path_call.h"
#include "terminal_host.h"

namespace mimeo {

using terminal_host::Job;

struct K17Score { int32_t match, mismatch, goe, ge, min_score; };   // goe = gap_open + gap_extend

constexpr int32_t K17_NEG = -(1 << 29);   // no E, no F: below every score, and K17_NEG - 1000 does not wrap

__device__ __forceinline__ int32_t k17_shr1(int32_t old, int32_t v) { return __builtin_amdgcn_update_dpp(old, v, 0x138, 0xf, 0xf, false); }   // wave_shr:1

__global__ __launch_bounds__(64) void k17_dp(const StrandView *__restrict__ fwd, const StrandView *__restrict__ rc, const Job *__restrict__ jobs,
                                             uint32_t njobs, K17Score S, uint32_t *__restrict__ trace, unsigned long long *__restrict__ best) {
    extern __shared__ int2 bnd[];   // H and E of the column in front of the strip: entry row + 64
    const uint32_t jid = blockIdx.x, lane = threadIdx.x;
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const uint32_t w = job.w;
    if (!w) {
        if (lane == 0) best[jid] = 0ull;
        return;
    }
    const GStrandView A(fwd[job.chrom]), B((job.strand ? rc : fwd)[job.chrom]);
    const uint32_t groups = terminal_host::step_groups(w), steps = groups * 8u, nstrips = terminal_host::strips(w);
    for (uint32_t k = lane; k < steps + 64u; k += 64u) bnd[k] = make_int2(0, K17_NEG);   // in front of column 0
    __syncthreads();
    uint32_t *__restrict__ tr = trace + job.trace_off;
    unsigned long long key = 0ull;
    for (uint32_t strip = 0; strip < nstrips; strip++) {
        const uint32_t j0 = strip << 6, j = j0 + lane;
        const Win64 wb = win64(B, (int32_t)(job.b0 + j0));
        const uint64_t blo = ((wb.lo >> lane) & 1ull) ? ~0ull : 0ull, bhi = ((wb.hi >> lane) & 1ull) ? ~0ull : 0ull;
        const uint64_t bnm = (((wb.nm >> lane) & 1ull) || j >= w) ? ~0ull : 0ull;
        int32_t hout = 0, eout = K17_NEG, hup = 0, fup = K17_NEG, hdiag = 0, bh = 0;
        uint32_t bt = 0;
        uint32_t *__restrict__ tw = tr + (uint64_t)strip * groups * 64u + lane;
        for (uint32_t T = 0; T < steps; T += 64u) {
            // the 64 rows of this lane's next 64 steps, T - lane + k: a mismatch wherever the row lies outside the matrix
            const int32_t r0 = (int32_t)T - (int32_t)lane;
            const Win64 wa = win64(A, (int32_t)job.a0 + r0);
            const int32_t klo = r0 < 0 ? -r0 : 0, khi = min(64, (int32_t)w - r0);   // the rows of the matrix are bits [klo, khi)
            uint64_t inside = 0ull;
            if (khi > klo) inside = (khi >= 64 ? ~0ull : (1ull << khi) - 1ull) & ~((1ull << klo) - 1ull);   // klo <= 63
            const uint64_t mism = (wa.lo ^ blo) | (wa.hi ^ bhi) | wa.nm | bnm | ~inside;
            for (uint32_t g = 0; g < 8u && T + 8u * g < steps; g++) {
                const uint32_t t0 = T + 8u * g, m8 = (uint32_t)(mism >> (8u * g));
                int2 left[8];
#pragma unroll
                for (int k = 0; k < 8; k++) left[k] = bnd[t0 + k + 64u];
                uint32_t acc = 0;
#pragma unroll
                for (int k = 0; k < 8; k++) {
                    const int32_t hl = k17_shr1(left[k].x, hout), el = k17_shr1(left[k].y, eout);
                    const int32_t eo = hl - S.goe, ee = el - S.ge, fo = hup - S.goe, fe = fup - S.ge;
                    const int32_t e = max(eo, ee), f = max(fo, fe);
                    const int32_t dg = hdiag + (((m8 >> k) & 1u) ? -S.mismatch : S.match);
                    const int32_t h = max(max(dg, 0), max(e, f));
                    const uint32_t src = h == 0 ? 0u : h == dg ? 1u : h == e ? 2u : 3u;
                    acc |= (src | (ee > eo ? 4u : 0u) | (fe > fo ? 8u : 0u)) << (4 * k);
                    if (h > bh) { bh = h; bt = t0 + k; }
                    if (lane == 63u) bnd[t0 + k + 1u] = make_int2(h, e);
                    hdiag = hl; hup = h; fup = f; hout = h; eout = e;
                }
                tw[(uint64_t)(t0 >> 3) * 64u] = acc;
            }
        }
        if (bh > 0) {   // row bt - lane >= 0: H is 0 above the matrix; below 65536 like the column
            const unsigned long long k = ((unsigned long long)(uint32_t)bh << 32) | ((unsigned long long)(0xFFFFu - (bt - lane)) << 16) | (0xFFFFu - j);
            key = max(key, k);
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)key, o), hi = (uint32_t)__shfl_xor((int)(uint32_t)(key >> 32), o);
        key = max(key, ((unsigned long long)hi << 32) | lo);
    }
    if (lane == 0) best[jid] = key;
}

// One lane per job: the walk back from the best cell.  Every step lowers i or j, so the walk ends; it reads cells of the
// matrix only and writes at most one block per row.
__global__ __launch_bounds__(64) void k17_walk(const StrandView *__restrict__ fwd, const StrandView *__restrict__ rc, const Job *__restrict__ jobs,
                                               uint32_t njobs, K17Score S, const uint32_t *__restrict__ trace, const unsigned long long *__restrict__ best,
                                               mimeo_path_block *__restrict__ region, mimeo_alignment *__restrict__ out, uint32_t *__restrict__ cnt) {
    const uint32_t jid = blockIdx.x * 64u + threadIdx.x;
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    mimeo_alignment r{};
    r.tid = r.qid = job.chrom;
    r.qstrand = job.strand;
    const unsigned long long key = best[jid];
    const int32_t score = (int32_t)(key >> 32);
    uint32_t nblk = 0;
    if (job.w && score >= S.min_score) {
        const GStrandView A(fwd[job.chrom]), B((job.strand ? rc : fwd)[job.chrom]);
        const uint32_t w = job.w;
        const uint32_t *__restrict__ tr = trace + job.trace_off;
        mimeo_path_block *__restrict__ reg = region + job.blk_off;
        const int32_t bi = (int32_t)(0xFFFFu - (uint32_t)((key >> 16) & 0xFFFFu)), bj = (int32_t)(0xFFFFu - (uint32_t)(key & 0xFFFFu));
        int32_t i = bi, j = bj, ci = 0, cj = 0;
        uint32_t clen = 0, id_n = 0, id_d = 0, state = 0;   // 0 H, 1 E, 2 F
        while (i >= 0 && j >= 0) {
            const uint32_t nib = (tr[terminal_host::trace_word(w, (uint32_t)i, (uint32_t)j)] >> terminal_host::trace_shift((uint32_t)i, (uint32_t)j)) & 15u;
            if (state == 0) {
                const uint32_t src = nib & 3u;
                if (src == 0u) break;
                if (src == 1u) {
                    if (clen && ci == i + 1 && cj == j + 1) {
                        ci = i; cj = j; clen++;
                    } else {
                        if (clen) reg[w - 1u - nblk++] = mimeo_path_block{job.a0 + (uint32_t)ci, job.b0 + (uint32_t)cj, clen};
                        ci = i; cj = j; clen = 1;
                    }
                    const Base1 x = base_at(A, (int32_t)(job.a0 + (uint32_t)i)), y = base_at(B, (int32_t)(job.b0 + (uint32_t)j));
                    id_n += !(x.nm | y.nm | (x.lo ^ y.lo) | (x.hi ^ y.hi));
                    id_d++;
                    i--; j--;
                } else {
                    state = src == 2u ? 1u : 2u;
                }
            } else if (state == 1u) {
                if (!(nib & 4u)) state = 0;
                j--;
            } else {
                if (!(nib & 8u)) state = 0;
                i--;
            }
        }
        if (clen) reg[w - 1u - nblk++] = mimeo_path_block{job.a0 + (uint32_t)ci, job.b0 + (uint32_t)cj, clen};
        if (nblk) {   // ci, cj: the first column of the path
            const uint32_t q0 = job.b0 + (uint32_t)cj, q1 = job.b0 + (uint32_t)bj + 1u;
            r.tstart = job.a0 + (uint32_t)ci;
            r.tend = job.a0 + (uint32_t)bi + 1u;
            r.qstart = job.strand ? B.len - q1 : q0;
            r.qend = job.strand ? B.len - q0 : q1;
            r.score = score;
            r.id_n = id_n;
            r.id_d = id_d;
        }
    }
    out[job.slot] = r;
    cnt[job.slot] = nblk;
}

// the blocks of job p from the end of its region to their dense place: one wavefront per job, four per workgroup
__global__ __launch_bounds__(256) void k17_gather(const Job *__restrict__ jobs, uint32_t njobs, const uint32_t *__restrict__ cnt,
                                                  const unsigned long long *__restrict__ first, const mimeo_path_block *__restrict__ region,
                                                  mimeo_path_block *__restrict__ dense) {
    const uint32_t jid = (blockIdx.x * 256u + threadIdx.x) >> 6, lane = threadIdx.x & 63u;
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const uint32_t n = cnt[job.slot];
    const mimeo_path_block *__restrict__ src = region + job.blk_off + (job.w - n);
    mimeo_path_block *__restrict__ dst = dense + first[job.slot];
    for (uint32_t k = lane; k < n; k += 64u) dst[k] = src[k];
}

static_assert(sizeof(Job) == 40 && sizeof(mimeo_alignment) == 48 && sizeof(mimeo_path_block) == 12, "layouts the kernels rely on");

// MIMEO_TERMINAL_SCRATCH_MB: the scratch of one launch (tests: force the cut into launches; default a quarter of the free device
// memory, 8 GiB at most); MIMEO_TERMINAL_STATS: a line when the checks have passed, before anything touches the device, and at
// the end what the call did and the HIP-event time of its kernels, on stderr.  Results
// depend on neither.
int terminal_repeats_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, const mimeo_terminal_params *p, mimeo_alignment *out,
                            uint64_t **path_first, mimeo_path_block **blocks, uint64_t *nblocks) {
    std::string msg;
    int rc = terminal_host::check_params(p, &msg);
    const std::vector<uint64_t> len = scaffold_lengths(G);
    if (!rc && !terminal_host::validate_items(len, iv, n, &msg)) rc = MIMEO_ERR_ARG;
    if (rc) { set_error(msg); return rc; }
    *blocks = nullptr;
    *nblocks = 0;
    uint64_t *pf = (uint64_t *)calloc(2 * n + 1, sizeof(uint64_t));
    if (!pf) { set_error("mimeo_terminal_repeats: out of host memory"); return MIMEO_ERR_NOMEM; }
    *path_first = pf;
    if (!n) return 0;
    // MIMEO_TERMINAL_STATS: this line is printed where the checks are behind and before the first HIP call of the call
    if (getenv("MIMEO_TERMINAL_STATS")) fprintf(stderr, "[k17] checked: %llu items go to the device\n", (unsigned long long)n);
    // from here on every way out with an error releases what the caller was to get
    struct Result {
        uint64_t **pf; mimeo_path_block **blk; bool keep = false;
        ~Result() { if (!keep) { free(*pf); free(*blk); *pf = nullptr; *blk = nullptr; } }
    } result{path_first, blocks};
    std::vector<uint32_t> w_of(n);
    for (uint64_t k = 0; k < n; k++) w_of[k] = terminal_host::windows(iv[k], len[iv[k].chrom], p->window).w;
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    std::vector<unsigned long long> firstL;
    PathCall pc(getenv("MIMEO_TERMINAL_STATS") != nullptr);
    uint64_t budget = env_u64("MIMEO_TERMINAL_SCRATCH_MB", 0) << 20;
    if (!budget) {
        size_t free_b = 0, total_b = 0;
        HIP_TRY(hipMemGetInfo(&free_b, &total_b));
        budget = std::min<uint64_t>((uint64_t)free_b / 4, 8ull << 30);
    }
    const auto launches = terminal_host::plan_launches(w_of, budget);
    DeviceBuf &djobs = pc.buf(), &dtrace = pc.buf(), &dregion = pc.buf(), &dbest = pc.buf(), &drec = pc.buf(), &dcnt = pc.buf(), &dfirst = pc.buf(),
              &dtmp = pc.buf(), &ddense = pc.buf();
    if ((rc = pc.views(G, G))) return rc;
    const K17Score S{p->match, p->mismatch, p->gap_open + p->gap_extend, p->gap_extend, p->min_score};
    double ms_dp = 0, ms_walk = 0;
    uint64_t cells = 0, total = 0, cap = 0;
    for (const auto &L : launches) {
        uint64_t tw = 0, nb = 0;
        terminal_host::plan_jobs(iv, len, p->window, L.first, L.second, jobs, &tw, &nb);
        const uint32_t nj = (uint32_t)jobs.size(), wmax = jobs[0].w;
        const uint64_t j0 = 2 * L.first;
        for (const Job &j : jobs) cells += (uint64_t)j.w * j.w;
        if ((rc = djobs.reserve(nj * sizeof(Job))) || (rc = dtrace.reserve(tw * 4 + 16)) || (rc = dregion.reserve(nb * sizeof(mimeo_path_block) + 16)) ||
            (rc = dbest.reserve(nj * 8ull)) || (rc = drec.reserve(nj * sizeof(mimeo_alignment))) || (rc = dcnt.reserve((nj + 1ull) * 4)) ||
            (rc = dfirst.reserve((nj + 1ull) * 8)))
            return rc;
        HIP_TRY(hipMemcpyAsync(djobs.p, jobs.data(), nj * sizeof(Job), hipMemcpyHostToDevice, pc.st));
        HIP_TRY(hipMemsetAsync(dcnt.p, 0, (nj + 1ull) * 4, pc.st));   // the entry behind the last job: the scan's total
        const size_t lds = ((size_t)terminal_host::step_groups(wmax) * 8u + 64u) * sizeof(int2);   // the launch's longest window
        double before = pc.ms_kernel;
        if (wmax && (rc = pc.timed([&] {
                hipLaunchKernelGGL(k17_dp, dim3(nj), dim3(64), lds, pc.st, pc.t_fwd(), pc.q_rc(), (const Job *)djobs.p, nj, S, (uint32_t *)dtrace.p,
                                   (unsigned long long *)dbest.p);
            })))
            return rc;
        if (!wmax) HIP_TRY(hipMemsetAsync(dbest.p, 0, nj * 8ull, pc.st));
        ms_dp += pc.ms_kernel - before;
        before = pc.ms_kernel;
        if ((rc = pc.timed([&] {
                hipLaunchKernelGGL(k17_walk, dim3((nj + 63u) / 64u), dim3(64), 0, pc.st, pc.t_fwd(), pc.q_rc(), (const Job *)djobs.p, nj, S, (const uint32_t *)dtrace.p,
                                   (const unsigned long long *)dbest.p, (mimeo_path_block *)dregion.p, (mimeo_alignment *)drec.p, (uint32_t *)dcnt.p);
            })))
            return rc;
        ms_walk += pc.ms_kernel - before;
        size_t tb = 0;
        HIP_TRY(rocprim::exclusive_scan(nullptr, tb, (uint32_t *)dcnt.p, (unsigned long long *)dfirst.p, 0ull, (size_t)nj + 1, rocprim::plus<unsigned long long>(), pc.st));
        if ((rc = dtmp.reserve(tb ? tb : 1))) return rc;
        HIP_TRY(rocprim::exclusive_scan(dtmp.p, tb, (uint32_t *)dcnt.p, (unsigned long long *)dfirst.p, 0ull, (size_t)nj + 1, rocprim::plus<unsigned long long>(), pc.st));
        firstL.resize(nj + 1ull);
        HIP_TRY(hipMemcpyAsync(firstL.data(), dfirst.p, (nj + 1ull) * 8, hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipMemcpyAsync(out + j0, drec.p, nj * sizeof(mimeo_alignment), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));
        const uint64_t got = firstL[nj];
        for (uint32_t s = 0; s < nj; s++) pf[j0 + s + 1] = total + firstL[s + 1ull];
        if (got) {
            if (total + got > cap) {
                cap = std::max<uint64_t>(2 * cap, total + got);
                mimeo_path_block *grown = (mimeo_path_block *)realloc(*blocks, cap * sizeof(mimeo_path_block));
                if (!grown) { set_error("mimeo_terminal_repeats: out of host memory"); return MIMEO_ERR_NOMEM; }
                *blocks = grown;
            }
            if ((rc = ddense.reserve(got * sizeof(mimeo_path_block)))) return rc;
            if ((rc = pc.timed([&] {
                    hipLaunchKernelGGL(k17_gather, dim3((nj + 3u) / 4u), dim3(256), 0, pc.st, (const Job *)djobs.p, nj, (const uint32_t *)dcnt.p,
                                       (const unsigned long long *)dfirst.p, (const mimeo_path_block *)dregion.p, (mimeo_path_block *)ddense.p);
                })))
                return rc;
            HIP_TRY(hipMemcpyAsync(*blocks + total, ddense.p, got * sizeof(mimeo_path_block), hipMemcpyDeviceToHost, pc.st));
            HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` is rebuilt for the next launch
            total += got;
        }
    }
    *nblocks = total;
    result.keep = true;
    if (pc.stats)
        fprintf(stderr, "[k17] terminal repeats: %llu items, %llu jobs, %zu launches, %llu cells, dp %.3f ms, walk %.3f ms, kernels %.3f ms, %llu blocks\n",
                (unsigned long long)n, (unsigned long long)(2 * n), launches.size(), (unsigned long long)cells, ms_dp, ms_walk, pc.ms_kernel,
                (unsigned long long)total);
    return 0;
}

}  // namespace mimeo
