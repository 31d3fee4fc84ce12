// K19 — open frames (mimeo_open_frames, include/mimeo_hip.h): the longest run of open codons in each of the six reading frames
// of an item, and the first ATG of that run.  The rules are in the header.
//
// k19_scan: one wavefront per chunk job (frames_host.h: one strand of one item, the codon starts of one chunk, all three frames
// together; the minus strand is the same code on the stored reverse complement), four per workgroup.  A step covers 4096 bases:
// lane l takes win64 at the job's origin + 64 (64 step + l).  The planes shifted by one and two bases need the first two bits
// of the next word: they come from lane l + 1 by DPP wave_shl:1, and lane 63 takes them from one extra load.  The closed mask
// of 64 codon starts follows in bit logic from the A0 C1 G2 T3 code (T = lo & hi, A = ~lo & ~hi, G = ~lo & hi):
// T0 & A1 & ~lo2 is TAA or TAG, T0 & G1 & A2 is TGA, and a set bit of the N plane at 0, +1 or +2 closes the codon.  The frame
// of a codon start is its item offset mod 3, and 64 mod 3 = 1, so the three residue masks rotate from word to word
// (frames_host.h: word_monoid).  Per frame the word reduces to the monoid (first codon, codons, open prefix, open suffix, best
// run, its start) by a walk over its closed codons — about one per frame and word in random sequence, none inside a gene — the
// lanes combine in order by a tree of shuffles, and the step's result combines with the carry of the steps before (lane 0).
// k19_merge: one lane per (item, strand, frame) combines the chunk elements in order and makes the record.
// k19_met: one wavefront per record with codons > 0 looks for ATG with ballots over the run's codons and stops at the first.
//
// Bounds.  A lane loads only where its word holds a base of the item (X < m), from origin + X < origin + m <= L on the strand:
// win64 reads three words from that base's word on, at most two behind the strand's last, inside the PLANE_PAD = 8 words that
// follow it; lane 63's two extra bases are read only where they belong to the item.  Bits behind the item's last codon start
// are masked by vb, so what lies behind the item — the scaffold's neighbours or the padding — never matters.  Positions are
// int32_t as everywhere (a scaffold has fewer than 2^31 - 256 bases).  mono[3 slot + phi], slot < the launch's jobs;
// out[idx] and t0[idx], idx < 6 items.  k19_met reads the bases of open codons, inside the item.  Every pointer is a kernel
// argument or a gptr: no flat access.
#include <cstdio>
#include <cstdlib>

#include "frames_host.h"
#include "path_call.h"

namespace mimeo {

using frames_host::Job;
using frames_host::Monoid;

__device__ __forceinline__ Monoid k19_from_lane_below(const Monoid &m, int d) {   // lane l takes lane l + d's
    return Monoid{(uint32_t)__shfl_down((int)m.t0, d), (uint32_t)__shfl_down((int)m.n, d),  (uint32_t)__shfl_down((int)m.pre, d),
                  (uint32_t)__shfl_down((int)m.suf, d), (uint32_t)__shfl_down((int)m.best, d), (uint32_t)__shfl_down((int)m.bs, d)};
}

__global__ __launch_bounds__(256) void k19_scan(const StrandView *__restrict__ fwd, const StrandView *__restrict__ rc, const Job *__restrict__ jobs,
                                                uint32_t njobs, Monoid *__restrict__ mono) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63u;
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const GStrandView V((job.strand ? rc : fwd)[job.chrom]);
    const uint32_t limit = job.x0 + job.bases;   // the chunk's codon starts end here: at most m - 2
    Monoid carry[3] = {};
    for (uint32_t x = job.x0; x < limit; x += frames_host::STEP) {   // wave-uniform
        const uint32_t X = x + 64u * lane;
        const uint32_t vb = X < limit ? min(64u, limit - X) : 0u;
        Win64 w{0ull, 0ull, 0ull, 0ull};
        if (X < job.m) w = win64(V, (int32_t)(job.origin + X));
        // the first two bases of the next word: lo, hi, nm in bits 0-1, 2-3, 4-5
        const uint32_t mine = ((uint32_t)w.lo & 3u) | (((uint32_t)w.hi & 3u) << 2) | (((uint32_t)w.nm & 3u) << 4);
        uint32_t next = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)mine, 0x130, 0xf, 0xf, false);   // wave_shl:1; lane 63 takes 0
        if (lane == 63u && X + 64u < job.m) {
            const Base1 b0 = base_at(V, (int32_t)(job.origin + X + 64u));
            next = b0.lo | (b0.hi << 2) | (b0.nm << 4);
            if (X + 65u < job.m) {
                const Base1 b1 = base_at(V, (int32_t)(job.origin + X + 65u));
                next |= (b1.lo << 1) | (b1.hi << 3) | (b1.nm << 5);
            }
        }
        const uint64_t nlo = next & 3u, nhi = (next >> 2) & 3u, nnm = (next >> 4) & 3u;
        const uint64_t lo1 = (w.lo >> 1) | (nlo << 63), lo2 = (w.lo >> 2) | (nlo << 62);
        const uint64_t hi1 = (w.hi >> 1) | (nhi << 63), hi2 = (w.hi >> 2) | (nhi << 62);
        const uint64_t nm1 = (w.nm >> 1) | (nnm << 63), nm2 = (w.nm >> 2) | (nnm << 62);
        const uint64_t T0 = w.lo & w.hi, A1 = ~lo1 & ~hi1, G1 = ~lo1 & hi1, A2 = ~lo2 & ~hi2;
        const uint64_t closed = (T0 & A1 & ~lo2) | (T0 & G1 & A2) | w.nm | nm1 | nm2;
#pragma unroll
        for (uint32_t phi = 0; phi < 3u; phi++) {
            Monoid e = frames_host::word_monoid(closed, vb, X, phi);
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {   // lane l ends with the words l .. l + 2 d - 1, where l is a multiple of 2 d
                const Monoid o = k19_from_lane_below(e, d);
                if (!(lane & (uint32_t)(2 * d - 1))) e = frames_host::combine(e, o);
            }
            carry[phi] = frames_host::combine(carry[phi], e);   // lane 0's is the step's
        }
    }
    if (lane == 0)
        for (uint32_t phi = 0; phi < 3u; phi++) mono[3ull * job.slot + phi] = carry[phi];
}

__global__ __launch_bounds__(256) void k19_merge(const mimeo_interval *__restrict__ items, uint32_t nrec, const uint32_t *__restrict__ first_slot,
                                                 const Monoid *__restrict__ mono, mimeo_open_frame *__restrict__ out, uint32_t *__restrict__ t0) {
    const uint32_t idx = blockIdx.x * 256u + threadIdx.x;
    if (idx >= nrec) return;
    const uint32_t k = idx / 6u, sigma = (idx % 6u) / 3u, phi = idx % 3u;
    const mimeo_interval it = items[k];
    Monoid acc{};
    for (uint32_t s = first_slot[2u * k + sigma], s1 = first_slot[2u * k + sigma + 1u]; s < s1; s++) acc = frames_host::combine(acc, mono[3ull * s + phi]);
    out[idx] = frames_host::record(acc, it.start, it.end, sigma, phi);
    t0[idx] = acc.bs;
}

__global__ __launch_bounds__(256) void k19_met(const StrandView *__restrict__ fwd, const StrandView *__restrict__ rc, const mimeo_interval *__restrict__ items,
                                               uint32_t nrec, const uint32_t *__restrict__ t0, mimeo_open_frame *__restrict__ out) {
    const uint32_t idx = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6), lane = threadIdx.x & 63u;
    if (idx >= nrec) return;
    const uint32_t codons = out[idx].codons;
    if (!codons) return;   // wave-uniform
    const uint32_t sigma = (idx % 6u) / 3u, phi = idx % 3u;
    const mimeo_interval it = items[idx / 6u];
    const GStrandView V((sigma ? rc : fwd)[it.chrom]);
    const uint32_t first = (sigma ? V.len - it.end : it.start) + phi + 3u * t0[idx];   // the run's first base on the strand
    uint32_t met = codons;
    for (uint32_t u0 = 0; u0 < codons; u0 += 64u) {
        const uint32_t u = u0 + lane;
        bool hit = false;
        if (u < codons) {
            const int32_t p = (int32_t)(first + 3u * u);
            const Base1 a = base_at(V, p), b = base_at(V, p + 1), c = base_at(V, p + 2);
            hit = !(a.lo | a.hi | a.nm) && (b.lo & b.hi & ~b.nm & 1u) && (~c.lo & c.hi & ~c.nm & 1u);
        }
        const unsigned long long any = __ballot(hit);
        if (any) { met = u0 + (uint32_t)__builtin_ctzll(any); break; }
    }
    if (lane == 0) out[idx].met = met;
}

static_assert(sizeof(Job) == 32 && sizeof(Monoid) == 24 && sizeof(mimeo_open_frame) == 16, "layouts the kernels rely on");

// MIMEO_FRAMES_CHUNK: the bases of a chunk (tests: force the cut; rounded up to whole steps; default 2^16); MIMEO_ELEMENTS_STATS:
// a line when the checks have passed, before anything touches the device, and at the end what the call did, the HIP-event times
// of its kernels and the bases scanned, on stderr.  Results depend on neither.
int open_frames_device(const mimeo_genome *G, const mimeo_interval *iv, uint64_t n, uint32_t flags, mimeo_open_frame *out) {
    std::string msg;
    int rc = frames_host::check_flags(flags, &msg);
    const std::vector<uint64_t> len = scaffold_lengths(G);
    if (!rc && !flank_host::validate_items(frames_host::NAME, len, iv, n, &msg)) rc = MIMEO_ERR_ARG;
    if (rc) { set_error(msg); return rc; }
    if (!n) return 0;
    const bool stats = getenv("MIMEO_ELEMENTS_STATS") != nullptr;
    const uint32_t chunk = frames_host::chunk_bases(env_u64("MIMEO_FRAMES_CHUNK", 0));
    if (stats) fprintf(stderr, "[k19] checked: %llu items go to the device, chunks of %u bases\n", (unsigned long long)n, chunk);
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    std::vector<uint32_t> first_slot;
    PathCall pc(stats);
    DeviceBuf &djobs = pc.buf(), &dmono = pc.buf(), &dfirst = pc.buf(), &ditems = pc.buf(), &dout = pc.buf(), &dt0 = pc.buf();
    if ((rc = pc.views(G, G))) return rc;
    const auto launches = frames_host::plan_launches(iv, n, chunk);
    double ms_scan = 0;
    uint64_t bases = 0, njobs = 0;
    for (const auto &L : launches) {
        frames_host::plan_jobs(iv, len, chunk, L.first, L.second, jobs, first_slot);
        const uint32_t ni = (uint32_t)(L.second - L.first), nj = (uint32_t)jobs.size(), nrec = 6u * ni;
        for (uint64_t k = L.first; k < L.second; k++) bases += 2ull * (iv[k].end - iv[k].start);
        njobs += nj;
        if ((rc = djobs.reserve(nj * sizeof(Job) + 16)) || (rc = dmono.reserve(3ull * nj * sizeof(Monoid) + 16)) || (rc = dfirst.reserve(first_slot.size() * 4ull)) ||
            (rc = ditems.reserve(ni * sizeof(mimeo_interval))) || (rc = dout.reserve(nrec * sizeof(mimeo_open_frame))) || (rc = dt0.reserve(nrec * 4ull)))
            return rc;
        if (nj) HIP_TRY(hipMemcpyAsync(djobs.p, jobs.data(), nj * sizeof(Job), hipMemcpyHostToDevice, pc.st));
        HIP_TRY(hipMemcpyAsync(dfirst.p, first_slot.data(), first_slot.size() * 4ull, hipMemcpyHostToDevice, pc.st));
        HIP_TRY(hipMemcpyAsync(ditems.p, iv + L.first, ni * sizeof(mimeo_interval), hipMemcpyHostToDevice, pc.st));
        const double before = pc.ms_kernel;
        if (nj && (rc = pc.timed([&] {
                hipLaunchKernelGGL(k19_scan, dim3((nj + 3u) / 4u), dim3(256), 0, pc.st, pc.t_fwd(), pc.q_rc(), (const Job *)djobs.p, nj, (Monoid *)dmono.p);
            })))
            return rc;
        ms_scan += pc.ms_kernel - before;
        if ((rc = pc.timed([&] {
                hipLaunchKernelGGL(k19_merge, dim3((nrec + 255u) / 256u), dim3(256), 0, pc.st, (const mimeo_interval *)ditems.p, nrec, (const uint32_t *)dfirst.p,
                                   (const Monoid *)dmono.p, (mimeo_open_frame *)dout.p, (uint32_t *)dt0.p);
            })))
            return rc;
        if ((rc = pc.timed([&] {
                hipLaunchKernelGGL(k19_met, dim3((nrec + 3u) / 4u), dim3(256), 0, pc.st, pc.t_fwd(), pc.q_rc(), (const mimeo_interval *)ditems.p, nrec,
                                   (const uint32_t *)dt0.p, (mimeo_open_frame *)dout.p);
            })))
            return rc;
        HIP_TRY(hipMemcpyAsync(out + 6ull * L.first, dout.p, nrec * sizeof(mimeo_open_frame), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` is rebuilt for the next launch
    }
    if (stats)
        fprintf(stderr, "[k19] open frames: %llu items, %llu chunk jobs, %zu launches, %llu bases scanned, scan %.3f ms, kernels %.3f ms\n", (unsigned long long)n,
                (unsigned long long)njobs, launches.size(), (unsigned long long)bases, ms_scan, pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
