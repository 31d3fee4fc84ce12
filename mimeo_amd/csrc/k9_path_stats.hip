// K9 — column statistics of alignment paths (mimeo_path_stats, include/mimeo_hip.h): for every alignment the matches,
// transitions, transversions and ambiguous columns of its gap-free blocks, and the insertion / deletion runs and bases
// between them.  Nothing in the reference does this (it keeps lastz's identity column and no alignment); it is what a
// substitution-divergence estimate (Kimura's two-parameter distance) and the NM / de tags of a PAF row are made of.
//
// The bit planes hold the answer (common.h): with x the target base and y the query base of a column,
//   ambiguous     nm(x) | nm(y)                      — masked first: what lo / hi hold under an N is never looked at
//   transversion  lo(x) ^ lo(y)                      (A0 C1 G2 T3: purines have lo = 0)
//   transition    lo equal, hi(x) ^ hi(y)
//   match         lo equal, hi equal                 == the oracle's x < 4 && x == y: matches == id_n
// so 64 columns are two XORs, a few ANDs and four popcounts over two win64 windows.
//
// Work layout: one wavefront per job (path_stats_host.h: an alignment, or split_chunks chunks of a long one), four per
// workgroup.  A typical alignment has ~35 blocks of a few hundred columns: one block per lane would idle most lanes, so
// the work is flattened.  64 blocks at a time: lane i loads block i and its chunk count ceil(len / 64), an inclusive wave
// scan gives the item offsets, and the lanes stride over the (block, 64-column chunk) items of the pass, each finding its
// block by a binary search of the scanned counts with lane shuffles.  Counters are per lane, 32 bits (an alignment has
// fewer than 2^32 columns), reduced once at the end; lane 0 writes the 32-byte result — or adds it with integer atomics
// where the alignment was cut into several jobs.  Integers only: exact, and independent of the grid, the slices, the cut
// into jobs and the order of the items.
// Coordinates are those of mimeo_path_block: t on the target's forward strand, q on the query's forward strand or, for
// qstrand == 1, on its stored reverse-complement strand (Scaffold::rc).  Nothing is flipped here.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "device_util.h"
#include "path_stats_host.h"

namespace mimeo {

using path_stats_host::Job;

__global__ __launch_bounds__(256) void k9_path_stats(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                     const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                     const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                     const Job *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ out) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);   // wave-uniform
    if (jid >= njobs) return;
    const Job job = jobs[jid];
    const uint32_t lane = threadIdx.x & 63u;
    const mimeo_alignment a = aln[job.aln];
    // the strand views come out of a device table: into global address space once per wavefront (device_util.h)
    const GStrandView T(t_fwd[a.tid]), Q((a.qstrand ? q_rc : q_fwd)[a.qid]);
    const uint64_t b0 = first[job.aln] - first[0], b1 = first[job.aln + 1] - first[0];   // the slice's blocks start at first[0]
    uint32_t n_match = 0, n_ts = 0, n_tv = 0, n_amb = 0, ins_runs = 0, ins_bases = 0, del_runs = 0, del_bases = 0;
    uint32_t done = 0;   // chunks of the passes before
    // the job that starts the alignment also counts its gaps: it passes over every block, the others stop behind their chunks
    for (uint64_t p = b0; p < b1 && (done < job.c1 || job.c0 == 0); p += 64) {
        const uint64_t idx = p + lane;
        uint32_t bt = 0, bq = 0, blen = 0;
        if (idx < b1) {
            const mimeo_path_block b = blocks[idx];
            bt = b.t; bq = b.q; blen = b.len;
            if (job.c0 == 0 && idx > b0) {   // the gap in front of this block: an insertion run, a deletion run, or both
                const mimeo_path_block pb = blocks[idx - 1];
                const uint32_t dq = bq - (pb.q + pb.len), dt = bt - (pb.t + pb.len);
                if (dq) { ins_runs++; ins_bases += dq; }
                if (dt) { del_runs++; del_bases += dt; }
            }
        }
        const uint32_t chunks = (blen >> 6) + ((blen & 63u) ? 1u : 0u);   // 0 for the lanes behind the last block
        uint32_t incl = chunks;
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
            if (lane >= (uint32_t)d) incl += v;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63), excl = incl - chunks;
        // the items of this pass that belong to the job: [lo, hi) of [0, total)
        const uint32_t lo = job.c0 > done ? min(job.c0 - done, total) : 0u, hi = job.c1 > done ? min(job.c1 - done, total) : 0u;
        for (uint32_t base = lo; base < hi; base += 64) {   // wave-uniform trip count: every lane takes part in the shuffles
            const bool active = base + lane < hi;
            const uint32_t item = active ? base + lane : hi - 1u;
            // block of the item = number of lanes whose inclusive count is <= item (at most 63: item < total = incl of lane 63)
            uint32_t j = 0;
#pragma unroll
            for (uint32_t s = 32; s > 0; s >>= 1)
                if ((uint32_t)__shfl((int)incl, (int)(j + s - 1u)) <= item) j += s;
            const uint32_t jt = (uint32_t)__shfl((int)bt, (int)j), jq = (uint32_t)__shfl((int)bq, (int)j);
            const uint32_t jlen = (uint32_t)__shfl((int)blen, (int)j), jex = (uint32_t)__shfl((int)excl, (int)j);
            if (active) {
                const uint32_t off = (item - jex) << 6, rem = jlen - off;   // rem >= 1: the chunk starts inside its block
                const uint64_t mask = rem >= 64u ? ~0ull : (1ull << rem) - 1ull;
                // bounds: the chunk starts at a base below t + len <= Lt (q + len <= Lq; checked on the host before anything is
                // launched), and win64 reads the three words from that base's word on: at most two words behind the strand's last,
                // inside the PLANE_PAD = 8 zero words that follow it
                const Win64 wt = win64(T, (int32_t)(jt + off)), wq = win64(Q, (int32_t)(jq + off));
                const uint64_t amb = (wt.nm | wq.nm) & mask, ok = mask & ~amb;
                const uint64_t dl = wt.lo ^ wq.lo, dh = wt.hi ^ wq.hi;
                n_amb += (uint32_t)__popcll(amb);
                n_tv += (uint32_t)__popcll(ok & dl);
                n_ts += (uint32_t)__popcll(ok & ~dl & dh);
                n_match += (uint32_t)__popcll(ok & ~dl & ~dh);
            }
        }
        done += total;
    }
    uint32_t c[8] = {n_match, n_ts, n_tv, n_amb, ins_runs, ins_bases, del_runs, del_bases};   // the order of mimeo_column_stats
#pragma unroll
    for (int k = 0; k < 8; k++)
        for (int o = 32; o > 0; o >>= 1) c[k] += (uint32_t)__shfl_xor((int)c[k], o);
    if (lane == 0) {
        uint32_t *dst = out + (uint64_t)job.aln * 8u;
        if (job.split) {   // the output was zeroed on the stream before the launch
#pragma unroll
            for (int k = 0; k < 8; k++) if (c[k]) atomicAdd(dst + k, c[k]);
        } else {
            uint4 *d4 = (uint4 *)dst;   // 32-byte records in a hipMalloc'ed buffer: 16-byte aligned
            d4[0] = make_uint4(c[0], c[1], c[2], c[3]);
            d4[1] = make_uint4(c[4], c[5], c[6], c[7]);
        }
    }
}

static_assert(sizeof(mimeo_column_stats) == 32 && sizeof(Job) == 16 && sizeof(mimeo_path_block) == 12, "layouts the kernel relies on");

// MIMEO_PATH_STATS_SLICE_BLOCKS: blocks per slice (default 2^24 = 192 MiB of blocks; 1: every alignment a slice of its own);
// MIMEO_PATH_STATS_SPLIT_CHUNKS: an alignment of more chunks than this is cut into jobs of this many (default 16384 = one
// megabase of columns; 0: never); MIMEO_PATH_STATS_STATS: what the call did and the HIP-event time of its kernels, on stderr.
// Results depend on none of them.
static uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    return end && *end == 0 ? (uint64_t)v : dflt;
}

int path_stats_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                      const mimeo_path_block *blocks, uint64_t nblocks, mimeo_column_stats *out) {
    if (!n) return 0;
    // every check on the host, before anything is uploaded: a bad path never reaches the kernel
    std::vector<uint64_t> len_t(T->scaf.size()), len_q(Q->scaf.size());
    for (size_t i = 0; i < len_t.size(); i++) len_t[i] = T->scaf[i].len;
    for (size_t i = 0; i < len_q.size(); i++) len_q[i] = Q->scaf[i].len;
    std::string msg;
    if (!path_stats_host::validate(len_t, len_q, aln, n, first, blocks, nblocks, &msg)) { set_error(msg); return MIMEO_ERR_ARG; }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_PATH_STATS_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;   // 48 + 8 + 32 + 16 bytes per record: 416 MiB
    const uint64_t split_chunks = env_u64("MIMEO_PATH_STATS_SPLIT_CHUNKS", 16384);
    const bool stats = getenv("MIMEO_PATH_STATS_STATS") != nullptr;
    hipStream_t st = stream();
    std::vector<StrandView> vt(len_t.size()), vqf(len_q.size()), vqr(len_q.size());
    for (size_t i = 0; i < vt.size(); i++) vt[i] = T->scaf[i].fwd.view(false);
    for (size_t i = 0; i < vqf.size(); i++) { vqf[i] = Q->scaf[i].fwd.view(false); vqr[i] = Q->scaf[i].rc.view(false); }
    DeviceBuf dvt, dvqf, dvqr, da, df, db, dj, dout;
    hipEvent_t ev[2] = {nullptr, nullptr};
    auto done = [&](int r) {
        for (DeviceBuf *b : {&dvt, &dvqf, &dvqr, &da, &df, &db, &dj, &dout}) b->release();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
        return r;
    };
#define K9_TRY(call) do { hipError_t e__ = (call); if (e__ != hipSuccess) return done(hip_fail(e__, #call, __FILE__, __LINE__)); } while (0)
    int rc;
    if ((rc = dvt.reserve(vt.size() * sizeof(StrandView) + 16)) || (rc = dvqf.reserve(vqf.size() * sizeof(StrandView) + 16)) ||
        (rc = dvqr.reserve(vqr.size() * sizeof(StrandView) + 16)))
        return done(rc);
    K9_TRY(hipMemcpyAsync(dvt.p, vt.data(), vt.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    K9_TRY(hipMemcpyAsync(dvqf.p, vqf.data(), vqf.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    K9_TRY(hipMemcpyAsync(dvqr.p, vqr.data(), vqr.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
    if (stats) { K9_TRY(hipEventCreate(&ev[0])); K9_TRY(hipEventCreate(&ev[1])); }
    const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
    std::vector<Job> jobs;
    uint64_t njobs_all = 0, chunks_all = 0;
    double ms_kernel = 0;
    for (const auto &s : slices) {
        const uint64_t a0 = s.first, na = s.second - s.first, k0 = first[a0], nb = first[s.second] - k0;
        path_stats_host::plan_jobs(first, blocks, a0, s.second, split_chunks, jobs);
        if (jobs.size() > 0x00FFFFFFull) { set_error("mimeo_path_stats: more than 2^24 jobs in one slice"); return done(MIMEO_ERR_LIMIT); }
        if ((rc = da.reserve(na * sizeof(mimeo_alignment))) || (rc = df.reserve((na + 1) * 8)) || (rc = db.reserve(nb * sizeof(mimeo_path_block) + 16)) ||
            (rc = dj.reserve(jobs.size() * sizeof(Job))) || (rc = dout.reserve(na * sizeof(mimeo_column_stats))))
            return done(rc);
        // the stream orders a slice's copies behind the launch that read the slice before; the copies themselves return when the
        // caller's (pageable) memory has been read
        K9_TRY(hipMemcpyAsync(da.p, aln + a0, na * sizeof(mimeo_alignment), hipMemcpyHostToDevice, st));
        K9_TRY(hipMemcpyAsync(df.p, first + a0, (na + 1) * 8, hipMemcpyHostToDevice, st));
        if (nb) K9_TRY(hipMemcpyAsync(db.p, blocks + k0, nb * sizeof(mimeo_path_block), hipMemcpyHostToDevice, st));
        K9_TRY(hipMemcpyAsync(dj.p, jobs.data(), jobs.size() * sizeof(Job), hipMemcpyHostToDevice, st));
        K9_TRY(hipStreamSynchronize(st));   // `jobs` is rebuilt for the next slice
        // the jobs of a split alignment add to zero; every other alignment has one job, which stores its whole record
        const bool any_split = std::any_of(jobs.begin(), jobs.end(), [](const Job &j) { return j.split != 0; });
        if (any_split) K9_TRY(hipMemsetAsync(dout.p, 0, na * sizeof(mimeo_column_stats), st));
        if (stats) K9_TRY(hipEventRecord(ev[0], st));
        hipLaunchKernelGGL(k9_path_stats, dim3((uint32_t)((jobs.size() + 3) / 4)), dim3(256), 0, st, (const StrandView *)dvt.p,
                           (const StrandView *)dvqf.p, (const StrandView *)dvqr.p, (const mimeo_alignment *)da.p, (const uint64_t *)df.p,
                           (const mimeo_path_block *)db.p, (const Job *)dj.p, (uint32_t)jobs.size(), (uint32_t *)dout.p);
        K9_TRY(hipGetLastError());
        if (stats) K9_TRY(hipEventRecord(ev[1], st));
        K9_TRY(hipMemcpyAsync(out + a0, dout.p, na * sizeof(mimeo_column_stats), hipMemcpyDeviceToHost, st));
        K9_TRY(hipStreamSynchronize(st));
        if (stats) {
            float ms = 0;
            K9_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
            ms_kernel += ms;
            njobs_all += jobs.size();
            for (const Job &j : jobs) chunks_all += j.c1 - j.c0;
        }
    }
#undef K9_TRY
    if (stats)
        fprintf(stderr, "[k9] path stats: %llu alignments, %llu blocks, %llu chunks, %llu jobs, slices %zu, kernels %.3f ms\n", (unsigned long long)n,
                (unsigned long long)nblocks, (unsigned long long)chunks_all, (unsigned long long)njobs_all, slices.size(), ms_kernel);
    return done(0);
}

}  // namespace mimeo
