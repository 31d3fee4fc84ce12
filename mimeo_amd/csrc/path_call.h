// path_call.h — what the kernels that consume alignment paths share (K9 k9_path_stats.hip, K10 k10_window_stats.hip,
// K11 k11_path_text.hip, K12 k12_link_regions.hip): on the host one driver of a call (PathCall), on the device the skeleton
// of a kernel that gives one wavefront to a job over the blocks of one alignment.  The next consumer of paths starts here: K13
// (k13_pileup.hip) takes the driver and the block search, and gives a workgroup to a tile of target columns.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <deque>

#include "device_util.h"
#include "path_stats_host.h"

namespace mimeo {

// a switch from the environment: missing, empty or malformed means the default
inline uint64_t env_u64(const char *name, uint64_t dflt) {
    const char *s = getenv(name);
    if (!s || !*s) return dflt;
    char *end = nullptr;
    const unsigned long long v = strtoull(s, &end, 10);
    return end && *end == 0 ? (uint64_t)v : dflt;
}

inline std::vector<uint64_t> scaffold_lengths(const mimeo_genome *g) {
    std::vector<uint64_t> len(g->scaf.size());
    for (size_t i = 0; i < len.size(); i++) len[i] = g->scaf[i].len;
    return len;
}

// One call of a path consumer, on the caller's stack.  It owns every device buffer and event of the call and releases them
// when it goes out of scope, so every step is HIP_TRY or `return rc`.  The host vectors it copies from outlive the copy on
// every way out: the caller declares its jobs in front of the PathCall and synchronises the stream before it rebuilds them, and
// the destructor's hipFree waits for the device before the view tables here and the caller's vectors go.
struct PathCall {
    static constexpr uint64_t LAUNCH_JOBS = 1ull << 22;   // jobs per launch: 64 MiB of 16-byte jobs, 2^20 workgroups of four
    const hipStream_t st = stream();                      // the calling thread's
    const bool stats;                                     // the caller's *_STATS switch: time the kernels
    // MIMEO_PATH_LAUNCH_JOBS (tests): jobs per launch; 0 or more than the default: the default.  Results do not depend on it.
    const uint64_t launch_jobs = [] { const uint64_t v = env_u64("MIMEO_PATH_LAUNCH_JOBS", LAUNCH_JOBS); return v && v < LAUNCH_JOBS ? v : LAUNCH_JOBS; }();
    double ms_kernel = 0;    // HIP-event time of the launches (stats)
    uint64_t launches = 0;

    explicit PathCall(bool stats_) : stats(stats_) {}
    PathCall(const PathCall &) = delete;
    ~PathCall() {
        for (DeviceBuf *b : {&dvt, &dvqf, &dvqr, &da, &df, &db, &dj}) b->release();
        for (DeviceBuf &b : more) b.release();
        for (hipEvent_t e : ev) if (e) (void)hipEventDestroy(e);
    }
    // a buffer of the caller's own, released with the call
    DeviceBuf &buf() { more.emplace_back(); return more.back(); }

    // the strand views of every scaffold, as the kernels look them up: target forward, query forward, query reverse-complement
    int views(const mimeo_genome *T, const mimeo_genome *Q) {
        vt.resize(T->scaf.size()); vqf.resize(Q->scaf.size()); vqr.resize(Q->scaf.size());
        for (size_t i = 0; i < vt.size(); i++) vt[i] = T->scaf[i].fwd.view(false);
        for (size_t i = 0; i < vqf.size(); i++) { vqf[i] = Q->scaf[i].fwd.view(false); vqr[i] = Q->scaf[i].rc.view(false); }
        int rc;
        if ((rc = dvt.reserve(vt.size() * sizeof(StrandView) + 16)) || (rc = dvqf.reserve(vqf.size() * sizeof(StrandView) + 16)) ||
            (rc = dvqr.reserve(vqr.size() * sizeof(StrandView) + 16)))
            return rc;
        HIP_TRY(hipMemcpyAsync(dvt.p, vt.data(), vt.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dvqf.p, vqf.data(), vqf.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dvqr.p, vqr.data(), vqr.size() * sizeof(StrandView), hipMemcpyHostToDevice, st));
        return 0;
    }
    const StrandView *t_fwd() const { return (const StrandView *)dvt.p; }
    const StrandView *q_fwd() const { return (const StrandView *)dvqf.p; }
    const StrandView *q_rc() const { return (const StrandView *)dvqr.p; }

    // The records [a0, a1) of the call, their path offsets and their blocks.  The stream orders a slice's copies behind the
    // launches that read the slice before; the copies themselves return when the caller's (pageable) memory has been read.
    int slice(const mimeo_alignment *aln, const uint64_t *first, const mimeo_path_block *blocks, uint64_t a0, uint64_t a1) {
        const uint64_t na = a1 - a0, k0 = first[a0], nb = first[a1] - k0;
        int rc;
        if ((rc = da.reserve(na * sizeof(mimeo_alignment))) || (rc = df.reserve((na + 1) * 8)) || (rc = db.reserve(nb * sizeof(mimeo_path_block) + 16)))
            return rc;
        HIP_TRY(hipMemcpyAsync(da.p, aln + a0, na * sizeof(mimeo_alignment), hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(df.p, first + a0, (na + 1) * 8, hipMemcpyHostToDevice, st));
        if (nb) HIP_TRY(hipMemcpyAsync(db.p, blocks + k0, nb * sizeof(mimeo_path_block), hipMemcpyHostToDevice, st));
        return 0;
    }
    const mimeo_alignment *aln() const { return (const mimeo_alignment *)da.p; }
    const uint64_t *first() const { return (const uint64_t *)df.p; }
    const mimeo_path_block *blocks() const { return (const mimeo_path_block *)db.p; }

    // one kernel launch, checked and counted; under `stats` between the two events, its time added to ms_kernel
    template <class Launch>
    int timed(Launch &&launch) {
        if (stats && !ev[0]) { HIP_TRY(hipEventCreate(&ev[0])); HIP_TRY(hipEventCreate(&ev[1])); }
        if (stats) HIP_TRY(hipEventRecord(ev[0], st));
        launch();
        HIP_TRY(hipGetLastError());
        launches++;
        if (stats) {
            float ms = 0;
            HIP_TRY(hipEventRecord(ev[1], st));
            HIP_TRY(hipEventSynchronize(ev[1]));
            HIP_TRY(hipEventElapsedTime(&ms, ev[0], ev[1]));
            ms_kernel += ms;
        }
        return 0;
    }
    // The jobs of a slice, at most launch_jobs per launch (a kernel numbers its jobs in 32 bits): each piece is uploaded and
    // launch(jobs on the device, their number, grid) called for it.  `jobs` stays as it is until the caller has synchronised.
    template <class Job, class Launch>
    int run(const std::vector<Job> &jobs, uint32_t jobs_per_workgroup, Launch &&launch) {
        int rc;
        if ((rc = dj.reserve(std::min<uint64_t>(jobs.size(), launch_jobs) * sizeof(Job)))) return rc;
        for (uint64_t j0 = 0; j0 < jobs.size(); j0 += launch_jobs) {
            const uint32_t nj = (uint32_t)std::min<uint64_t>(launch_jobs, jobs.size() - j0);
            HIP_TRY(hipMemcpyAsync(dj.p, jobs.data() + j0, nj * sizeof(Job), hipMemcpyHostToDevice, st));
            if ((rc = timed([&] { launch((const Job *)dj.p, nj, dim3((nj + jobs_per_workgroup - 1) / jobs_per_workgroup)); }))) return rc;
        }
        return 0;
    }

private:
    std::vector<StrandView> vt, vqf, vqr;
    DeviceBuf dvt, dvqf, dvqr, da, df, db, dj;
    std::deque<DeviceBuf> more;   // a deque: buf() hands out references that stay
    hipEvent_t ev[2] = {nullptr, nullptr};
};

// ---- the device skeleton: one wavefront per job, four per workgroup of 256 -------------------------------------------------

// What a wavefront of K9, K10 or K11 knows before its own work starts: its job, its alignment, the two strands and the
// alignment's blocks [b0, b1) of the slice's.
template <class Job>
struct PathJob {
    Job job;
    uint32_t lane;
    mimeo_alignment a;
    GStrandView T, Q;
    uint64_t b0, b1;
    // false: the wavefront lies behind the last job (wave-uniform)
    __device__ __forceinline__ bool load(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd, const StrandView *__restrict__ q_rc,
                                         const mimeo_alignment *__restrict__ aln, const uint64_t *__restrict__ first, const Job *__restrict__ jobs,
                                         uint32_t njobs) {
        const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);   // wave-uniform
        if (jid >= njobs) return false;
        job = jobs[jid];
        lane = threadIdx.x & 63u;
        a = aln[job.aln];
        // the strand views come out of a device table: into global address space once per wavefront (device_util.h)
        T = GStrandView(t_fwd[a.tid]);
        Q = GStrandView((a.qstrand ? q_rc : q_fwd)[a.qid]);
        b0 = first[job.aln] - first[0];   // the slice's blocks start at first[0]
        b1 = first[job.aln + 1] - first[0];
        return true;
    }
};

// The first block of [lo, hi) that ends behind target base w0; hi where none does.  Every lane that calls it with the same
// arguments takes the same steps.
__device__ __forceinline__ uint64_t first_block_ending_behind(const mimeo_path_block *__restrict__ blocks, uint64_t lo, uint64_t hi, uint32_t w0) {
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        const mimeo_path_block b = blocks[mid];
        if (b.t + b.len > w0) hi = mid; else lo = mid + 1;   // t + len <= the scaffold's length: no wrap in 32 bits
    }
    return lo;
}

// Flattening (K9's header has the why): lane i holds a stretch of `len` columns — a block, or what a window leaves of it; 0
// for a lane without one — and the 64 stretches become one list of (stretch, 64-column chunk) items for the lanes to stride over.
struct ChunkScan { uint32_t incl, excl, total; };   // items up to and with this lane's stretch, in front of it, of all 64
__device__ __forceinline__ ChunkScan scan_chunks(uint32_t len, uint32_t lane) {
    const uint32_t chunks = (len >> 6) + ((len & 63u) ? 1u : 0u);
    uint32_t incl = chunks;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t v = (uint32_t)__shfl_up((int)incl, d);
        if (lane >= (uint32_t)d) incl += v;
    }
    return ChunkScan{incl, incl - chunks, (uint32_t)__shfl((int)incl, 63)};
}
// the stretch of an item = the number of lanes whose inclusive count is <= item (at most 63: item < total = incl of lane 63)
__device__ __forceinline__ uint32_t block_of_item(uint32_t incl, uint32_t item) {
    uint32_t j = 0;
#pragma unroll
    for (uint32_t s = 32; s > 0; s >>= 1)
        if ((uint32_t)__shfl((int)incl, (int)(j + s - 1u)) <= item) j += s;
    return j;
}
// The items [lo, hi) of a pass, hi <= total: chunk(t, q, mask) for each, with t / q the chunk's first base on either strand
// (lane i's stretch starts at st / sq) and mask its columns.
// Bounds: a chunk starts at a base of its stretch, below t + len <= Lt (q + len <= Lq; checked on the host before anything is
// launched), and win64 reads the three words from that base's word on: at most two words behind the strand's last, inside the
// PLANE_PAD = 8 zero words that follow it.  A chunk starts at any alignment mod 64 on either strand: win64 shifts both into place.
template <class Chunk>
__device__ __forceinline__ void for_each_chunk(const ChunkScan &s, uint32_t lane, uint32_t st, uint32_t sq, uint32_t len, uint32_t lo, uint32_t hi,
                                               Chunk &&chunk) {
    for (uint32_t base = lo; base < hi; base += 64) {   // wave-uniform trip count: every lane takes part in the shuffles
        const bool active = base + lane < hi;
        const uint32_t item = active ? base + lane : hi - 1u;
        const uint32_t j = block_of_item(s.incl, item);
        const uint32_t jt = (uint32_t)__shfl((int)st, (int)j), jq = (uint32_t)__shfl((int)sq, (int)j);
        const uint32_t jlen = (uint32_t)__shfl((int)len, (int)j), jex = (uint32_t)__shfl((int)s.excl, (int)j);
        if (active) {
            const uint32_t off = (item - jex) << 6, rem = jlen - off;   // rem >= 1: the chunk starts inside its stretch
            chunk(jt + off, jq + off, rem >= 64u ? ~0ull : (1ull << rem) - 1ull);
        }
    }
}

// A lane's column counters: 32 bits each (a job has fewer than 2^32 columns), reduced once at the end.  The bit planes hold
// the classes (K9's header): ambiguous first, then transversion, transition, match.
struct ColumnCounts : mimeo_column_stats {
    __device__ __forceinline__ ColumnCounts() : mimeo_column_stats{} {}
    __device__ __forceinline__ void count(const Win64 &wt, const Win64 &wq, uint64_t mask) {
        const uint64_t amb = (wt.nm | wq.nm) & mask, ok = mask & ~amb;
        const uint64_t dl = wt.lo ^ wq.lo, dh = wt.hi ^ wq.hi;
        ambiguous += (uint32_t)__popcll(amb);
        transversions += (uint32_t)__popcll(ok & dl);
        transitions += (uint32_t)__popcll(ok & ~dl & dh);
        matches += (uint32_t)__popcll(ok & ~dl & ~dh);
    }
    // the wavefront's sums in every lane, in the order of mimeo_column_stats
    __device__ __forceinline__ void wave_sums(uint32_t c[8]) const {
        const uint32_t v[8] = {matches, transitions, transversions, ambiguous, ins_runs, ins_bases, del_runs, del_bases};
#pragma unroll
        for (int k = 0; k < 8; k++) {
            c[k] = v[k];
            for (int o = 32; o > 0; o >>= 1) c[k] += (uint32_t)__shfl_xor((int)c[k], o);
        }
    }
};

}  // namespace mimeo
