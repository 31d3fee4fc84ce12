// K13 — column pileup of alignment paths and a base called from every column (mimeo_path_pileup, include/mimeo_hip.h "pileup
// v1"): the pile K10 (k10_window_stats.hip) collapses to eight sums per region, kept per column of the target, and the
// consensus letter of every column.  The first consumer of paths that does not reduce over the target axis.
//
// The rules (mimeo_hip.h has them in full), for an item's window [w0, w1) and block b_k with p_k the end of the block before it:
//   a c g t n   per target base x of b_k inside the window: the aligned query strand's base at b_k.q + (x - b_k.t); the N plane
//               decides first; the target's own base plays no part
//   del         per target base of [p_k, b_k.t) inside the window
//   ins_runs, ins_bases   at column p_k where dq_k > 0 and w0 <= p_k < w1: never split, K10's rule
// so every counter is additive over any partition of a window, which is what lets the host cut a window into tiles.
//
// Work layout.  K10 gives a lane a 64-column chunk and reduces; here every column keeps its counters, and a chunk per lane would
// put the 64 lanes on addresses 64 columns apart: one LDS bank.  So it is turned round: the lanes are consecutive columns, and an
// alignment's blocks are walked wave-uniformly.  The host (pileup_host.h) cuts the windows into tiles of TILE columns, buckets
// the items of a slice onto the tiles they touch, clipped to the tile, and a job is a tile with a run of at most JOB_ITEMS of its
// entries.  One workgroup of four wavefronts takes a job: it zeroes the tile's eight counter planes in LDS (32 KiB), the
// wavefronts take the entries round-robin, and for an entry a wavefront finds the first block that ends behind w0 by binary
// search (path_call.h) and goes on 64 blocks per pass — lane i loads block i and the end of the block before it, and the blocks
// that take part (p_k < w1: a prefix, the blocks are ordered) are then broadcast one by one: the lanes are the deleted bases of the
// gap in front of the block, one lane adds the insertion at p_k, and the block's columns go 64 per step: one win64 of the query at
// the wave-uniform start gives the planes, lane j takes bit j, picks its class and adds 1 at counter[class][x - t0], consecutive
// lanes on consecutive banks.  Every LDS add is a non-returning atomic: four wavefronts share the tile.  After a barrier the
// workgroup adds the tile's non-zero counters to the batch's counts in global memory with integer atomics, eight consecutive
// counters of eight consecutive columns per 64 lanes: coalesced, and (the planes are TILE + 8 words apart) free of bank
// conflicts.  A tile may be fed by several jobs, launches and slices; the batch's counts are zeroed once on the stream.
// k13_call then reads a column's eight counts and the target's base and writes the call byte.
// Integers only: exact, and independent of the grid, the slices, the batches, the cut into jobs and the order of the items.
// Coordinates are those of mimeo_path_block; nothing is flipped.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include "path_call.h"
#include "pileup_host.h"

namespace mimeo {

using pileup_host::Entry;
using pileup_host::Job;
using pileup_host::TILE;
using pileup_host::TileDesc;

constexpr uint32_t PLANE = TILE + 8;   // words between two counter planes in LDS: column i of plane c lies on bank (i + 8 c) mod 64
enum { C_N = 4, C_DEL = 5, C_INS_RUNS = 6, C_INS_BASES = 7 };   // the planes, in the order of mimeo_pileup_column; 0 .. 3: A C G T

__global__ __launch_bounds__(256) void k13_pileup(const StrandView *__restrict__ q_fwd, const StrandView *__restrict__ q_rc,
                                                  const mimeo_alignment *__restrict__ aln, const uint64_t *__restrict__ first,
                                                  const mimeo_path_block *__restrict__ blocks, const Entry *__restrict__ entries,
                                                  const Job *__restrict__ jobs, uint32_t njobs, uint32_t *__restrict__ counts) {
    __shared__ uint32_t cnt[8 * PLANE];
    if (blockIdx.x >= njobs) return;   // never: the grid is the number of jobs
    const Job job = jobs[blockIdx.x];
    const uint32_t lane = threadIdx.x & 63u, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    for (uint32_t i = threadIdx.x; i < 8 * PLANE; i += 256) cnt[i] = 0;
    __syncthreads();
    const uint32_t t0 = job.t0;
    for (uint32_t e = wave; e < job.nitems; e += 4) {   // wave-uniform
        const Entry en = entries[job.item0 + e];
        const mimeo_alignment a = aln[en.aln];
        const GStrandView Q((a.qstrand ? q_rc : q_fwd)[a.qid]);
        const uint32_t w0 = en.w0, w1 = en.w1;   // t0 <= w0 < w1 <= t0 + ncols, and inside the alignment (pileup_host.h)
        const uint64_t b0 = first[en.aln] - first[0], b1 = first[en.aln + 1] - first[0];   // the slice's blocks start at first[0]; b1 > b0
        // the first block that ends behind w0: w0 lies in front of the last block's end, so there is one
        const uint64_t ks = first_block_ending_behind(blocks, b0, b1 - 1, w0);
        for (uint64_t p = ks; p < b1; p += 64) {
            const uint64_t idx = p + lane;
            uint32_t bt = 0, bq = 0, blen = 0, pend = 0, dq = 0;
            bool part = false;   // the block takes part: p_k < w1 (the alignment's first block: t < w1)
            if (idx < b1) {
                const mimeo_path_block b = blocks[idx];
                bt = b.t; bq = b.q; blen = b.len;
                pend = b.t;      // the alignment's first block has no gap in front of it
                if (idx > b0) {
                    const mimeo_path_block pb = blocks[idx - 1];
                    pend = pb.t + pb.len;
                    dq = b.q - (pb.q + pb.len);
                }
                part = pend < w1;
            }
            const uint32_t np = (uint32_t)__popcll(__ballot(part));   // p_k rises with k: the blocks that take part are the first np
            for (uint32_t j = 0; j < np; j++) {   // wave-uniform: block p + j in every lane
                const uint32_t jt = (uint32_t)__shfl((int)bt, (int)j), jq = (uint32_t)__shfl((int)bq, (int)j), jlen = (uint32_t)__shfl((int)blen, (int)j);
                const uint32_t jp = (uint32_t)__shfl((int)pend, (int)j), jdq = (uint32_t)__shfl((int)dq, (int)j);
                // the gap in front of the block, [p_k, t) on the target: also that of the first block found, whose p_k is at most w0
                const uint32_t g0 = max(jp, w0), g1 = min(jt, w1);
                for (uint32_t x = g0 + lane; x < g1; x += 64) atomicAdd(&cnt[C_DEL * PLANE + (x - t0)], 1u);
                if (jdq && jp >= w0 && lane == 0) {   // jp < w1: the block takes part
                    atomicAdd(&cnt[C_INS_RUNS * PLANE + (jp - t0)], 1u);
                    atomicAdd(&cnt[C_INS_BASES * PLANE + (jp - t0)], jdq);
                }
                // the block clipped to the window, 64 columns per step.  Bounds of the window read: x is a base of the block, so
                // its query base lies below q + len <= Lq (checked on the host), and win64 reads the three words from that base's
                // word on: at most two words behind the strand's last, inside the PLANE_PAD = 8 zero words that follow it.
                const uint32_t s = max(jt, w0), end = min(jt + jlen, w1);
                for (uint32_t x = s; x < end; x += 64) {
                    const Win64 w = win64(Q, (int32_t)(jq + (x - jt)));
                    if (x + lane < end) {
                        const uint32_t cls = ((w.nm >> lane) & 1ull) ? (uint32_t)C_N : (uint32_t)(((w.lo >> lane) & 1ull) | (((w.hi >> lane) & 1ull) << 1));
                        atomicAdd(&cnt[cls * PLANE + (x + lane - t0)], 1u);
                    }
                }
            }
            if (np < 64) break;   // the first block with p_k >= w1, or the alignment's last, ends the entry
        }
    }
    __syncthreads();
    // the batch's counts are laid out as the output: eight counters per column.  64 lanes: eight columns, on 64 different banks.
    uint32_t *dst = counts + (uint64_t)job.col0 * 8u;
    for (uint32_t i = threadIdx.x; i < (uint32_t)job.ncols * 8u; i += 256) {
        const uint32_t v = cnt[(i & 7u) * PLANE + (i >> 3)];
        if (v) atomicAdd(dst + i, v);
    }
}

// The call byte of every column of a batch (mimeo_hip.h "Call, per column"): one workgroup per tile.
__global__ __launch_bounds__(256) void k13_call(const StrandView *__restrict__ t_fwd, const TileDesc *__restrict__ tiles, uint32_t ntiles,
                                                const uint32_t *__restrict__ counts, uint8_t *__restrict__ call) {
    if (blockIdx.x >= ntiles) return;
    const TileDesc d = tiles[blockIdx.x];
    const GStrandView T(t_fwd[d.tid]);
    for (uint32_t i = threadIdx.x; i < d.ncols; i += 256) {
        const uint4 *c = (const uint4 *)(counts + (uint64_t)(d.col0 + i) * 8u);   // 32 bytes per column in a hipMalloc'ed buffer
        const uint4 base = c[0], rest = c[1];
        const Base1 x0 = base_at(T, (int32_t)(d.t0 + i));   // t0 + i < the scaffold's length (checked on the host)
        const uint32_t own = x0.nm ? 4u : (x0.lo | (x0.hi << 1));
        uint32_t v[4] = {base.x, base.y, base.z, base.w};
        if (own < 4u) v[own]++;
        uint32_t best = 0;
#pragma unroll
        for (uint32_t b = 1; b < 4; b++) if (v[b] > v[best]) best = b;   // among equal votes the order is A, C, G, T ...
        if (own < 4u && v[own] == v[best]) best = own;                   // ... but the target's own base wins a tie it is part of
        const uint32_t vd = rest.y;   // n, del, ins_runs, ins_bases
        call[d.col0 + i] = vd > v[best] ? (uint8_t)'-' : v[best] == 0 ? (uint8_t)'N' : (uint8_t)(0x54474341u /* 'A' 'C' 'G' 'T' */ >> (best << 3));
    }
}

static_assert(sizeof(mimeo_pileup_window) == 12 && sizeof(mimeo_pileup_column) == 32 && sizeof(mimeo_window_item) == 16 && sizeof(Job) == 16 &&
                  sizeof(Entry) == 12 && sizeof(TileDesc) == 16 && sizeof(mimeo_path_block) == 12,
              "layouts the kernels rely on");
static_assert(TILE % 64 == 0 && TILE <= 0xFFFFu && 8 * PLANE * 4 <= 64 * 1024, "the tile: whole wavefronts, Job::ncols, static LDS");

// MIMEO_PILEUP_SLICE_BLOCKS: blocks per slice (default 2^24, as K9; 1: every alignment a slice of its own);
// MIMEO_PILEUP_JOB_ITEMS: entries of a job, at most (default 64); MIMEO_PILEUP_COLUMNS: columns per batch (default 2^22: 128 MiB of
// counts; at most 2^28; a tile goes in whole); MIMEO_PILEUP_STATS: what the call did and the HIP-event time of its kernels, on
// stderr.  Results depend on none of them.
int path_pileup_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                       const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                       uint64_t nitems, mimeo_pileup_column *cols, uint8_t *call) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad window or item reaches the kernels
    std::string msg;
    if (!pileup_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, windows, nwin, items, nitems, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    const pileup_host::Tiles tiles = pileup_host::plan_tiles(windows, nwin);
    if ((!cols && !call) || !tiles.ncols()) return 0;
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_PILEUP_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t job_items = env_u64("MIMEO_PILEUP_JOB_ITEMS", pileup_host::JOB_ITEMS);
    const uint64_t batch_columns = std::min(std::max<uint64_t>(1, env_u64("MIMEO_PILEUP_COLUMNS", 1ull << 22)), pileup_host::MAX_BATCH_COLUMNS);
    const uint64_t run_entries = 1ull << 22;   // entries of one upload: 48 MiB
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    pileup_host::TileItems ti;
    pileup_host::Batch batch;
    PathCall pc(getenv("MIMEO_PILEUP_STATS") != nullptr);
    DeviceBuf &dcnt = pc.buf(), &dcall = pc.buf(), &dtiles = pc.buf(), &dent = pc.buf();
    int rc;
    if ((rc = pc.views(T, Q))) return rc;
    std::vector<std::pair<uint64_t, uint64_t>> slices;
    std::vector<uint64_t> order, start;
    if (nitems) {
        slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
        window_stats_host::bucket_items(slices, items, nitems, order, start);
    }
    uint64_t njobs_all = 0, nbatches = 0, slice_uploads = 0, win = 0;
    for (uint64_t tile0 = 0; tile0 < tiles.ntiles(); tile0 = batch.tile1) {
        while (tiles.tile_first[win + 1] <= tile0) win++;   // the window that holds the tile
        batch = pileup_host::plan_batch(tiles, windows, nwin, win, tile0, batch_columns);
        nbatches++;
        if ((rc = dcnt.reserve(batch.ncols * sizeof(mimeo_pileup_column)))) return rc;
        HIP_TRY(hipMemsetAsync(dcnt.p, 0, batch.ncols * sizeof(mimeo_pileup_column), pc.st));   // once per batch: every job adds to it
        for (size_t si = 0; si < slices.size(); si++) {
            bool uploaded = false;
            for (uint64_t i0 = start[si]; i0 < start[si + 1];) {
                i0 = pileup_host::bucket_tiles(tiles, batch, first, blocks, slices[si].first, windows, items, order.data(), i0, start[si + 1], run_entries, ti);
                if (ti.entries.empty()) continue;   // no item of the run touches the batch: nothing of the slice is uploaded for it
                pileup_host::plan_jobs(batch, ti, job_items, jobs);
                if (!uploaded && (rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
                slice_uploads += !uploaded;
                uploaded = true;
                if ((rc = dent.reserve(ti.entries.size() * sizeof(Entry)))) return rc;
                HIP_TRY(hipMemcpyAsync(dent.p, ti.entries.data(), ti.entries.size() * sizeof(Entry), hipMemcpyHostToDevice, pc.st));
                rc = pc.run(jobs, 1, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
                    hipLaunchKernelGGL(k13_pileup, grid, dim3(256), 0, pc.st, pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), (const Entry *)dent.p,
                                       d_jobs, nj, (uint32_t *)dcnt.p);
                });
                if (rc) return rc;
                HIP_TRY(hipStreamSynchronize(pc.st));   // `jobs` and `ti` are rebuilt for the next run
                njobs_all += jobs.size();
            }
        }
        if (call) {
            const uint32_t nt = (uint32_t)batch.desc.size();   // at most the batch's columns
            if ((rc = dtiles.reserve(nt * sizeof(TileDesc))) || (rc = dcall.reserve(batch.ncols))) return rc;
            HIP_TRY(hipMemcpyAsync(dtiles.p, batch.desc.data(), nt * sizeof(TileDesc), hipMemcpyHostToDevice, pc.st));
            if ((rc = pc.timed([&] {
                    hipLaunchKernelGGL(k13_call, dim3(nt), dim3(256), 0, pc.st, pc.t_fwd(), (const TileDesc *)dtiles.p, nt, (const uint32_t *)dcnt.p, (uint8_t *)dcall.p);
                })))
                return rc;
            HIP_TRY(hipMemcpyAsync(call + batch.col0, dcall.p, batch.ncols, hipMemcpyDeviceToHost, pc.st));
        }
        if (cols) HIP_TRY(hipMemcpyAsync(cols + batch.col0, dcnt.p, batch.ncols * sizeof(mimeo_pileup_column), hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));   // the batch is out, and `batch` may be rebuilt
    }
    if (pc.stats)
        fprintf(stderr, "[k13] pileup: %llu items, %llu windows, %llu columns, %llu tiles, %llu jobs, slices %llu of %zu, batches %llu, launches %llu, kernels %.3f ms\n",
                (unsigned long long)nitems, (unsigned long long)nwin, (unsigned long long)tiles.ncols(), (unsigned long long)tiles.ntiles(),
                (unsigned long long)njobs_all, (unsigned long long)slice_uploads, slices.size(), (unsigned long long)nbatches, (unsigned long long)pc.launches,
                pc.ms_kernel);
    return 0;
}

}  // namespace mimeo
