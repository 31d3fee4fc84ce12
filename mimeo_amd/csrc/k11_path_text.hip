// K11 — the text of alignment paths (mimeo_path_text, include/mimeo_hip.h): for every alignment the two rows of its
// pairwise alignment, target over query, as letters — what a MAF block and a cs:Z: tag are written from.  The host holds no
// sequence text (Genome.from_fasta streams it to the device), so the rows are made here, from the bit planes.
//
// A row (path_text_host.h): for every block b_k, k > 0, the dq insertion columns ('-' over the query bases) and then the dt
// deletion columns (the target bases over '-') of the jump from b_{k-1}, then the len columns of b_k.  Letters: A C G T, N
// for every base that is not one of them — decided by the nm plane first, as in K9; the planes keep neither case nor IUPAC
// codes.  Coordinates are those of mimeo_path_block: t on the target's forward strand, q on the query's forward strand or,
// for qstrand == 1, on its stored reverse-complement strand (Scaffold::rc).  Nothing is flipped here.
//
// Work layout: the kernel lives on its stores, and a byte or short store costs about as much as a 16-byte one.  So the unit
// is the 16-byte group of the output: a lane owns 16 consecutive columns at a 16-byte-aligned byte of the row buffers and
// writes them with one 16-byte store per row; only the groups that hold a row's head or tail, which it shares with its
// neighbours' rows, go out byte by byte.  One wavefront per job (a row, or split_columns columns of a long one, cut at
// multiples of 16 output bytes), four per workgroup; the lanes stride over the job's groups, so a wavefront's stores are 1 KiB
// of consecutive bytes.  A lane finds the block that holds its first column by binary search of the blocks' column starts
// (bcol, a prefix sum the host makes) and walks on from there: a group may cross any number of one-column blocks and gaps.
// Bases to bytes without a branch per base or a table in memory: the pieces of a group are shifted into six 16-bit masks
// (lo, hi, nm of either row; a gap column is nm | lo), four columns of the masks are spread to the bytes of a selector with
// a multiply, and v_perm_b32 picks the letters out of the eight bytes "ACGTN-".
// The output is a function of the sequences and the blocks alone: independent of the slices, of the cut into jobs and of
// the grid.
#include <algorithm>
#include <cstdio>
#include <cstdlib>

#include <memory>

#include "path_call.h"
#include "path_text_host.h"

namespace mimeo {

using path_text_host::Job;

// four columns (bits 0..3 of lo / hi / nm) as four letters: bit k of x * 0x00204081 lands on bit 8k (the four shifted copies
// occupy bits [7k, 7k + 3] and never meet), so the selector byte of column k is lo | hi << 1 | nm << 2 = 0..5
__device__ __forceinline__ uint32_t letters4(uint32_t lo, uint32_t hi, uint32_t nm) {
    const uint32_t sel = (((lo & 15u) * 0x00204081u) & 0x01010101u) | ((((hi & 15u) * 0x00204081u) & 0x01010101u) << 1) |
                         ((((nm & 15u) * 0x00204081u) & 0x01010101u) << 2);
    // selector 0..3: a byte of the second operand "ACGT"; 4, 5: of the first, "N-"
    return __builtin_amdgcn_perm(0x00002D4Eu /* 'N' '-' */, 0x54474341u /* 'A' 'C' 'G' 'T' */, sel);
}
__device__ __forceinline__ uint4 letters16(uint32_t lo, uint32_t hi, uint32_t nm) {
    return make_uint4(letters4(lo, hi, nm), letters4(lo >> 4, hi >> 4, nm >> 4), letters4(lo >> 8, hi >> 8, nm >> 8),
                      letters4(lo >> 12, hi >> 12, nm >> 12));
}
__device__ __forceinline__ uint32_t byte_of(const uint4 &v, uint32_t x) {   // x < 16
    const uint32_t w = x < 8 ? (x < 4 ? v.x : v.y) : (x < 12 ? v.z : v.w);
    return (w >> ((x & 3u) << 3)) & 0xFFu;
}

__global__ __launch_bounds__(256) void k11_path_text(const StrandView *__restrict__ t_fwd, const StrandView *__restrict__ q_fwd,
                                                     const StrandView *__restrict__ q_rc, const mimeo_alignment *__restrict__ aln,
                                                     const uint64_t *__restrict__ first, const mimeo_path_block *__restrict__ blocks,
                                                     const uint64_t *__restrict__ bcol, const uint64_t *__restrict__ rowoff, uint32_t lead,
                                                     const Job *__restrict__ jobs, uint32_t njobs, uint8_t *__restrict__ trow,
                                                     uint8_t *__restrict__ qrow) {
    PathJob<Job> J;
    if (!J.load(t_fwd, q_fwd, q_rc, aln, first, jobs, njobs)) return;
    const Job job = J.job;
    const GStrandView &T = J.T, &Q = J.Q;
    const uint64_t b0 = J.b0, b1 = J.b1;
    // byte of the row buffers that holds column 0 of this row: the slice's rows lie as in the output arrays, behind `lead`
    // bytes that give the buffers the output's alignment mod 16
    const uint64_t o = lead + (rowoff[job.aln] - rowoff[0]);
    const uint64_t lo = o + job.c0, hi = o + job.c1;   // the job's bytes; lo < hi, and b0 < b1: a row with columns has blocks
    for (uint64_t g = (lo >> 4) + J.lane; g < ((hi + 15u) >> 4); g += 64) {
        const uint64_t gs = g << 4;
        // the bytes [va, vb) of the group belong to the job: all 16, except at a row's head and tail
        const uint32_t va = gs < lo ? (uint32_t)(lo - gs) : 0u, vb = gs + 16u > hi ? (uint32_t)(hi - gs) : 16u;
        const uint64_t c = gs + va - o;   // the group's first column
        // the last block k with bcol[k] <= c: its region [bcol[k], bcol[k + 1]) holds the column (bcol[b0] == 0, and bcol rises)
        uint64_t k = b0, kh = b1;
        while (kh - k > 1) {
            const uint64_t mid = (k + kh) >> 1;
            if (bcol[mid] <= c) k = mid; else kh = mid;
        }
        mimeo_path_block b = blocks[k];
        uint32_t pt = 0, pq = 0, dq = 0, dt = 0;   // end of the block before, and the jump from it
        if (k > b0) {
            const mimeo_path_block pb = blocks[k - 1];
            pt = pb.t + pb.len; pq = pb.q + pb.len;
            dq = b.q - pq; dt = b.t - pt;
        }
        uint64_t off = c - bcol[k];   // column inside the region: below dq + dt + len < 2^33
        uint32_t tl = 0, th = 0, tn = 0, ql = 0, qh = 0, qn = 0;   // bit x: byte x of the group
        uint32_t j = va;
        for (;;) {
            const uint32_t left = vb - j;   // 1 .. 16
            uint32_t m;
            // bounds of the window reads: a piece starts at a base of its strand — an inserted base lies in [pq, b.q), a deleted
            // one in [pt, b.t), a block's in [t, t + len) with t + len <= Lt and q + len <= Lq (checked on the host before anything
            // is launched) — so its word is at most the strand's last, also for a lane whose columns end on a block's last
            // base; win32 reads that word and the next: one word behind the strand, inside the PLANE_PAD = 8 zero words that
            // follow it.  Only the low m <= 16 bits of the 32 are used.
            if (off < dq) {   // insertion columns: '-' over query bases
                m = (uint32_t)min((uint64_t)left, dq - off);
                const uint32_t mask = (1u << m) - 1u;
                const Win32 w = win32(Q, (int32_t)(pq + (uint32_t)off));
                tl |= mask << j; tn |= mask << j;
                ql |= (w.lo & ~w.nm & mask) << j; qh |= (w.hi & ~w.nm & mask) << j; qn |= (w.nm & mask) << j;
            } else if (off < (uint64_t)dq + dt) {   // deletion columns: target bases over '-'
                const uint64_t d = off - dq;
                m = (uint32_t)min((uint64_t)left, dt - d);
                const uint32_t mask = (1u << m) - 1u;
                const Win32 w = win32(T, (int32_t)(pt + (uint32_t)d));
                ql |= mask << j; qn |= mask << j;
                tl |= (w.lo & ~w.nm & mask) << j; th |= (w.hi & ~w.nm & mask) << j; tn |= (w.nm & mask) << j;
            } else {   // the block's diagonal
                const uint32_t d = (uint32_t)(off - dq - dt);
                m = min(left, b.len - d);
                const uint32_t mask = (1u << m) - 1u;
                const Win32 wt = win32(T, (int32_t)(b.t + d)), wq = win32(Q, (int32_t)(b.q + d));
                tl |= (wt.lo & ~wt.nm & mask) << j; th |= (wt.hi & ~wt.nm & mask) << j; tn |= (wt.nm & mask) << j;
                ql |= (wq.lo & ~wq.nm & mask) << j; qh |= (wq.hi & ~wq.nm & mask) << j; qn |= (wq.nm & mask) << j;
            }
            j += m;
            if (j >= vb) break;
            off += m;
            if (off == (uint64_t)dq + dt + b.len) {   // on to the next block: there is one, the row has columns left
                if (++k >= b1) break;                 // (never: the host counted the columns from the same blocks)
                pt = b.t + b.len; pq = b.q + b.len;
                b = blocks[k];
                dq = b.q - pq; dt = b.t - pt;
                off = 0;
            }
        }
        const uint4 tv = letters16(tl, th, tn), qv = letters16(ql, qh, qn);
        if (va == 0 && vb == 16) {   // gs is a multiple of 16 and the buffers come from hipMalloc
            *(uint4 *)(trow + gs) = tv;
            *(uint4 *)(qrow + gs) = qv;
        } else {
            for (uint32_t x = va; x < vb; x++) {
                trow[gs + x] = (uint8_t)byte_of(tv, x);
                qrow[gs + x] = (uint8_t)byte_of(qv, x);
            }
        }
    }
}

static_assert(sizeof(Job) == 24 && sizeof(mimeo_path_block) == 12, "layouts the kernel relies on");

// MIMEO_PATH_TEXT_SLICE_COLUMNS: output columns per slice (default 2^28: two row buffers of 256 MiB; 1: every alignment a
// slice of its own); MIMEO_PATH_TEXT_SPLIT_COLUMNS: a row of more columns than this is cut into jobs of this many (default
// 16384; 0: never); MIMEO_PATH_TEXT_STATS: what the call did and the HIP-event time of its kernels, on stderr.  Results depend
// on none of them.
int path_text_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                     const mimeo_path_block *blocks, uint64_t nblocks, uint64_t **row_first_out, uint8_t **trow_out, uint8_t **qrow_out) {
    // every check on the host, before anything is uploaded: a bad path never reaches the kernel
    std::string msg;
    if (!path_text_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, &msg)) { set_error(msg); return MIMEO_ERR_ARG; }
    // the three arrays of the result: freed on every way out but the last line, which hands them to the caller
    std::unique_ptr<uint64_t, decltype(&free)> row_first((uint64_t *)malloc((n + 1) * sizeof(uint64_t)), &free);
    if (!row_first) { set_error("mimeo_path_text: out of host memory"); return MIMEO_ERR_NOMEM; }
    path_text_host::row_first_of(first, blocks, n, row_first.get());
    const uint64_t total = row_first.get()[n];
    std::unique_ptr<uint8_t, decltype(&free)> h_t(total ? (uint8_t *)malloc(total) : nullptr, &free), h_q(total ? (uint8_t *)malloc(total) : nullptr, &free);
    if (total && (!h_t || !h_q)) { set_error("mimeo_path_text: out of host memory for the rows"); return MIMEO_ERR_NOMEM; }
    const uint64_t slice_columns = std::max<uint64_t>(1, env_u64("MIMEO_PATH_TEXT_SLICE_COLUMNS", path_text_host::DEFAULT_SLICE_COLUMNS));
    const uint64_t split_columns = env_u64("MIMEO_PATH_TEXT_SPLIT_COLUMNS", path_text_host::DEFAULT_SPLIT_COLUMNS);
    std::vector<Job> jobs;   // in front of the call: what it copies from outlives it
    std::vector<uint64_t> bcol;
    PathCall pc(getenv("MIMEO_PATH_TEXT_STATS") != nullptr);
    DeviceBuf &dc = pc.buf(), &dr = pc.buf(), &dtrow = pc.buf(), &dqrow = pc.buf();
    int rc;
    if (total && (rc = pc.views(T, Q))) return rc;   // no column anywhere: nothing to launch
    const auto slices = path_text_host::plan_slices(row_first.get(), first, n, path_text_host::SLICE_RECORDS, path_text_host::SLICE_BLOCKS, slice_columns);
    uint64_t njobs_all = 0, nslices = 0;
    for (const auto &s : slices) {
        const uint64_t a0 = s.first, na = s.second - s.first, nb = first[s.second] - first[a0];
        const uint64_t col0 = row_first.get()[a0], cols = row_first.get()[s.second] - col0;
        if (!cols) continue;   // a slice of alignments without columns
        const uint32_t lead = (uint32_t)(col0 & 15u);
        path_text_host::plan_jobs(row_first.get(), a0, s.second, split_columns, jobs);
        path_text_host::block_columns(first, blocks, a0, s.second, bcol);
        const size_t row_bytes = (size_t)(((lead + cols + 15u) & ~15ull) + 16u);
        if ((rc = pc.slice(aln, first, blocks, a0, s.second)) || (rc = dr.reserve((na + 1) * 8)) || (rc = dc.reserve(nb * 8 + 16)) ||
            (rc = dtrow.reserve(row_bytes)) || (rc = dqrow.reserve(row_bytes)))
            return rc;
        HIP_TRY(hipMemcpyAsync(dr.p, row_first.get() + a0, (na + 1) * 8, hipMemcpyHostToDevice, pc.st));
        HIP_TRY(hipMemcpyAsync(dc.p, bcol.data(), nb * 8, hipMemcpyHostToDevice, pc.st));
        rc = pc.run(jobs, 4, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
            hipLaunchKernelGGL(k11_path_text, grid, dim3(256), 0, pc.st, pc.t_fwd(), pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(),
                               (const uint64_t *)dc.p, (const uint64_t *)dr.p, lead, d_jobs, nj, (uint8_t *)dtrow.p, (uint8_t *)dqrow.p);
        });
        if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(h_t.get() + col0, (const uint8_t *)dtrow.p + lead, cols, hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipMemcpyAsync(h_q.get() + col0, (const uint8_t *)dqrow.p + lead, cols, hipMemcpyDeviceToHost, pc.st));
        HIP_TRY(hipStreamSynchronize(pc.st));   // the rows are here, and `jobs` and `bcol` may be rebuilt for the next slice
        nslices++;
        njobs_all += jobs.size();
    }
    if (pc.stats && total)   // a call without columns has launched nothing and says nothing
        fprintf(stderr, "[k11] path text: %llu alignments, %llu columns, %llu jobs, slices %llu, kernels %.3f ms\n", (unsigned long long)n,
                (unsigned long long)total, (unsigned long long)njobs_all, (unsigned long long)nslices, pc.ms_kernel);
    *row_first_out = row_first.release();
    *trow_out = h_t.release();
    *qrow_out = h_q.release();
    return 0;
}

}  // namespace mimeo
