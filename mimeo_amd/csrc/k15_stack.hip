// K15 — the stacked rows of a pile (mimeo_path_stack, include/mimeo_hip.h "pileup v3, the stack"): for every item of a pileup
// one row of text in the coordinates of its window, with the insertion columns of the window's sites opened up — the copies
// behind a consensus laid out as one alignment per family.  What K13 (k13_pileup.hip) reduces to eight counters per column and
// K14 (k14_insertions.hip) to five per insertion column is kept here letter by letter; the host holds no sequence text, so the
// rows are made on the device from the bit planes of the aligned query strand.
//
// A row (stack_host.h): the window's target bases in order, and directly in front of the column of a site's base x the site's
// ncols insertion columns.  Target columns hold A C G T N (the query base under a block), '-' (a gap of the path) or '.' (the
// item does not reach there); insertion columns hold a c g t n (the run that starts at p_k == x, left-aligned) or '.'.
//
// Work layout: K11's.  The kernel lives on its stores, so the unit is the 16-byte group of the row buffer: a lane owns 16
// consecutive bytes at a 16-byte-aligned address and writes them with one 16-byte store; only the groups that hold a row's (or
// a job's) head or tail, which it shares with its neighbours, go out byte by byte.  Every byte is written exactly once: there
// is no memset and no scatter.  One wavefront per job (a row, or job_columns columns of a long one), four per workgroup; the
// lanes stride over the job's groups.  A lane maps its first column to a target base or to (site, j) by binary search over the
// columns of the window's sites (SiteDesc::col, the prefix the host makes: the analogue of K11's bcol), finds the first block
// that ends behind its base (path_call.h) and walks forward through sites, blocks and gaps: a group may cross any number of
// one-column pieces.  Bases to bytes without a branch per base: the pieces of a group are shifted into 16-bit masks (lo, hi, nm
// and the lower-case columns; '-' is nm | lo, '.' is nm | hi), four columns of the masks are spread to the bytes of a selector
// with a multiply, v_perm_b32 picks the letters out of "ACGTN-.", and the lower-case columns get bit 5.
// The letters of a row are counted on the way (mimeo_stack_row.bases): popcounts per lane, one integer atomic per wavefront.
// The output is a function of the sequences, blocks, windows, items and sites alone: independent of the slices, the batches,
// the cut into jobs and the grid.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include <memory>

#include "path_call.h"
#include "stack_host.h"

namespace mimeo {

using stack_host::Job;
using stack_host::RowDesc;
using stack_host::SiteDesc;
using stack_host::WinDesc;

// four columns (bits 0..3 of lo / hi / nm / lc) as four bytes: the selector of column k is lo | hi << 1 | nm << 2 (K11's
// letters4 has the multiply): 0..3 a byte of "ACGT", 4 'N', 5 '-', 6 '.'; a lower-case column gets 0x20
__device__ __forceinline__ uint32_t stack4(uint32_t lo, uint32_t hi, uint32_t nm, uint32_t lc) {
    const uint32_t sel = (((lo & 15u) * 0x00204081u) & 0x01010101u) | ((((hi & 15u) * 0x00204081u) & 0x01010101u) << 1) |
                         ((((nm & 15u) * 0x00204081u) & 0x01010101u) << 2);
    return __builtin_amdgcn_perm(0x002E2D4Eu /* 'N' '-' '.' */, 0x54474341u /* 'A' 'C' 'G' 'T' */, sel) | ((((lc & 15u) * 0x00204081u) & 0x01010101u) << 5);
}

__global__ __launch_bounds__(256) void k15_stack(const StrandView *__restrict__ q_fwd, const StrandView *__restrict__ q_rc,
                                                 const mimeo_alignment *__restrict__ aln, const uint64_t *__restrict__ first,
                                                 const mimeo_path_block *__restrict__ blocks, const WinDesc *__restrict__ wins,
                                                 const SiteDesc *__restrict__ sites, const RowDesc *__restrict__ rows, const Job *__restrict__ jobs,
                                                 uint32_t njobs, uint8_t *__restrict__ out, uint32_t *__restrict__ nbases) {
    const uint32_t jid = __builtin_amdgcn_readfirstlane((blockIdx.x * 256u + threadIdx.x) >> 6);   // wave-uniform
    if (jid >= njobs) return;
    const uint32_t lane = threadIdx.x & 63u;
    const Job job = jobs[jid];
    const RowDesc row = rows[job.row];
    const WinDesc win = wins[row.window];
    const mimeo_alignment a = aln[row.aln];
    const GStrandView Q((a.qstrand ? q_rc : q_fwd)[a.qid]);
    const uint64_t b0 = first[row.aln] - first[0], b1 = first[row.aln + 1] - first[0];   // the slice's blocks start at first[0]
    // the target bases [lo2, hi2) that the item reaches: its window clipped to the alignment; none: both behind every base
    uint32_t lo2 = 0xFFFFFFFFu, hi2 = 0xFFFFFFFFu;
    if (b0 < b1) {
        const mimeo_path_block bf = blocks[b0], bl = blocks[b1 - 1];
        const uint32_t l = max(row.w0, bf.t), h = min(row.w1, bl.t + bl.len);   // t + len <= the scaffold's length: no wrap
        if (l < h) { lo2 = l; hi2 = h; }
    }
    const uint64_t o = row.off;
    const uint64_t lo = o + job.c0, hi = o + job.c1;   // the job's bytes; lo < hi
    uint32_t letters = 0;
    for (uint64_t g = (lo >> 4) + lane; g < ((hi + 15u) >> 4); g += 64) {
        const uint64_t gs = g << 4;
        // the bytes [va, vb) of the group belong to the job: all 16, except at its head and tail
        const uint32_t va = gs < lo ? (uint32_t)(lo - gs) : 0u, vb = gs + 16u > hi ? (uint32_t)(hi - gs) : 16u;
        const uint64_t c = gs + va - o;   // the group's first column
        // where the column lies: the last site of the window whose insertion column 0 is not behind it (SiteDesc::col rises)
        uint32_t sl = win.site0, sh = win.site1;   // sites[sl - 1].col <= c < sites[sh].col
        while (sl < sh) {
            const uint32_t mid = sl + ((sh - sl) >> 1);
            if (sites[mid].col <= c) sl = mid + 1; else sh = mid;
        }
        uint32_t x, ns = sl, ij = 0;   // the next target base; the first site not yet passed; the next column of a site at x
        if (sl == win.site0) x = win.start + (uint32_t)c;
        else {
            const SiteDesc s = sites[sl - 1];
            const uint64_t d = c - s.col;
            if (d < s.ncols) { ns = sl - 1; ij = (uint32_t)d; x = s.x; }
            else x = s.x + (uint32_t)(d - s.ncols);
        }
        // the first block that ends behind x, or behind the item's first base where x lies in front of it; b1 where none does.
        // In front of lo2 and from hi2 on it is not looked at.
        uint64_t k = lo2 != 0xFFFFFFFFu ? first_block_ending_behind(blocks, b0, b1, max(x, lo2)) : b1;
        uint32_t ml = 0, mh = 0, mn = 0, mc = 0;   // bit i: byte i of the group
        uint32_t j = va;
        while (j < vb) {
            const uint32_t left = vb - j;   // 1 .. 16
            uint32_t sx = win.end, sn = 0;
            if (ns < win.site1) { const SiteDesc s = sites[ns]; sx = s.x; sn = s.ncols; }
            uint32_t m;
            if (ns < win.site1 && x == sx) {   // insertion columns ij .. of the site in front of x
                m = min(left, sn - ij);
                uint32_t nl = 0;
                // the run that starts here: x inside the item's window, a block before, p_k == x and dq_k > ij.  Inside [lo2, hi2)
                // k is the first block that ends behind x; outside one of the tests fails (x < w0, x >= w1, k == b0 or k == b1).
                if (x >= row.w0 && x < row.w1 && k > b0 && k < b1) {
                    const mimeo_path_block pb = blocks[k - 1], b = blocks[k];
                    const uint32_t pq = pb.q + pb.len, dq = b.q - pq;
                    if (pb.t + pb.len == x && ij < dq) {
                        nl = min(m, dq - ij);
                        // bounds: an inserted base lies below b.q < Lq (checked on the host); win32 reads its word and the next: at
                        // most one word behind the strand, inside the PLANE_PAD = 8 zero words that follow it
                        const Win32 w = win32(Q, (int32_t)(pq + ij));
                        const uint32_t lm = (1u << nl) - 1u;
                        ml |= (w.lo & ~w.nm & lm) << j; mh |= (w.hi & ~w.nm & lm) << j; mn |= (w.nm & lm) << j; mc |= lm << j;
                        letters += nl;
                    }
                }
                const uint32_t dots = ((1u << m) - 1u) & ~((1u << nl) - 1u);   // behind the run, or no run: '.'
                mh |= dots << j; mn |= dots << j;
                ij += m;
                if (ij == sn) { ns++; ij = 0; }   // on to the column of x itself; the next site lies behind x
            } else {   // target columns from x on, up to the next site's base or the window's end
                const uint32_t mt = min(left, sx - x);
                if (x < lo2 || x >= hi2) {   // the item does not reach there: '.'
                    m = x < lo2 ? min(mt, lo2 - x) : mt;
                    const uint32_t dm = (1u << m) - 1u;
                    mh |= dm << j; mn |= dm << j;
                    x += m;
                } else {   // k < b1: block k ends behind x
                    const mimeo_path_block b = blocks[k];
                    if (x < b.t) {   // a gap of the path: '-'
                        m = min(mt, min(b.t, hi2) - x);
                        const uint32_t dm = (1u << m) - 1u;
                        ml |= dm << j; mn |= dm << j;
                        x += m;
                    } else {   // under the block: the query's letters (bounds as above: the base lies below b.q + b.len <= Lq)
                        m = min(mt, min(b.t + b.len, hi2) - x);
                        const Win32 w = win32(Q, (int32_t)(b.q + (x - b.t)));
                        const uint32_t lm = (1u << m) - 1u;
                        ml |= (w.lo & ~w.nm & lm) << j; mh |= (w.hi & ~w.nm & lm) << j; mn |= (w.nm & lm) << j;
                        letters += m;
                        x += m;
                        if (x == b.t + b.len) k++;
                    }
                }
            }
            if (!m) break;   // never: the host counted the columns from the same windows and sites
            j += m;
        }
        const uint4 v = make_uint4(stack4(ml, mh, mn, mc), stack4(ml >> 4, mh >> 4, mn >> 4, mc >> 4), stack4(ml >> 8, mh >> 8, mn >> 8, mc >> 8),
                                   stack4(ml >> 12, mh >> 12, mn >> 12, mc >> 12));
        if (va == 0 && vb == 16) *(uint4 *)(out + gs) = v;   // gs is a multiple of 16 and the buffer comes from hipMalloc
        else {
            for (uint32_t i = va; i < vb; i++) {
                const uint32_t w = i < 8 ? (i < 4 ? v.x : v.y) : (i < 12 ? v.z : v.w);
                out[gs + i] = (uint8_t)(w >> ((i & 3u) << 3));
            }
        }
    }
    for (int d = 32; d > 0; d >>= 1) letters += (uint32_t)__shfl_xor((int)letters, d);
    if (lane == 0 && letters) atomicAdd(nbases + job.row, letters);
}

static_assert(sizeof(Job) == 24 && sizeof(RowDesc) == 24 && sizeof(SiteDesc) == 16 && sizeof(WinDesc) == 16 && sizeof(mimeo_path_block) == 12 &&
                  sizeof(mimeo_stack_row) == 16,
              "layouts the kernel relies on");

// MIMEO_PATH_STACK_SLICE_BLOCKS: blocks per slice (default 2^24, as K9; 1: every alignment a slice of its own);
// MIMEO_PATH_STACK_BATCH_BYTES: row bytes per device batch (default 2^28; a row goes in whole); MIMEO_PATH_STACK_JOB_COLUMNS:
// columns of a job, at most (default 16384); MIMEO_PATH_STACK_STATS: what the call did and the HIP-event time of its kernels,
// on stderr.  Results depend on none of them.
int path_stack_device(const mimeo_genome *T, const mimeo_genome *Q, const mimeo_alignment *aln, uint64_t n, const uint64_t *first,
                      const mimeo_path_block *blocks, uint64_t nblocks, const mimeo_pileup_window *windows, uint64_t nwin, const mimeo_window_item *items,
                      uint64_t nitems, const mimeo_insert_site *sites, uint64_t nsites, mimeo_stack_row *res, uint64_t **row_first_out, uint8_t **rows_out) {
    // every check on the host, before anything is uploaded: neither a bad path nor a bad window, item or site reaches the kernel
    std::string msg;
    if (!stack_host::validate(scaffold_lengths(T), scaffold_lengths(Q), aln, n, first, blocks, nblocks, windows, nwin, items, nitems, sites, nsites, &msg)) {
        set_error(msg);
        return MIMEO_ERR_ARG;
    }
    // the two arrays of the result: freed on every way out but the last line, which hands them to the caller
    std::unique_ptr<uint64_t, decltype(&free)> row_first((uint64_t *)calloc(nitems + 1, sizeof(uint64_t)), &free);
    if (!row_first) { set_error("mimeo_path_stack: out of host memory"); return MIMEO_ERR_NOMEM; }
    if (!nitems) { *row_first_out = row_first.release(); return 0; }
    const stack_host::Layout L = stack_host::plan_layout(windows, nwin, sites, nsites);
    stack_host::row_first_of(L, items, nitems, row_first.get());
    const uint64_t total = row_first.get()[nitems];
    std::unique_ptr<uint8_t, decltype(&free)> h_rows(total ? (uint8_t *)malloc(total) : nullptr, &free);
    if (total && !h_rows) { set_error("mimeo_path_stack: out of host memory for the rows"); return MIMEO_ERR_NOMEM; }
    if (res)
        for (uint64_t k = 0; k < nitems; k++) {
            res[k] = mimeo_stack_row{0, 0, 0, 0};
            stack_host::query_stretch(first, blocks, items[k], &res[k].q_lo, &res[k].q_hi);
        }
    const uint64_t slice_blocks = std::max<uint64_t>(1, env_u64("MIMEO_PATH_STACK_SLICE_BLOCKS", 1ull << 24));
    const uint64_t slice_records = 1ull << 22;
    const uint64_t batch_bytes = std::max<uint64_t>(1, env_u64("MIMEO_PATH_STACK_BATCH_BYTES", stack_host::DEFAULT_BATCH_BYTES));
    const uint64_t job_columns = env_u64("MIMEO_PATH_STACK_JOB_COLUMNS", stack_host::DEFAULT_JOB_COLUMNS);
    stack_host::Batch batch;   // in front of the call: what it copies from outlives it
    std::vector<uint8_t> stage;
    std::vector<uint32_t> nb;
    PathCall pc(getenv("MIMEO_PATH_STACK_STATS") != nullptr);
    DeviceBuf &dwin = pc.buf(), &dsites = pc.buf(), &drows = pc.buf(), &dout = pc.buf(), &dnb = pc.buf();
    int rc;
    uint64_t njobs_all = 0, nbatches = 0, nslices = 0;
    if (total) {   // no column anywhere: nothing to launch
        if ((rc = pc.views(T, Q)) || (rc = dwin.reserve(nwin * sizeof(WinDesc) + 16)) || (rc = dsites.reserve(nsites * sizeof(SiteDesc) + 16))) return rc;
        HIP_TRY(hipMemcpyAsync(dwin.p, L.win.data(), nwin * sizeof(WinDesc), hipMemcpyHostToDevice, pc.st));
        if (nsites) HIP_TRY(hipMemcpyAsync(dsites.p, L.site.data(), nsites * sizeof(SiteDesc), hipMemcpyHostToDevice, pc.st));
        const auto slices = path_stats_host::plan_slices(first, n, slice_records, slice_blocks);
        std::vector<uint64_t> order, start;
        window_stats_host::bucket_items(slices, items, nitems, order, start);
        for (size_t si = 0; si < slices.size(); si++) {
            bool uploaded = false;
            for (uint64_t i0 = start[si]; i0 < start[si + 1]; i0 = batch.i1) {
                stack_host::plan_batch(L, items, order.data(), slices[si].first, i0, start[si + 1], batch_bytes, job_columns, batch);
                if (batch.jobs.empty()) continue;   // rows without a column
                if (!uploaded && (rc = pc.slice(aln, first, blocks, slices[si].first, slices[si].second))) return rc;
                nslices += !uploaded;
                uploaded = true;
                const size_t nrows = batch.rows.size();
                // the row buffer ends on a whole group and a spare one: a full-group store never crosses its end
                if ((rc = drows.reserve(nrows * sizeof(RowDesc))) || (rc = dout.reserve(((batch.bytes + 15u) & ~15ull) + 16u)) || (rc = dnb.reserve(nrows * 4)))
                    return rc;
                HIP_TRY(hipMemcpyAsync(drows.p, batch.rows.data(), nrows * sizeof(RowDesc), hipMemcpyHostToDevice, pc.st));
                HIP_TRY(hipMemsetAsync(dnb.p, 0, nrows * 4, pc.st));
                rc = pc.run(batch.jobs, 4, [&](const Job *d_jobs, uint32_t nj, dim3 grid) {
                    hipLaunchKernelGGL(k15_stack, grid, dim3(256), 0, pc.st, pc.q_fwd(), pc.q_rc(), pc.aln(), pc.first(), pc.blocks(), (const WinDesc *)dwin.p,
                                       (const SiteDesc *)dsites.p, (const RowDesc *)drows.p, d_jobs, nj, (uint8_t *)dout.p, (uint32_t *)dnb.p);
                });
                if (rc) return rc;
                stage.resize(batch.bytes);
                nb.resize(nrows);
                HIP_TRY(hipMemcpyAsync(stage.data(), dout.p, batch.bytes, hipMemcpyDeviceToHost, pc.st));
                HIP_TRY(hipMemcpyAsync(nb.data(), dnb.p, nrows * 4, hipMemcpyDeviceToHost, pc.st));
                HIP_TRY(hipStreamSynchronize(pc.st));   // the batch is here, and `batch` may be rebuilt
                for (size_t r = 0; r < nrows; r++) {   // every row to its place in the order of the items
                    const uint64_t k = order[batch.i0 + r], w = row_first.get()[k + 1] - row_first.get()[k];
                    if (w) memcpy(h_rows.get() + row_first.get()[k], stage.data() + batch.rows[r].off, w);
                    if (res) res[k].bases = nb[r];
                }
                nbatches++;
                njobs_all += batch.jobs.size();
            }
        }
    }
    if (res)
        for (uint64_t k = 0; k < nitems; k++) {   // the bases of the stretch that have no column
            if (res[k].q_hi == res[k].q_lo) continue;
            res[k].hidden = res[k].q_hi - res[k].q_lo - res[k].bases;
        }
    if (pc.stats && total)
        fprintf(stderr, "[k15] stack: %llu items, %llu sites, %llu bytes, %llu jobs, slices %llu, batches %llu, launches %llu, kernels %.3f ms\n",
                (unsigned long long)nitems, (unsigned long long)nsites, (unsigned long long)total, (unsigned long long)njobs_all, (unsigned long long)nslices,
                (unsigned long long)nbatches, (unsigned long long)pc.launches, pc.ms_kernel);
    *row_first_out = row_first.release();
    *rows_out = h_rows.release();
    return 0;
}

}  // namespace mimeo
