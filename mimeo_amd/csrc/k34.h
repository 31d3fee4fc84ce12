// k34.h — what the extension batch (k4_extend.hip) sees of K34, the fused seed scan (k34_fused.hip): the plan of its split pass,
// the device buffers that are K34's alone, and its launches.
#pragma once
#include <vector>

#include "k4_device.h"

namespace mimeo {

struct HeavyPlan {                       // the listed tiles of one launch, dense (k34_plan)
    const unsigned long long *est;       // per listed slot (unit * NTILE + i): the first pass's estimate of the tile's hits
    uint2 *tile;                         // dense k -> (unit index in the launch, tile)
    uint32_t *base;                      // dense k -> first part; base[ntiles] = all parts
    uint4 *split;                        // dense k -> (target shares, query ranges, entries per query range, 0)
    unsigned int *ctr;                   // [0] parts handed out, [1] listed tiles, [2] parts
};

// grid.y limit: K34 and the walk-queue kernel behind it take the batch's units this many to a launch
constexpr uint32_t K34_LAUNCH_UNITS = 32768;

// K34's own buffers of a batch.  They only ever grow; prepare() carves them for the batch's units.
struct K34Buffers {
    DeviceBuf lists;      // per unit NTILE slots: the estimates of the tiles the first pass listed (8 bytes), then their numbers (4)
    DeviceBuf plan_buf;   // the split pass's plan of one launch: splits, tiles, part bases, three counters
    DeviceBuf counters;   // per unit: the walk queue's 8 shard counters; behind them, per unit, the number of listed tiles
    HeavyPlan plan = {};
    uint32_t nactive = 0;
    // room for the units of the table, the counters zeroed on st; q gets the kernels' view: nwalk_u, nheavy_u, heavy, heavy_est.
    // MIMEO_ERR_NOMEM when the device has no room (the caller may cut the batch)
    int prepare(const std::vector<FusedUnit> &units, ExtQueues &q, hipStream_t st);
    // the split pass of the batch's last launch: tiles listed, slots they were listed in, parts, hits aimed at per part
    int split_stats(unsigned int *tiles, unsigned int *slots, unsigned int *parts, unsigned long long *part_hits) const;
    void release();
};

// both passes over the `K.nactive` units of the table d_units, K34_LAUNCH_UNITS to a launch; dbg: MIMEO_K34_DEBUG (16, 32)
int launch_fused_batch(const K34Buffers &K, const FusedUnit *d_units, const ExtQueues &q, const mimeo_params *p, hipStream_t st, uint32_t dbg);
// unit_hits[u] = sum of the unit's tile counts (once per batch)
void launch_sum_hits(const ExtQueues &q, uint32_t nunits, hipStream_t st);

}  // namespace mimeo
