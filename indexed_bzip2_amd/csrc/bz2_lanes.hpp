/**
 * bz2_lanes.hpp -- which HIP streams ("lanes") a batch runs on: pure host arithmetic, no HIP, so that a CPU test
 * (tests/native/lanes_cases.cpp) pins every choice.  bz2_device.hip creates the streams and launches by lane.
 *
 * The HIP runtime maps streams onto at most GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says otherwise).
 * A queue runs its packets in order, whichever stream queued them: streams that share a queue run one after the other,
 * and a cross-stream wait on a shared queue stops every stream behind it.  A context therefore gets its share of the
 * queues, not more:
 *   - lanes = queues / live contexts on the device (at least one);
 *   - one lane: the batch is not cut into block groups (planBatch with noSplit), both k_mtf instances run on the
 *     context's stream;
 *   - more: the expensive group gets a lane of its own (high priority), the cheap chunks share the others in turn, and
 *     lanes that are left over carry the second k_mtf instance of a group (small batches, BatchPlan::mtfSide).
 * Lane 0 is the context's stream; the join and the output kernels run there.  Input copies keep a stream of their own
 * whatever the lanes (bz2_device.hip, queueInput).
 */
#pragma once

#include <cstdint>
#include <cstdlib>

#include "bz2_plan.hpp"

namespace bz2gpu
{
constexpr uint32_t DEFAULT_QUEUE_BUDGET = 4;     /* the HIP runtime's default */
constexpr uint32_t MAX_QUEUE_BUDGET = 32;
constexpr uint32_t MAX_LANES = 2 * MAX_GROUPS;   /* a lane per group and one per group's second k_mtf instance */

/** GPU_MAX_HW_QUEUES as the runtime reads it: unset or not a number -> 4, else clamped to 1..32. */
inline uint32_t
queueBudgetOf( const char* value )
{
    if ( value == nullptr || value[0] == '\0' ) return DEFAULT_QUEUE_BUDGET;
    char* end = nullptr;
    const long v = std::strtol( value, &end, 10 );
    if ( end == value ) return DEFAULT_QUEUE_BUDGET;
    return v < 1 ? 1u : ( v > (long)MAX_QUEUE_BUDGET ? MAX_QUEUE_BUDGET : (uint32_t)v );
}

/** The lanes a context may use while `liveContexts` contexts are alive on its device. */
inline uint32_t
laneBudget( uint32_t queueBudget, uint32_t liveContexts )
{
    const uint32_t share = queueBudget / ( liveContexts > 0 ? liveContexts : 1u );
    return share > 0 ? share : 1u;
}

/** The lanes a context creates with itself rather than with its first batch.  The runtime gives a new stream a queue of
 * its own while it has fewer than its budget, and then the least used one: streams created first get the queues.  When
 * the budget has been raised above the default, the contexts' lanes are created before the input, scan and copy streams
 * (created on first use), so that these are the ones that share (the four-context bench with 16 queues: 58.8-59.3 ms per
 * step; lanes created with the first batch: 75.6-90.1).  At the default a context alone would take queues that the
 * contexts created after it need for their own streams: lanes come with the first batch. */
inline uint32_t
lanesAtCreation( uint32_t queueBudget, uint32_t liveContexts )
{
    return queueBudget > DEFAULT_QUEUE_BUDGET ? laneBudget( queueBudget, liveContexts ) : 1u;
}

struct LaneLayout
{
    uint32_t lanes{ 1 };               /* lanes this batch uses, <= the budget */
    int laneOf[MAX_GROUPS]{};          /* lane of group g */
    int sideLaneOf[MAX_GROUPS]{};      /* lane of group g's second k_mtf instance; -1: on laneOf[g], behind the first */
    int highLane{ -1 };                /* the expensive group's lane (a high-priority stream); -1 if none */
};

/** The lanes of a batch planned by planBatch, within `budget` lanes (laneBudget).  A budget of one expects a plan made
 * with noSplit; a split plan then runs on lane 0 as a whole. */
inline LaneLayout
layLanes( uint32_t budget, const BatchPlan& p )
{
    LaneLayout l;
    const int groups = p.groups > 0 ? p.groups : 1;
    for ( int g = 0; g < MAX_GROUPS; ++g ) {
        l.laneOf[g] = 0;
        l.sideLaneOf[g] = -1;
    }
    if ( budget <= 1 ) return l;
    const bool expensive = p.expensive >= 0 && groups >= 2;
    const uint32_t cheap = (uint32_t)groups - ( expensive ? 1u : 0u );
    const uint32_t cheapLanes = cheap < budget - ( expensive ? 1u : 0u ) ? cheap : budget - ( expensive ? 1u : 0u );
    uint32_t used = cheapLanes;
    for ( int g = 0, k = 0; g < groups; ++g ) {
        if ( expensive && g == p.expensive ) continue;
        l.laneOf[g] = (int)( (uint32_t)k++ % cheapLanes );
    }
    if ( expensive ) {
        l.highLane = (int)used++;
        l.laneOf[p.expensive] = l.highLane;
    }
    if ( p.mtfSide ) {
        for ( int g = 0; g < groups && used < budget; ++g ) l.sideLaneOf[g] = (int)used++;
    }
    l.lanes = used;
    return l;
}
}  // namespace bz2gpu
