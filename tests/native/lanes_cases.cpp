/* The stream layout (bz2_lanes.hpp): the queue budget as read from GPU_MAX_HW_QUEUES, a context's share of it, the lanes
 * created with a context and the lanes of batches planned by planBatch, for budgets 1, 2, 4, 8, 16 and 32 and 1 to 8 live
 * contexts, with and without an expensive group and side-by-side k_mtf instances.  Hand-derived layouts are pinned; every
 * case checks the invariants the launcher relies on (a lane for every group below the lane count, a context's lanes
 * within its share, one lane = one group, lanes of the expensive group and of the second k_mtf instances not shared).
 * Prints "lanes ok". */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_lanes.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
const char* currentCase = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 30 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

/* a batch of n blocks laid out back to back: ordinary blocks of `cheapBits`, `nExpensive` of 6 000 000 bits spread evenly */
struct Batch
{
    const char* name;
    uint32_t n;
    uint64_t cheapBits;
    uint32_t nExpensive;
};

BatchPlan
planOf( const Batch& b, bool crowd, bool noSplit )
{
    std::vector<uint64_t> offsets( b.n );
    uint64_t at = 0;
    for ( uint32_t i = 0; i < b.n; ++i ) {
        offsets[i] = at;
        const bool expensive = (uint64_t)( i + 1 ) * b.nExpensive / b.n > (uint64_t)i * b.nExpensive / b.n;
        at += expensive ? 6000000 : b.cheapBits;
    }
    PlanOverrides knobs;
    knobs.noSplit = noSplit;
    return planBatch( offsets.data(), b.n, at / 8, crowd, knobs );
}

/* what the launcher does: the lane budget first, a one-lane context plans without block groups */
void
checkLayout( uint32_t queues, uint32_t live, const Batch& b )
{
    const uint32_t budget = laneBudget( queues, live );
    CHECK( budget >= 1 );
    if ( queues >= live ) CHECK( budget * live <= queues );
    if ( queues < live ) CHECK( budget == 1 );
    const uint32_t atCreation = lanesAtCreation( queues, live );
    CHECK( atCreation >= 1 && atCreation <= budget );
    if ( queues <= DEFAULT_QUEUE_BUDGET ) CHECK( atCreation == 1 );
    const BatchPlan p = planOf( b, live >= 3, budget == 1 );
    const LaneLayout l = layLanes( budget, p );
    CHECK( l.lanes >= 1 && l.lanes <= budget && l.lanes <= MAX_LANES );
    int usedBy[MAX_LANES];   /* group of a group lane, MAX_GROUPS + g for group g's side lane, -1 unused */
    int groupsOn[MAX_LANES]{};
    for ( auto& u : usedBy ) u = -1;
    for ( int g = 0; g < p.groups; ++g ) {
        CHECK( l.laneOf[g] >= 0 && (uint32_t)l.laneOf[g] < l.lanes );
        if ( l.laneOf[g] < 0 || l.laneOf[g] >= (int)MAX_LANES ) continue;
        usedBy[l.laneOf[g]] = g;
        ++groupsOn[l.laneOf[g]];
    }
    for ( int g = 0; g < p.groups; ++g ) {
        const int s = l.sideLaneOf[g];
        if ( s < 0 ) continue;
        CHECK( p.mtfSide );
        CHECK( (uint32_t)s < l.lanes );
        if ( s >= (int)MAX_LANES ) continue;
        CHECK( usedBy[s] == -1 );   /* neither a group's lane nor another group's side lane */
        usedBy[s] = MAX_GROUPS + g;
    }
    for ( uint32_t k = 0; k < l.lanes; ++k ) CHECK( usedBy[k] != -1 );   /* no lane created for nothing */
    CHECK( groupsOn[0] >= 1 );   /* the context's stream carries a group: the join and the output kernels run there */
    if ( budget == 1 ) {
        CHECK( p.groups == 1 );
        CHECK( l.lanes == 1 && l.laneOf[0] == 0 && l.sideLaneOf[0] == -1 && l.highLane == -1 );
    }
    if ( p.expensive >= 0 ) {
        CHECK( l.highLane == l.laneOf[p.expensive] );
        CHECK( groupsOn[l.laneOf[p.expensive]] == 1 );
        CHECK( l.highLane != 0 );
    } else {
        CHECK( l.highLane == -1 );
    }
    if ( p.mtfSide && budget >= 2 * (uint32_t)p.groups ) {
        for ( int g = 0; g < p.groups; ++g ) CHECK( l.sideLaneOf[g] >= 0 );
    }
    /* no two groups share a lane while there are lanes for all of them */
    if ( budget >= (uint32_t)p.groups ) {
        for ( uint32_t k = 0; k < l.lanes; ++k ) CHECK( groupsOn[k] <= 1 );
    }
}
}  // namespace

int
main()
{
    /* GPU_MAX_HW_QUEUES as the runtime reads it */
    currentCase = "queueBudgetOf";
    CHECK( queueBudgetOf( nullptr ) == 4 );
    CHECK( queueBudgetOf( "" ) == 4 );
    CHECK( queueBudgetOf( "queues" ) == 4 );
    CHECK( queueBudgetOf( "0" ) == 1 );
    CHECK( queueBudgetOf( "-3" ) == 1 );
    CHECK( queueBudgetOf( "1" ) == 1 );
    CHECK( queueBudgetOf( "4" ) == 4 );
    CHECK( queueBudgetOf( "16" ) == 16 );
    CHECK( queueBudgetOf( "32" ) == 32 );
    CHECK( queueBudgetOf( "33" ) == 32 );
    CHECK( queueBudgetOf( "99999999999999999999" ) == 32 );

    currentCase = "laneBudget";
    CHECK( laneBudget( 4, 1 ) == 4 );
    CHECK( laneBudget( 4, 2 ) == 2 );
    CHECK( laneBudget( 4, 3 ) == 1 );
    CHECK( laneBudget( 4, 4 ) == 1 );   /* the bench at the runtime's default: one queue per context */
    CHECK( laneBudget( 4, 5 ) == 1 );
    CHECK( laneBudget( 16, 4 ) == 4 );  /* the bench with 16 queues: the layout of the fixed four streams */
    CHECK( laneBudget( 16, 5 ) == 3 );
    CHECK( laneBudget( 32, 1 ) == 32 );
    CHECK( laneBudget( 1, 1 ) == 1 );
    CHECK( laneBudget( 2, 0 ) == 2 );

    currentCase = "lanesAtCreation";
    CHECK( lanesAtCreation( 4, 1 ) == 1 );    /* the default: lanes come with the first batch */
    CHECK( lanesAtCreation( 2, 1 ) == 1 );
    CHECK( lanesAtCreation( 16, 1 ) == 16 );  /* a raised budget: the context's share, now */
    CHECK( lanesAtCreation( 16, 4 ) == 4 );
    CHECK( lanesAtCreation( 8, 3 ) == 2 );
    CHECK( lanesAtCreation( 32, 40 ) == 1 );

    /* pinned layouts */
    const Batch bench{ "bench batch: 2 560 text blocks, 40 incompressible", 2560, 2600000, 40 };
    const Batch text{ "2 560 text blocks", 2560, 2600000, 0 };
    const Batch small{ "320 text blocks, 32 incompressible", 320, 2600000, 32 };
    {
        currentCase = "bench batch, 16 queues, 4 contexts";
        const BatchPlan p = planOf( bench, true, false );
        CHECK( p.groups == 4 && p.expensive == 3 && !p.mtfSide );
        const LaneLayout l = layLanes( laneBudget( 16, 4 ), p );
        CHECK( l.lanes == 4 && l.highLane == 3 );
        CHECK( l.laneOf[0] == 0 && l.laneOf[1] == 1 && l.laneOf[2] == 2 && l.laneOf[3] == 3 );
    }
    {
        currentCase = "bench batch, 4 queues, 2 contexts";
        const BatchPlan p = planOf( bench, false, false );
        const LaneLayout l = layLanes( laneBudget( 4, 2 ), p );
        CHECK( l.lanes == 2 && l.highLane == 1 );
        CHECK( l.laneOf[0] == 0 && l.laneOf[1] == 0 && l.laneOf[2] == 0 && l.laneOf[3] == 1 );
    }
    {
        currentCase = "bench batch, 4 queues, 4 contexts";
        const BatchPlan p = planOf( bench, true, laneBudget( 4, 4 ) == 1 );
        CHECK( p.groups == 1 && p.expensive == -1 );
        const LaneLayout l = layLanes( laneBudget( 4, 4 ), p );
        CHECK( l.lanes == 1 && l.laneOf[0] == 0 && l.highLane == -1 && l.sideLaneOf[0] == -1 );
    }
    {
        currentCase = "text batch, 4 queues, 1 context";
        const BatchPlan p = planOf( text, false, false );
        CHECK( p.groups == 3 && p.expensive == -1 );
        const LaneLayout l = layLanes( laneBudget( 4, 1 ), p );
        CHECK( l.lanes == 3 && l.highLane == -1 );
        CHECK( l.laneOf[0] == 0 && l.laneOf[1] == 1 && l.laneOf[2] == 2 );
    }
    {
        currentCase = "text batch, 2 lanes";
        const BatchPlan p = planOf( text, false, false );
        const LaneLayout l = layLanes( 2, p );
        CHECK( l.lanes == 2 && l.laneOf[0] == 0 && l.laneOf[1] == 1 && l.laneOf[2] == 0 );
    }
    {
        currentCase = "small batch, 16 queues, 1 context";
        const BatchPlan p = planOf( small, false, false );
        CHECK( p.groups == 2 && p.expensive == 1 && p.mtfSide );
        const LaneLayout l = layLanes( laneBudget( 16, 1 ), p );
        CHECK( l.lanes == 4 && l.highLane == 1 );
        CHECK( l.laneOf[0] == 0 && l.laneOf[1] == 1 );
        CHECK( l.sideLaneOf[0] == 2 && l.sideLaneOf[1] == 3 );
    }
    {
        currentCase = "small batch, 3 lanes";
        const BatchPlan p = planOf( small, false, false );
        const LaneLayout l = layLanes( 3, p );
        CHECK( l.lanes == 3 && l.sideLaneOf[0] == 2 && l.sideLaneOf[1] == -1 );
    }
    {
        currentCase = "small batch, one lane";
        const BatchPlan p = planOf( small, false, true );
        CHECK( p.groups == 1 && p.mtfSide );
        const LaneLayout l = layLanes( 1, p );
        CHECK( l.lanes == 1 && l.sideLaneOf[0] == -1 );
    }
    {
        currentCase = "split plan given one lane";
        const BatchPlan p = planOf( bench, false, false );
        const LaneLayout l = layLanes( 1, p );
        CHECK( l.lanes == 1 && l.highLane == -1 );
        for ( int g = 0; g < p.groups; ++g ) CHECK( l.laneOf[g] == 0 && l.sideLaneOf[g] == -1 );
    }

    /* invariants over the whole grid */
    const Batch batches[] = {
        bench, text, small,
        { "one block", 1, 2600000, 0 },
        { "64 uniform blocks", 64, 6000000, 0 },
        { "640 text blocks, 64 incompressible", 640, 2600000, 64 },
        { "1 280 text blocks", 1280, 2600000, 0 },
        { "1 281 text blocks, 200 incompressible", 1281, 2600000, 200 },
    };
    int cases = 0;
    for ( const uint32_t queues : { 1u, 2u, 4u, 8u, 16u, 32u } ) {
        for ( uint32_t live = 1; live <= 8; ++live ) {
            for ( const Batch& b : batches ) {
                currentCase = b.name;
                checkLayout( queues, live, b );
                ++cases;
            }
        }
    }
    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "lanes ok (%d layouts)\n", cases );
    return 0;
}
