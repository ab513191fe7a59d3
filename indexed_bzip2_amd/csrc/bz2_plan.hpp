/**
 * bz2_plan.hpp -- how a batch is cut up and which kernel forms it runs: pure host arithmetic, no HIP, so that a CPU test
 * (tests/native/plan_cases.cpp) pins every choice.  bz2_device.hip turns the plan into launches.
 *
 * cost = estimated compressed size (distance to the next requested offset, or to the end of the input).
 * The group-start scan (k_hscan<1>) is one serial chain per block: a launch lasts as long as its LARGEST block.
 * Everything behind it (symbols, MTF, BWT, walk, RLE, CRC) is throughput work of about the same size for every block.
 * The batch is therefore cut into groups, each on a HIP stream of its own where the queues allow it (bz2_lanes.hpp),
 * such that the throughput work starts early and never runs dry:
 *   - the "expensive" group: blocks above 45 % of the largest cost, if they are a minority (incompressible blocks
 *     among text).  Its scan starts at once and runs beside everything else on a high-priority stream.
 *   - the other blocks, sorted by cost, in up to MAX_CHUNKS chunks of growing size.  All scans start together; a chunk
 *     of cheap blocks is through early, and its MTF .. RLE kernels run while the later chunks are still being scanned.
 * Inside a group the stage-1 kernels start their largest blocks first (LPT).
 * Slots: group g occupies slots [first[g], +count[g]) of every per-block buffer; results are mapped back to input order.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace bz2gpu
{
constexpr uint32_t MAX_CHUNKS = 3;          /* groups of cheap blocks; each gets a stream only if the context's share
                                               of the hardware queues allows it (bz2_lanes.hpp) */
constexpr int MAX_GROUPS = MAX_CHUNKS + 1;   /* + the expensive group */
constexpr uint32_t BWT_SPLIT_BLOCKS = 640;   /* batches up to this size build their tables with several workgroups per block */
constexpr uint32_t BWT_SPLIT_MAX = 8;        /* most slices per block */
constexpr uint32_t WALK_CHUNK = 256;         /* segments per queue grab */
constexpr uint32_t WALK_WGS_PER_XCD = 128;   /* one or two contexts */
constexpr uint32_t WALK_WGS_CROWD = 32;      /* three or more contexts alive, with claims of 4 x WALK_CHUNK */

/** Kernel forms a test asks for whatever the batch size (MI355X_BZ2_SCAN_WAVES, _BWT_SPLIT, _MTF_NARROW, _MTF_SERIAL), and
 * MI355X_BZ2_NO_SPLIT (one group for the whole batch). */
struct PlanOverrides
{
    uint32_t scanWaves{ 0 };   /* 1 = k_hscan<1>, 4 / 8 = k_hscan_spec<4 / 8>; 0: by batch size */
    uint32_t bwtSplit{ 0 };    /* workgroups per block of the table build (1, 2, 4, 8); 0: by batch size */
    bool mtfNarrow{ false };   /* 256 lanes per block in k_mtf */
    bool noSplit{ false };
    bool mtfSerial{ false };   /* every block through k_mtf's serial pass B, which otherwise sees damaged blocks only */
};

struct BatchPlan
{
    int groups{ 0 };
    int expensive{ -1 };                   /* the group of the expensive minority, -1 if none */
    uint32_t first[MAX_GROUPS]{};          /* first slot of group g */
    uint32_t count[MAX_GROUPS]{};          /* blocks of group g */
    uint32_t scanWaves[MAX_GROUPS]{};      /* 1: k_hscan<1>, 4 / 8: k_hscan_spec<4 / 8> */
    std::vector<uint32_t> slotOf;          /* input index -> slot */
    std::vector<uint64_t> offsets;         /* by slot */
    std::vector<uint32_t> order;           /* by slot: group-relative slots, largest block first */
    bool mtfSide{ false };                 /* the two k_mtf instances of a group side by side on two streams */
    uint32_t mtfSmallLanes{ 256 };         /* lanes per block of k_mtf<MTF_SMALL_STRIDE>: 1 024, 512 or 256 */
    bool mtfSerial{ false };               /* k_mtf's forceSerial argument */
    uint32_t bwtSlices{ 1 };               /* 1: k_bwt_build; more: k_bwt_count + k_bwt_rank with that many per block */
    uint32_t walkWgsPerXcd{ 0 };
    uint32_t walkChunk{ 0 };               /* segments per claim of k_walk */
};

/** `crowd`: three or more contexts alive on the device.  Batches then run side by side (a reader, the bench) and kernels
 * are chosen for the throughput of the crowd; with one or two, for the latency of the batch. */
inline BatchPlan
planBatch( const uint64_t* offsets, uint32_t n, uint64_t inSizeBytes, bool crowd, const PlanOverrides& knobs )
{
    BatchPlan p;
    std::vector<uint64_t> cost( n );
    {
        std::vector<uint32_t> byOffset( n );
        for ( uint32_t i = 0; i < n; ++i ) byOffset[i] = i;
        std::sort( byOffset.begin(), byOffset.end(), [&] ( uint32_t a, uint32_t b ) { return offsets[a] < offsets[b]; } );
        for ( uint32_t k = 0; k < n; ++k ) {
            const uint64_t next = k + 1 < n ? offsets[byOffset[k + 1]] : inSizeBytes * 8;
            const uint64_t cur = offsets[byOffset[k]];
            cost[byOffset[k]] = next > cur ? next - cur : 0;
        }
    }
    uint64_t maxCost = 0;
    for ( const auto v : cost ) maxCost = std::max( maxCost, v );
    const bool split = n >= 64 && !knobs.noSplit;

    std::vector<uint32_t> ascending( n );   /* block indices by increasing cost */
    for ( uint32_t i = 0; i < n; ++i ) ascending[i] = i;
    std::stable_sort( ascending.begin(), ascending.end(), [&] ( uint32_t a, uint32_t b ) { return cost[a] < cost[b]; } );

    uint32_t nExpensive = 0;
    if ( split ) {
        while ( nExpensive < n && cost[ascending[n - 1 - nExpensive]] * 100 > maxCost * 45 ) ++nExpensive;
        if ( nExpensive < 16 || (uint64_t)nExpensive * 100 > (uint64_t)n * 35 ) nExpensive = 0;
    }
    const uint32_t nCheap = n - nExpensive;
    uint32_t nChunks = 1;
    if ( split ) {
        /* measured on MI355X (round 1, and still the right proportion): a lone stage-1 wave takes about 5.5 ns per
         * compressed bit; the kernels behind it together about 0.04 ms per block when the GPU is full */
        const double huffMs = (double)cost[ascending[nCheap - 1]] * 5.5e-6;
        const double restMs = (double)nCheap * 0.04;
        const double ratio = restMs / std::max( huffMs, 1e-3 );
        nChunks = (uint32_t)std::min<double>( { ratio, (double)MAX_CHUNKS, (double)( nCheap / 128 ) } );
        nChunks = std::max( nChunks, 1u );
    }
    p.groups = (int)nChunks + ( nExpensive > 0 ? 1 : 0 );
    p.expensive = nExpensive > 0 ? (int)nChunks : -1;
    {
        /* chunk g ends at rank nCheap * (g + 1)(g + 2) / (K (K + 1)): 1/3, 1 for two chunks; 1/6, 1/2, 1 for three --
         * a small first chunk gets the throughput kernels going early, the later ones keep them fed */
        uint32_t begin = 0;
        for ( uint32_t g = 0; g < nChunks; ++g ) {
            const uint32_t end = (uint32_t)( (uint64_t)nCheap * ( g + 1 ) * ( g + 2 ) / ( (uint64_t)nChunks * ( nChunks + 1 ) ) );
            p.count[g] = end - begin;
            begin = end;
        }
    }
    if ( p.expensive >= 0 ) p.count[p.expensive] = nExpensive;
    for ( int g = 1; g < p.groups; ++g ) p.first[g] = p.first[g - 1] + p.count[g - 1];
    /* slot = rank by cost: group g = ranks [first[g], +count[g]); LPT order inside the group = descending */
    p.slotOf.resize( n );
    p.offsets.resize( n );
    p.order.resize( n );
    for ( uint32_t rank = 0; rank < n; ++rank ) {
        p.slotOf[ascending[rank]] = rank;
        p.offsets[rank] = offsets[ascending[rank]];
    }
    for ( int g = 0; g < p.groups; ++g ) {
        for ( uint32_t k = 0; k < p.count[g]; ++k ) p.order[p.first[g] + k] = p.count[g] - 1 - k;
    }

    /* wavefronts per block: one when the batch fills the GPU by itself; four or eight, each on a group of its own
     * (k_hscan_spec, bz2_hscan.hip.h), when few blocks have to be through quickly (their LDS, one build per wave,
     * allows 4 and 2 blocks per CU).  Measured: sixteen waves gain nothing over eight (the chain from group to
     * group and the barriers grow with the waves); eight are faster than four for ONE batch of 320 blocks (15 vs
     * 18 ms) but slower when four such batches run side by side (14.5 vs 13.4 ms per batch): eight up to 384
     * blocks for a caller with one or two contexts, up to 128 in a crowd */
    /* In a big batch the launch of one wave per block lasts as long as its largest block's chain (34 ms for an
     * incompressible block, against 14.6 ms of average wave life): the expensive minority gets its own waves per
     * group */
    /* (in a crowd -- batches side by side, the scan of one under the other kernels of the rest -- one wave per block
     * from 800 blocks on: a share of 1 270 blocks 37.5 -> 33.4 ms per step, of 960 blocks 28.1 -> 26.7, of 630 blocks
     * 20.2 -> 20.7, profiles/r03_ab_share.txt) */
    for ( int g = 0; g < p.groups; ++g ) {
        uint32_t waves = knobs.scanWaves != 0 ? knobs.scanWaves
                                              : ( n <= ( crowd ? 128u : 384u ) ? 8u : ( n <= ( crowd ? 800u : 1280u ) ? 4u : 1u ) );
        if ( knobs.scanWaves == 0 && waves == 1 && g == p.expensive ) waves = p.count[g] <= 128 ? 8u : 4u;
        p.scanWaves[g] = waves >= 8 ? 8u : ( waves >= 4 ? 4u : 1u );
    }

    /* Every block belongs to one of the two k_mtf instances (by its symbol count), the other returns at once.  In a
     * small batch each lasts as long as its slowest block (4 and 7 ms): side by side instead of one behind the other.
     * (512 lanes per block, each with half the symbols, up to 640 blocks: one batch of 320 blocks 30.4 -> 28.0 ms, but
     * four side by side 11.9 -> 12.1 ms per batch.  The 128-entry lists of 1 024 lanes still fit the LDS of a CU: 152 KB) */
    p.mtfSide = n <= 1280;
    if ( p.mtfSide && n <= ( crowd ? 256u : 640u ) && !knobs.mtfNarrow ) p.mtfSmallLanes = n <= 64 ? 1024u : 512u;
    p.mtfSerial = knobs.mtfSerial;

    /* table build: one workgroup per block when the batch fills the GPU with that (1 024 threads each: 512 at a time);
     * fewer blocks are spread over 2, 4 or 8 workgroups each (a lone block: 1.0 -> 0.3 ms) */
    const uint32_t slices = knobs.bwtSplit != 0 ? std::min( knobs.bwtSplit, BWT_SPLIT_MAX )
                                                : ( n > BWT_SPLIT_BLOCKS ? 1u : ( n > 256 ? 2u : ( n > 128 ? 4u : BWT_SPLIT_MAX ) ) );
    p.bwtSlices = n <= BWT_SPLIT_BLOCKS ? slices : 1u;

    /* measured, walks in turn: four contexts in flight 64 workgroups 67.4 ms per step, 128: 68.6, 256: 72.8; a single context
     * 64: 85.6 ms per batch, 128: 81.0, 256 (walks of the block groups side by side): 84.0 */
    p.walkWgsPerXcd = crowd ? WALK_WGS_CROWD : WALK_WGS_PER_XCD;
    /* Segments per claim.  A lane takes a new segment whenever it has finished one, so a claim has to hold several segments
     * per lane for the lanes to stay busy (segment lengths are geometric: with one segment per lane 22 % of the lanes of a
     * gather instruction are alive, PMC) -- but the segments an XCD has claimed should not span more than a block or two,
     * or its workgroups work on more tables than its L2 holds (claims of 1 024 with 128 workgroups per XCD: FETCH_SIZE of
     * k_walk 14.8 -> 77.6 GB per step).  Workgroups x claim = 32 768 = one block's segments; measured on one box, ms per
     * step (k_walk alone): 128 x 256: 65.1 (17.3), 64 x 256: 63.3 (22.1), 64 x 512: 61.6 (18.7), 32 x 1 024: 60.9 / 62.0 (22.2),
     * 24 x 1 536: 61.6, 16 x 2 048: 65.4.  In a crowd: 32 workgroups per XCD (an eighth of the wave slots) with claims of 1 024. */
    p.walkChunk = crowd && n >= 256 ? 4 * WALK_CHUNK : WALK_CHUNK;
    return p;
}
}  // namespace bz2gpu
