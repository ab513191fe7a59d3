/* The scratch layout of a decoder context (bz2_scratch.hpp): for the capacities that batches of 1 to
 * MI355X_BZ2_MAX_BATCH_BLOCKS blocks reach, with and without MI355X_BZ2_FLAG_KEEP_STAGES, every region starts at a
 * multiple of 256 bytes inside its allocation and no two regions of one allocation overlap, except exactly the two
 * declared pairs (dSym in dStash; dR in dL without KEEP_STAGES), where the guest is no larger than its host.  The totals
 * are pinned as numbers taken from the hand-written arithmetic that the list replaced, so that a transcription error in
 * the list cannot pass.  Prints "scratch ok". */
#include <cstdio>
#include <cstdlib>

#include "../../include/mi355x_bz2.h"
#include "../../indexed_bzip2_amd/csrc/bz2_scratch.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
char currentCase[64] = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 30 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

/* sizeof( BlockMeta ), ( HuffMeta ), ( ScanMeta ), ( HuffTables ), ( WalkPlan ): bz2_device.hip pins the same values */
constexpr ScratchSizes SIZES{ 88, 16, 32, 17216, 160 };

const char* const NAMES[] = {
#define NAME( memory, name, ... ) #name,
    BZ2_SCRATCH_REGIONS( NAME )
#undef NAME
};

/* the rule in words: 8 up, powers of two to 512, then multiples of 256 */
uint32_t
capacityByRule( uint32_t nBlocks )
{
    for ( uint32_t cap = 8; cap <= 512; cap *= 2 ) {
        if ( nBlocks <= cap ) return cap;
    }
    return ( nBlocks + 255 ) / 256 * 256;
}

void
checkLayout( uint32_t cap, bool keepStages )
{
    std::snprintf( currentCase, sizeof( currentCase ), "cap %u%s", cap, keepStages ? ", KEEP_STAGES" : "" );
    const ScratchLayout l = layScratch( cap, keepStages, SIZES );
    CHECK( l.capacity == cap );
    CHECK( l.deviceBytes % 256 == 0 && l.hostBytes % 256 == 0 );
    int aliases = 0;
    for ( int r = 0; r < SCRATCH_REGIONS; ++r ) {
        const uint64_t total = l.host[r] ? l.hostBytes : l.deviceBytes;
        CHECK( l.host[r] == ( NAMES[r][0] == 'h' ) );
        CHECK( l.bytes[r] > 0 );
        CHECK( l.offset[r] % 256 == 0 );
        CHECK( l.offset[r] + l.bytes[r] <= total );
        const int a = l.aliasOf[r];
        if ( a >= 0 ) {
            ++aliases;
            CHECK( a < r && l.aliasOf[a] < 0 && l.host[a] == l.host[r] );
            CHECK( l.offset[r] == l.offset[a] && l.bytes[r] <= l.bytes[a] );
        }
        for ( int q = 0; q < r; ++q ) {
            if ( l.host[q] != l.host[r] ) continue;
            const bool overlap = l.offset[q] < l.offset[r] + l.bytes[r] && l.offset[r] < l.offset[q] + l.bytes[q];
            if ( overlap != ( a == q ) ) std::printf( "%s: %s and %s\n", currentCase, NAMES[q], NAMES[r] );
            CHECK( overlap == ( a == q ) );
        }
    }
    /* exactly the declared pairs */
    CHECK( l.aliasOf[R_dSym] == R_dStash );
    CHECK( l.aliasOf[R_dR] == ( keepStages ? -1 : (int)R_dL ) );
    CHECK( aliases == ( keepStages ? 1 : 2 ) );
}

struct Pinned
{
    uint32_t cap;
    uint64_t device, deviceKeepStages, host;
};
}  // namespace

int
main()
{
    for ( const uint32_t nBlocks : { 1u, 8u, 9u, 64u, 512u, 513u, 640u, 641u, 2560u, (uint32_t)MI355X_BZ2_MAX_BATCH_BLOCKS } ) {
        std::snprintf( currentCase, sizeof( currentCase ), "%u blocks", nBlocks );
        const uint32_t cap = capacityFor( nBlocks );
        CHECK( cap == capacityByRule( nBlocks ) );
        CHECK( cap >= nBlocks );
        checkLayout( cap, false );
        checkLayout( cap, true );
    }
    std::snprintf( currentCase, sizeof( currentCase ), "capacityFor" );
    CHECK( capacityFor( 0 ) == 8 && capacityFor( 1 ) == 8 && capacityFor( 8 ) == 8 && capacityFor( 9 ) == 16 );
    CHECK( capacityFor( 64 ) == 64 && capacityFor( 65 ) == 128 && capacityFor( 512 ) == 512 && capacityFor( 513 ) == 768 );
    CHECK( capacityFor( 640 ) == 768 && capacityFor( 768 ) == 768 && capacityFor( 769 ) == 1024 && capacityFor( 2560 ) == 2560 );
    CHECK( capacityFor( 2561 ) == 2816 );

    /* bytes of the two allocations as the arithmetic written out region by region gave them before there was a list */
    const Pinned pinned[] = {
        { 8, 81661184ull, 88862208ull, 2048 },
        { 16, 163318528ull, 177720320ull, 2816 },
        { 64, 653264896ull, 710871296ull, 7424 },
        { 512, 5226104832ull, 5686954240ull, 57600 },
        { 768, 7822379008ull, 8513652992ull, 86272 },
        { 2560, 25878857728ull, 28183103744ull, 286976 },
        { 2816, 28458354688ull, 30993025280ull, 315648 },
    };
    for ( const Pinned& p : pinned ) {
        std::snprintf( currentCase, sizeof( currentCase ), "totals, cap %u", p.cap );
        const ScratchLayout plain = layScratch( p.cap, false, SIZES ), keep = layScratch( p.cap, true, SIZES );
        CHECK( plain.deviceBytes == p.device );
        CHECK( keep.deviceBytes == p.deviceKeepStages );
        CHECK( plain.hostBytes == p.host && keep.hostBytes == p.host );
        /* KEEP_STAGES costs one more L column: cap * L_STRIDE + 256 bytes, rounded up to 256 */
        CHECK( keep.deviceBytes - plain.deviceBytes == ( ( (uint64_t)p.cap * L_STRIDE + 256 + 255 ) & ~uint64_t( 255 ) ) );
    }
    {
        /* the figure of the documents and of the bench record (scratch_MB_per_block): 10.11 MB per block at 2 560 blocks */
        std::snprintf( currentCase, sizeof( currentCase ), "MB per block" );
        const double perBlock = (double)layScratch( 2560, false, SIZES ).deviceBytes / 2560 / 1e6;
        CHECK( (long)( perBlock * 100 + 0.5 ) == 1011 );
    }
    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "scratch ok (%d regions)\n", (int)SCRATCH_REGIONS );
    return 0;
}
