/* The planner of mi355x_bz2_compress_buffers (bz2_compress.hpp) against plain restatements.  Block cuts: a byte-by-byte
 * model of libbz2's fill loop (a piece is flushed when the next byte differs or the piece holds 255 bytes; the block is
 * closed before the next byte, and after the last one, once the flushed RLE1 bytes reach the limit) on runs, random bytes and run edges at a cut.
 * Launches: caps of 1, 2, 3, 7 and 512 blocks and several memory budgets (including one below a single block), checked
 * for every block in exactly one launch, in order, counts and budgets kept, and the launch sums (positions, symbol and
 * selector slots, input span).  Beyond 2^32: 200 blocks of one repeated byte (45 899 235 input bytes in 899 985 RLE1
 * positions each) are cut by the budget at 148, so the first launch holds 6.8 GB of input, block offsets in it (inOff, the
 * prefix sums runCall forms) pass 2^32 at block 94 and the second launch's inputStart lies above 2^32; the same blocks as
 * one buffer whose Block::start values pass 2^32; caps of 1 and 0.  Map layout: one entry per block plus two, or one for an empty buffer.  Prints
 * "compress plan ok". */
#include <cstdio>
#include <random>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_compress.hpp"

using namespace mi355x::compress;

namespace
{
int failures = 0;
const char* currentCase = "";

#define CHECK( cond )                                                                                      \
    do {                                                                                                   \
        if ( !( cond ) ) {                                                                                 \
            if ( failures < 20 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                                    \
        }                                                                                                  \
    } while ( 0 )

/** libbz2's loop, byte by byte: decoded sizes of the blocks. */
std::vector<uint64_t>
modelCuts( const std::vector<uint8_t>& x, int level )
{
    std::vector<uint64_t> sizes;
    const uint64_t limit = blockLimit( level );
    uint64_t flushed = 0, inBlock = 0, pending = 0;
    int pendingByte = -1;
    const auto flushPiece = [&] () {
        if ( pending == 0 ) return;
        flushed += pending < 4 ? pending : 5;
        inBlock += pending;
        pending = 0;
    };
    for ( const uint8_t c : x ) {
        if ( flushed >= limit ) {   /* block full: the pending piece stays for the next block */
            sizes.push_back( inBlock );
            flushed = 0;
            inBlock = 0;
        }
        if ( c != pendingByte || pending == 255 ) {
            flushPiece();
            pendingByte = c;
        }
        ++pending;
    }
    if ( flushed >= limit ) {   /* the loop checks once more after the last byte (BZ_RUN, then BZ_FINISH) */
        sizes.push_back( inBlock );
        flushed = 0;
        inBlock = 0;
    }
    flushPiece();
    if ( inBlock > 0 ) sizes.push_back( inBlock );
    return sizes;
}

void
checkCuts( const std::vector<uint8_t>& x )
{
    for ( const int level : { 1, 2, 9 } ) {
        std::vector<Block> blocks;
        planBlocks( x.data(), x.size(), level, blocks );
        const auto want = modelCuts( x, level );
        CHECK( blocks.size() == want.size() );
        uint64_t at = 0;
        for ( size_t i = 0; i < blocks.size() && i < want.size(); ++i ) {
            CHECK( blocks[i].start == at );
            CHECK( blocks[i].size == want[i] );
            CHECK( blocks[i].rle <= blockLimit( level ) + 4 );
            CHECK( i + 1 == blocks.size() || blocks[i].rle >= blockLimit( level ) );
            at += blocks[i].size;
        }
        CHECK( at == x.size() );
    }
}

void
checkLaunches( const std::vector<Block>& blocks, uint32_t cap, uint64_t budget )
{
    const auto launches = planLaunches( blocks, cap, budget );
    const uint32_t maxBlocks = cap == 0 ? DEFAULT_LAUNCH_BLOCKS : cap;
    const uint64_t maxBytes = budget == 0 ? DEFAULT_LAUNCH_BYTES : budget;
    uint32_t next = 0;
    uint64_t input = 0;
    for ( const Launch& l : launches ) {
        CHECK( l.first == next );
        CHECK( l.count >= 1 && l.count <= maxBlocks );
        uint64_t positions = 0, symbols = 0, selectors = 0, bytes = 0, span = 0;
        for ( uint32_t k = l.first; k < l.first + l.count; ++k ) {
            positions += blocks[k].rle;
            symbols += symbolSlots( blocks[k].rle );
            selectors += selectorSlots( blocks[k].rle );
            bytes += blockBytes( blocks[k] );
            span += blocks[k].size;
        }
        CHECK( l.positions == positions && l.symbols == symbols && l.selectors == selectors && l.bytes == bytes );
        CHECK( l.inputStart == input && l.inputBytes == span );
        /* the launch's input span, the last of the inOff prefix sums runCall forms, against a 128-bit sum */
        unsigned __int128 wide = 0;
        for ( uint32_t k = l.first; k < l.first + l.count; ++k ) wide += blocks[k].size;
        CHECK( (unsigned __int128)l.inputBytes == wide );
        CHECK( l.count == 1 || l.bytes <= maxBytes );
        CHECK( positions < ( uint64_t( 1 ) << 32 ) );
        next += l.count;
        input += span;
    }
    CHECK( next == blocks.size() );
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 1234 );
    std::vector<std::vector<uint8_t>> inputs;
    inputs.push_back( {} );
    inputs.push_back( { 7 } );
    {
        std::vector<uint8_t> x( 700'000 );
        for ( auto& c : x ) c = (uint8_t)rng();
        inputs.push_back( x );
    }
    {
        std::vector<uint8_t> x;
        while ( x.size() < 1'500'000 ) x.insert( x.end(), 1 + rng() % 700, (uint8_t)( rng() % 4 ) );
        inputs.push_back( x );
    }
    for ( const uint64_t run : { 3, 4, 5, 255, 256, 259, 300'000 } ) {
        for ( const int level : { 1, 2 } ) {
            std::vector<uint8_t> x;
            for ( uint64_t i = 0; i + 2 < blockLimit( level ); ++i ) x.push_back( (uint8_t)( i % 251 ) );
            x.insert( x.end(), run, 0xEE );
            x.push_back( 1 );
            inputs.push_back( x );
        }
    }
    {
        std::vector<uint8_t> x;   /* ends exactly at a cut */
        for ( uint64_t i = 0; i < blockLimit( 1 ); ++i ) x.push_back( (uint8_t)( i % 251 ) );
        inputs.push_back( x );
    }
    currentCase = "cuts";
    for ( const auto& x : inputs ) checkCuts( x );

    currentCase = "launches";
    std::vector<Block> all;
    std::vector<uint32_t> counts;
    for ( const auto& x : inputs ) {
        const size_t before = all.size();
        planBlocks( x.data(), x.size(), 1, all );
        counts.push_back( (uint32_t)( all.size() - before ) );
    }
    for ( const uint32_t cap : { 0u, 1u, 2u, 3u, 7u, 512u } ) {
        for ( const uint64_t budget : { uint64_t( 0 ), uint64_t( 1 ) << 20, uint64_t( 50 ) << 20, uint64_t( 400 ) << 20 } ) {
            checkLaunches( all, cap, budget );
        }
    }
    CHECK( planLaunches( {}, 0, 0 ).empty() );

    currentCase = "launches beyond 2^32";
    {
        constexpr uint64_t FILLER = 45'899'235, CUT = uint64_t( 1 ) << 32;   /* 179 997 pieces of 255 equal bytes */
        constexpr uint32_t FILLER_RLE = 899'985;
        std::vector<Block> fillers;   /* 200 buffers of one block each: every start is 0 */
        for ( int i = 0; i < 200; ++i ) fillers.push_back( { 0, FILLER, FILLER_RLE } );
        CHECK( blockBytes( fillers[0] ) == 86'542'560 );
        const auto byBudget = planLaunches( fillers, 0, 0 );
        CHECK( byBudget.size() == 2 && byBudget[0].count == 148 && byBudget[1].count == 52 );
        CHECK( byBudget.size() == 2 && byBudget[0].bytes <= DEFAULT_LAUNCH_BYTES
               && byBudget[0].bytes + blockBytes( fillers[0] ) > DEFAULT_LAUNCH_BYTES );
        CHECK( byBudget.size() == 2 && byBudget[0].inputBytes == 148 * FILLER && byBudget[0].inputBytes > CUT );
        CHECK( byBudget.size() == 2 && byBudget[1].inputStart == 148 * FILLER && byBudget[1].inputStart > CUT
               && byBudget[1].inputBytes == 52 * FILLER );
        CHECK( 93 * FILLER < CUT && 94 * FILLER >= CUT );   /* inOff of block 94 is the first at or above 2^32 */
        std::vector<Block> oneBuffer;   /* the same bytes as ONE buffer: Block::start passes 2^32 */
        for ( uint64_t i = 0; i < 200; ++i ) oneBuffer.push_back( { i * FILLER, FILLER, FILLER_RLE } );
        CHECK( oneBuffer[94].start >= CUT && oneBuffer[93].start < CUT );
        const auto again = planLaunches( oneBuffer, 0, 0 );
        CHECK( again.size() == byBudget.size() );
        for ( size_t i = 0; i < again.size() && i < byBudget.size(); ++i ) {
            CHECK( again[i].first == byBudget[i].first && again[i].count == byBudget[i].count
                   && again[i].inputStart == byBudget[i].inputStart && again[i].inputBytes == byBudget[i].inputBytes );
            CHECK( again[i].inputStart == oneBuffer[again[i].first].start );
        }
        const auto single = planLaunches( oneBuffer, 1, 0 );
        CHECK( single.size() == 200 );
        for ( size_t i = 0; i < single.size(); ++i ) {
            CHECK( single[i].inputStart == i * FILLER && single[i].inputBytes == FILLER && single[i].count == 1 );
        }
        for ( const uint32_t cap : { 0u, 1u, 93u, 94u, 95u, 512u } ) {
            for ( const uint64_t budget : { uint64_t( 0 ), uint64_t( 1 ) << 20, uint64_t( 9 ) << 30, uint64_t( 64 ) << 30 } ) {
                checkLaunches( fillers, cap, budget );
                checkLaunches( oneBuffer, cap, budget );
            }
        }
        /* a budget that does not bind: the cap of 512 does, and one launch holds all 200 (9.2 GB of input) */
        const auto wide = planLaunches( fillers, 0, uint64_t( 64 ) << 30 );
        CHECK( wide.size() == 1 && wide[0].inputBytes == 200 * FILLER && wide[0].positions == 200ull * FILLER_RLE );
    }

    currentCase = "map layout";
    for ( const uint32_t c : counts ) CHECK( mapEntries( c ) == ( c == 0 ? 1u : c + 2u ) );
    CHECK( streamBytes( streamBits( 0 ) ) == 14 );
    CHECK( combineCrc( 0x80000000u, 1 ) == 0 );

    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "compress plan ok\n" );
    return 0;
}
