/* The range planner (bz2_ranges.hpp) against a brute-force restatement: every decoded byte of the file is looked up block
 * by block, every launch output is laid out from the plan's own launches, the pieces are applied to a destination, and
 * the result is compared with the file's bytes byte for byte.  Maps are hand-written (end-of-stream entries, two streams,
 * an empty file) and seeded random ones; ranges unsorted, overlapping, duplicated, empty, at and beyond the end of the
 * file, longer than a launch; caps 1, 2, 3 and 512.  With bounded residency the packed input is built from the windows
 * and every block's rebased bit offset must see the file's bytes from its magic word to the end of its slack.
 * The same cases once more behind one block of 2^32 - k decoded bytes that no range touches, its successors' bit offsets
 * starting just below 2^32 as well: blocks, extents, pieces and windows that lie below, across and above 2^32.
 * Prints "ranges ok". */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_ranges.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
const char* currentCase = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 20 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

using Map = std::vector<std::pair<uint64_t, uint64_t> >;

/* decoded byte x of the file, and compressed byte y of the file: any value that depends on the position */
uint8_t decodedByte( uint64_t x ) { return (uint8_t)( ( x * 2654435761u ) >> 13 ); }
uint8_t fileByte( uint64_t y ) { return (uint8_t)( ( y * 40503u + 17 ) >> 3 ); }

/* the data block (index into the map) holding decoded byte x: a brute-force walk over the map */
size_t
entryHolding( const Map& map, uint64_t x )
{
    for ( size_t i = 0; i + 1 < map.size(); ++i ) {
        if ( map[i].second <= x && x < map[i + 1].second ) return i;
    }
    return SIZE_MAX;
}

void
checkPlan( const Map& map, const std::vector<uint64_t>& offsets, const std::vector<uint64_t>& sizes, size_t cap,
           bool packed, uint64_t fileBytes )
{
    const auto plan = planRanges( map, offsets.data(), sizes.data(), offsets.size(), cap, packed, fileBytes );
    const uint64_t total = map.empty() ? 0 : map.back().second;

    /* the blocks every range needs, found byte by byte */
    std::set<uint64_t> needed;
    uint64_t dstBytes = 0;
    for ( size_t i = 0; i < offsets.size(); ++i ) {
        dstBytes += sizes[i];
        for ( uint64_t x = offsets[i]; x < offsets[i] + sizes[i] && x < total; ++x ) {
            needed.insert( map[entryHolding( map, x )].first );
        }
    }
    CHECK( plan.dstBytes == dstBytes );
    CHECK( plan.distinctBlocks == needed.size() );

    /* launches: ascending, distinct, at most `cap`, together exactly the needed blocks, each once */
    std::vector<uint64_t> launched;
    for ( const auto& launch : plan.launches ) {
        CHECK( !launch.bits.empty() && launch.bits.size() <= cap );
        CHECK( launch.sizes.size() == launch.bits.size() && launch.outOffsets.size() == launch.bits.size() );
        for ( size_t k = 0; k < launch.bits.size(); ++k ) {
            if ( k > 0 ) CHECK( launch.bits[k - 1] < launch.bits[k] );
            if ( !launched.empty() ) CHECK( launched.back() < launch.bits[k] );
            launched.push_back( launch.bits[k] );
        }
    }
    CHECK( std::vector<uint64_t>( needed.begin(), needed.end() ) == launched );
    for ( size_t l = 0; l + 1 < plan.launches.size(); ++l ) CHECK( plan.launches[l].bits.size() == cap );

    /* every launch's ragged output, built from the map: block k at the exclusive prefix sum of the sizes before it */
    std::vector<std::vector<uint8_t> > outputs;
    for ( const auto& launch : plan.launches ) {
        std::vector<uint8_t> out;
        for ( size_t k = 0; k < launch.bits.size(); ++k ) {
            size_t e = 0;
            while ( map[e].first != launch.bits[k] ) ++e;
            CHECK( launch.sizes[k] == map[e + 1].second - map[e].second );
            CHECK( launch.outOffsets[k] == out.size() );
            for ( uint64_t x = map[e].second; x < map[e + 1].second; ++x ) out.push_back( decodedByte( x ) );
        }
        CHECK( launch.outBytes == out.size() );
        outputs.push_back( std::move( out ) );
    }

    /* the destination, from the pieces, against the file; bytes behind n_read stay as they were */
    constexpr uint8_t UNTOUCHED = 0xA5;
    std::vector<uint8_t> dst( dstBytes, UNTOUCHED );
    std::vector<int> written( dstBytes, 0 );
    for ( const auto& piece : plan.pieces ) {
        CHECK( piece.launch < outputs.size() );
        if ( piece.launch >= outputs.size() ) continue;
        CHECK( piece.size > 0 );
        CHECK( piece.src + piece.size <= outputs[piece.launch].size() );
        CHECK( piece.dst + piece.size <= dstBytes );
        if ( piece.src + piece.size > outputs[piece.launch].size() || piece.dst + piece.size > dstBytes ) continue;
        for ( uint64_t k = 0; k < piece.size; ++k ) {
            dst[piece.dst + k] = outputs[piece.launch][piece.src + k];
            ++written[piece.dst + k];
        }
    }
    uint64_t at = 0;
    for ( size_t i = 0; i < offsets.size(); at += sizes[i], ++i ) {
        const uint64_t expect = offsets[i] >= total ? 0 : std::min( sizes[i], total - offsets[i] );
        CHECK( plan.nRead[i] == expect );
        for ( uint64_t k = 0; k < sizes[i]; ++k ) {
            if ( k < expect ) {
                CHECK( dst[at + k] == decodedByte( offsets[i] + k ) && written[at + k] == 1 );
            } else {
                CHECK( dst[at + k] == UNTOUCHED && written[at + k] == 0 );
            }
        }
    }

    /* bounded residency: the packed input holds, at every block's rebased offset, the file's bytes from the word of its
     * magic to the next entry's byte plus the slack (clipped to the file) */
    for ( const auto& launch : plan.launches ) {
        if ( !packed ) {
            CHECK( launch.windows.empty() && launch.packedBits.empty() && launch.packedBytes == 0 );
            continue;
        }
        CHECK( launch.packedBits.size() == launch.bits.size() );
        std::vector<uint8_t> input( launch.packedBytes, 0 );
        uint64_t end = 0, windowBytes = 0;
        for ( const auto& w : launch.windows ) {
            CHECK( w.at % 4 == 0 && w.at >= end && w.from < w.to && w.to <= fileBytes );
            for ( uint64_t y = w.from; y < w.to && w.at + ( y - w.from ) < input.size(); ++y ) {
                input[w.at + ( y - w.from )] = fileByte( y );
            }
            end = w.at + ( w.to - w.from );
            windowBytes += w.to - w.from;
        }
        CHECK( end == launch.packedBytes );
        CHECK( launch.packedBytes <= windowBytes + 3 * launch.windows.size() );
        for ( size_t k = 0; k < launch.bits.size(); ++k ) {
            size_t e = 0;
            while ( map[e].first != launch.bits[k] ) ++e;
            const uint64_t bits = launch.bits[k], rel = launch.packedBits[k];
            CHECK( ( rel & 31 ) == ( bits & 31 ) );    /* same position in its 32-bit word */
            const uint64_t from = ( bits / 8 ) & ~uint64_t( 3 );
            const uint64_t to = std::min( fileBytes, ( map[e + 1].first + 7 ) / 8 + RANGE_WINDOW_SLACK );
            for ( uint64_t y = from; y < to; ++y ) {
                const uint64_t p = rel / 8 - ( bits / 8 - y );
                CHECK( p < input.size() && input[p] == fileByte( y ) );
            }
        }
    }
}

/* a map from block sizes: streams of data blocks (decoded sizes), each followed by its end-of-stream entry, then the
 * end-of-file entry; compressed sizes of the blocks vary */
Map
makeMap( const std::vector<std::vector<uint64_t> >& streams, std::mt19937_64& rng, uint64_t* fileBytes,
         uint64_t frontBytes = 0, uint64_t frontBits = 0 )
{
    Map map;
    uint64_t bits = 32, bytes = 0;
    if ( frontBytes > 0 ) {
        /* a stream of one block of frontBytes decoded bytes that ends at bit frontBits */
        map.push_back( { bits, 0 } );
        map.push_back( { frontBits - 80, frontBytes } );
        bits = frontBits + 32;
        bytes = frontBytes;
    }
    for ( const auto& stream : streams ) {
        for ( const auto size : stream ) {
            map.push_back( { bits, bytes } );
            bits += 200 + rng() % 5000;
            bytes += size;
        }
        map.push_back( { bits, bytes } );              /* end-of-stream block: 80 bits and the padding */
        bits = ( bits + 80 + 7 ) / 8 * 8 + 32;         /* the next stream's header */
    }
    const uint64_t endBits = bits - 32;
    map.push_back( { endBits, bytes } );
    *fileBytes = endBits / 8;
    return map;
}

/* `low`: the ranges keep to the decoded bytes from `low` on (the front block of a high map is never asked for: the
 * restatement would walk its 2^32 bytes one by one) */
void
runCases( const char* name, const Map& map, uint64_t fileBytes, std::mt19937_64& rng, uint64_t low = 0 )
{
    currentCase = name;
    const uint64_t total = ( map.empty() ? 0 : map.back().second ) - low;
    std::vector<uint64_t> offsets, sizes;
    /* hand-picked: empty, at the end, beyond it, straddling it, the whole file, every block boundary +-1 */
    const auto add = [&] ( uint64_t o, uint64_t s ) { offsets.push_back( low + o ); sizes.push_back( s ); };
    add( 0, 0 );
    add( total, 5 );
    add( total + 100, 7 );
    add( total > 3 ? total - 3 : 0, 10 );
    add( 0, total );
    add( 0, total + 1 );
    for ( size_t i = 0; i < map.size(); ++i ) {
        if ( map[i].second < low ) continue;
        const uint64_t b = map[i].second - low;
        add( b > 0 ? b - 1 : 0, 2 );
        add( b, 1 );
        add( b, 0 );
    }
    /* seeded: unsorted, overlapping, duplicated */
    for ( int k = 0; k < 60; ++k ) {
        const uint64_t o = total > 0 ? rng() % ( total + 50 ) : rng() % 50;
        const uint64_t s = rng() % 4 == 0 ? 0 : rng() % ( 1 + total / 3 );
        add( o, s );
        if ( k % 7 == 0 ) add( o, s );
    }
    for ( const size_t cap : { 1, 2, 3, 512 } ) {
        for ( const bool packed : { false, true } ) {
            checkPlan( map, offsets, sizes, cap, packed, fileBytes );
        }
    }
    /* few ranges: one range longer than a launch holds */
    for ( const size_t cap : { 1, 2 } ) {
        checkPlan( map, { low + 1 }, { total }, cap, true, fileBytes );
    }
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0x3A11 );
    uint64_t fileBytes = 0;

    /* two streams, 3 + 2 blocks, end-of-stream entries between */
    {
        const auto map = makeMap( { { 100, 250, 50 }, { 300, 1 } }, rng, &fileBytes );
        runCases( "two streams", map, fileBytes, rng );
    }
    /* a single block, a single stream */
    {
        const auto map = makeMap( { { 1 } }, rng, &fileBytes );
        runCases( "one byte", map, fileBytes, rng );
    }
    /* an empty file: the stream's end-of-stream block and the end-of-file entry */
    {
        const Map map = { { 32, 0 }, { 112, 0 } };
        runCases( "empty file", map, 14, rng );
    }
    /* no map at all */
    runCases( "no map", Map{}, 0, rng );
    /* an index that is not complete yet: the last entry is the end of the open block */
    {
        const Map map = { { 32, 0 }, { 5000, 900 }, { 9000, 1800 } };
        runCases( "open index", map, 2000, rng );
    }
    /* seeded maps: one to four streams of up to 40 blocks of random sizes */
    for ( int m = 0; m < 12; ++m ) {
        std::vector<std::vector<uint64_t> > streams( 1 + rng() % 4 );
        for ( auto& stream : streams ) {
            stream.resize( 1 + rng() % 40 );
            for ( auto& size : stream ) size = 1 + rng() % 400;
        }
        const auto map = makeMap( streams, rng, &fileBytes );
        runCases( "seeded", map, fileBytes, rng );
    }

    /* offsets at and across 2^32: the maps above behind a front block of 2^32 - k bytes, the bit offsets of what follows
     * starting 8 * j bits below 2^32.  With k inside the first blocks, one block holds byte 2^32 - 1 and byte 2^32 (or ends
     * exactly there: k = the first block's size), extents start below and end above it, and so do the packed windows */
    {
        const uint64_t cut = uint64_t( 1 ) << 32;
        const std::vector<std::vector<uint64_t> > streams = { { 100, 250, 50 }, { 300, 1 } };
        for ( const uint64_t k : { 1, 37, 100, 101, 349, 350, 400, 700 } ) {
            for ( const uint64_t j : { 5, 61, 120 } ) {
                const auto map = makeMap( streams, rng, &fileBytes, cut - k, cut - 8 * j );
                currentCase = "high";
                CHECK( map[2].second == cut - k && map[2].first < cut && map.back().first > cut && map.back().second > cut );
                runCases( "high", map, fileBytes, rng, cut - k );
            }
        }
        for ( int m = 0; m < 6; ++m ) {
            std::vector<std::vector<uint64_t> > seeded( 1 + rng() % 4 );
            for ( auto& stream : seeded ) {
                stream.resize( 1 + rng() % 40 );
                for ( auto& size : stream ) size = 1 + rng() % 400;
            }
            const auto map = makeMap( seeded, rng, &fileBytes, cut - 1 - rng() % 3000, cut - 8 * ( 1 + rng() % 3000 ) );
            runCases( "high seeded", map, fileBytes, rng, map[2].second );
        }
    }

    /* the requested sizes must add up within 64 bits; a cap of 0 is refused */
    currentCase = "arguments";
    {
        const Map map = { { 32, 0 }, { 1000, 100 } };
        const uint64_t offsets[2] = { 0, 0 };
        const uint64_t sizes[2] = { ~uint64_t( 0 ), 2 };
        bool thrown = false;
        try { (void)planRanges( map, offsets, sizes, 2, 4, false, 200 ); } catch ( const std::invalid_argument& ) { thrown = true; }
        CHECK( thrown );
        thrown = false;
        try { (void)planRanges( map, offsets, sizes, 1, 0, false, 200 ); } catch ( const std::invalid_argument& ) { thrown = true; }
        CHECK( thrown );
    }

    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "ranges ok\n" );
    return 0;
}
