/* The search planner (bz2_search.hpp) against a byte-by-byte restatement.
 *
 * seamMatches: a text is cut into extents back to back, every extent gives its first and last min(m - 1, size) bytes and
 * nothing else, and the result must be exactly the matches of the whole text that do not lie inside a single extent,
 * ascending and once each.  Extent sizes 0, 1, m - 2, m - 1, m, 2m - 3, 2m - 2, 2m - 1 and large, in seeded orders and in
 * rows of tiny ones; m in {1, 2, 3, 16, 255, 256}; periodic text (periods 1, 2, 3, 5 and m - 1, a few bytes flipped), so
 * that matches overlap themselves and cross one, two and five and more boundaries -- the harness counts the boundaries
 * every expected match crosses and insists on having seen each kind.
 *
 * planSearch: the plan is executed on the CPU the way the reader executes it on the GPU.  Every launch's ragged output is
 * laid out from the plan's own launches, the matches inside its extent come from a scan of that stretch of the output,
 * head and tail are cut from it, and the launches' matches merged with seamMatches' must be the matches of the file in
 * [start, end) -- with start and end cutting the first and the last extent, beyond the size, empty, and shorter than m.
 * The extents must lie back to back from the clipped start to the clipped end, inside their launches' outputs, and the
 * launches must hold exactly the blocks that intersect the range, once, at most `cap` each.
 *
 * Offsets at and across 2^32: seamCase with the extents' file offsets shifted so that two of them meet exactly at 2^32 (and
 * one byte to either side of it), and planCase on maps whose blocks lie behind a front block of 2^32 - k bytes that no
 * range touches (`base`: the file offset of the bytes held), the bit offsets of what follows from just below 2^32 on:
 * extents that start below and end above 2^32, matches that straddle it.  Prints "search ok". */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <set>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_search.hpp"

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
using Bytes = std::vector<uint8_t>;

/* every p in [from, to - m] with text[p : p + m] == pattern */
std::vector<uint64_t>
matchesIn( const Bytes& text, uint64_t from, uint64_t to, const Bytes& pattern )
{
    std::vector<uint64_t> found;
    const size_t m = pattern.size();
    for ( uint64_t p = from; p + m <= to; ++p ) {
        if ( std::memcmp( text.data() + p, pattern.data(), m ) == 0 ) found.push_back( p );
    }
    return found;
}

ExtentSeam
seamOf( const Bytes& text, uint64_t offset, uint64_t size, uint32_t m )
{
    const auto k = seamLength( m, size );
    return { offset, size, Bytes( text.begin() + offset, text.begin() + offset + k ),
             Bytes( text.begin() + offset + size - k, text.begin() + offset + size ) };
}

/* periodic text with a few bytes flipped, and the pattern that the undisturbed text holds at every multiple of the period */
void
periodic( size_t size, size_t period, uint32_t m, std::mt19937_64& rng, Bytes& text, Bytes& pattern )
{
    text.resize( size );
    for ( size_t i = 0; i < size; ++i ) text[i] = (uint8_t)( 'a' + i % period );
    pattern.assign( text.begin(), text.begin() + m );
    for ( size_t k = 0; k < size / 97; ++k ) text[rng() % size] = '#';
}

int crossedKinds = 0;   /* bit 0: a match crossed exactly 1 boundary, bit 1: exactly 2, bit 2: 5 or more */

/* `shift`: added to every extent's file offset, and so to every expected match */
void
seamCase( const Bytes& text, const Bytes& pattern, const std::vector<uint64_t>& sizes, uint64_t from, uint64_t shift = 0 )
{
    const auto m = (uint32_t)pattern.size();
    std::vector<ExtentSeam> seams;
    uint64_t at = from;
    for ( const auto size : sizes ) {
        seams.push_back( seamOf( text, at, size, m ) );
        at += size;
    }
    CHECK( at <= text.size() );
    std::vector<uint64_t> expected;
    for ( const auto p : matchesIn( text, from, at, pattern ) ) {
        /* the distinct boundaries strictly inside (p, p + m): ends of non-empty extents */
        size_t crossed = 0;
        bool inside = false;
        for ( const auto& seam : seams ) {
            const uint64_t end = seam.fileOffset + seam.size;
            if ( seam.size > 0 && end > p && end < p + m ) ++crossed;
            if ( seam.fileOffset <= p && p + m <= end ) inside = true;
        }
        CHECK( inside == ( crossed == 0 ) );
        if ( !inside ) {
            expected.push_back( p );
            crossedKinds |= crossed == 1 ? 1 : crossed == 2 ? 2 : crossed >= 5 ? 4 : 0;
        }
    }
    for ( auto& seam : seams ) seam.fileOffset += shift;
    for ( auto& p : expected ) p += shift;
    const auto got = seamMatches( pattern.data(), m, seams );
    CHECK( got == expected );
}

void
seamCases()
{
    std::mt19937_64 rng( 0x5EA4 );
    for ( const uint32_t m : { 1u, 2u, 3u, 16u, 255u, 256u } ) {
        std::vector<uint64_t> kinds{ 0, 1, m, 2ull * m - 1, 3ull * m + 17, 1000 };
        if ( m >= 2 ) kinds.insert( kinds.end(), { m - 2ull, m - 1ull, 2ull * m - 2 } );
        if ( m >= 3 ) kinds.push_back( 2ull * m - 3 );
        for ( const size_t period : { (size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)std::max( 1u, m - 1 ) } ) {
            Bytes text, pattern;
            periodic( 100000, period, m, rng, text, pattern );
            currentCase = "seeded extent sizes";
            for ( int round = 0; round < 6; ++round ) {
                std::vector<uint64_t> sizes;
                for ( int k = 0; k < 14; ++k ) sizes.push_back( kinds[rng() % kinds.size()] );
                seamCase( text, pattern, sizes, rng() % 300 );
            }
            currentCase = "every size next to every size";
            std::vector<uint64_t> pairs;
            for ( const auto a : kinds ) {
                for ( const auto b : kinds ) {
                    pairs.push_back( a );
                    pairs.push_back( b );
                }
            }
            seamCase( text, pattern, pairs, 7 );
            currentCase = "rows of tiny extents";
            seamCase( text, pattern, { 1000, 1, 1, 1, 1, 1, 1, 1000, 2, 3, 1000, 1, 0, 0, 1, 1000, 0, 1, 2, 1, 0 }, 11 );
            seamCase( text, pattern, std::vector<uint64_t>( 600, 1 ), 0 );
            seamCase( text, pattern, std::vector<uint64_t>( 300, 3 ), 5 );
            currentCase = "two extents that meet at 2^32, and next to it";
            for ( const uint64_t first : { (uint64_t)1000, (uint64_t)m, (uint64_t)1 } ) {
                const uint64_t cut = uint64_t( 1 ) << 32;
                for ( const uint64_t meet : { cut - 1, cut, cut + 1, cut + m - 1 } ) {
                    /* the first extent ends at `meet`; rows of tiny ones and long ones follow */
                    seamCase( text, pattern, { first, 1000, 1, 1, m, 2, 1000, 0, 1, 3ull * m + 17 }, 13, meet - 13 - first );
                }
            }
            currentCase = "one extent, no extent, empty extents only";
            seamCase( text, pattern, { 5000 }, 3 );
            seamCase( text, pattern, {}, 0 );
            seamCase( text, pattern, { 0, 0, 0 }, 9 );
        }
    }
    currentCase = "coverage";
    CHECK( crossedKinds == 7 );

    currentCase = "argument checks";
    const Bytes text( 100, 'x' );
    for ( const uint32_t bad : { 0u, 257u } ) {
        bool thrown = false;
        try {
            (void)seamMatches( text.data(), bad, {} );
        } catch ( const std::invalid_argument& ) {
            thrown = true;
        }
        CHECK( thrown );
    }
    bool thrown = false;
    try {
        (void)seamMatches( text.data(), 4, { seamOf( text, 0, 10, 4 ), seamOf( text, 11, 10, 4 ) } );   /* a gap */
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
    thrown = false;
    try {
        (void)seamMatches( text.data(), 4, { seamOf( text, 0, 10, 3 ) } );   /* head and tail of another m */
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
}

/* streams of data blocks (decoded sizes), each followed by its end-of-stream entry, then the end-of-file entry */
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
        map.push_back( { bits, bytes } );
        bits = ( bits + 80 + 7 ) / 8 * 8 + 32;
    }
    const uint64_t endBits = bits - 32;
    map.push_back( { endBits, bytes } );
    *fileBytes = endBits / 8;
    return map;
}

/* `base`: `file` holds the decoded bytes from file offset `base` on (a high map's front block is not held, and no range
 * of such a case starts below `base`) */
void
planCase( const Map& map, uint64_t fileBytes, const Bytes& file, const Bytes& pattern, uint64_t start, uint64_t end, size_t cap,
          uint64_t base = 0 )
{
    const auto m = (uint32_t)pattern.size();
    const uint64_t total = base + file.size();
    const uint64_t to = std::min( end, total ), from = std::min( start, to );
    for ( const bool packed : { false, true } ) {
        const auto plan = planSearch( map, start, end, m, cap, packed, fileBytes );
        CHECK( plan.extents.size() == plan.launches.size() );
        if ( to - from < m ) {
            CHECK( plan.launches.empty() && plan.start == plan.end );
            continue;
        }
        CHECK( plan.start == from && plan.end == to );
        /* the blocks that intersect [from, to), from the map alone */
        std::vector<uint64_t> wantedBits;
        std::vector<std::pair<uint64_t, uint64_t> > blockOfBits;   /* per wanted block: {start, length} */
        for ( size_t i = 0; i + 1 < map.size(); ++i ) {
            const uint64_t s = map[i].second, e = map[i + 1].second;
            if ( e > s && s < to && e > from ) {
                wantedBits.push_back( map[i].first );
                blockOfBits.push_back( { s, e - s } );
            }
        }
        std::vector<uint64_t> launchedBits;
        uint64_t at = from;
        std::vector<ExtentSeam> seams;
        std::vector<uint64_t> found;
        for ( size_t l = 0; l < plan.launches.size(); ++l ) {
            const auto& launch = plan.launches[l];
            CHECK( !launch.bits.empty() && launch.bits.size() <= cap );
            CHECK( packed == !launch.windows.empty() );
            /* the launch's ragged output: its blocks back to back */
            Bytes output;
            for ( size_t k = 0; k < launch.bits.size(); ++k ) {
                const auto& block = blockOfBits[launchedBits.size() < blockOfBits.size() ? launchedBits.size() : 0];
                launchedBits.push_back( launch.bits[k] );
                CHECK( launch.outOffsets[k] == output.size() && launch.sizes[k] == block.second );
                output.insert( output.end(), file.begin() + ( block.first - base ), file.begin() + ( block.first - base ) + block.second );
            }
            CHECK( launch.outBytes == output.size() );
            const auto& extent = plan.extents[l];
            CHECK( extent.fileOffset == at && extent.size > 0 );
            CHECK( extent.src <= output.size() && extent.size <= output.size() - extent.src );
            if ( extent.src + extent.size > output.size() ) return;
            /* extent offset -> file offset is one addition */
            CHECK( extent.fileOffset >= base );
            if ( extent.fileOffset < base ) return;
            CHECK( std::memcmp( output.data() + extent.src, file.data() + ( extent.fileOffset - base ), extent.size ) == 0 );
            /* only the first launch's extent may start, and only the last one's may end, inside the output */
            CHECK( l == 0 || extent.src == 0 );
            CHECK( l + 1 == plan.launches.size() || extent.src + extent.size == output.size() );
            for ( const auto p : matchesIn( output, extent.src, extent.src + extent.size, pattern ) ) {
                found.push_back( extent.fileOffset + ( p - extent.src ) );
            }
            seams.push_back( seamOf( output, extent.src, extent.size, m ) );
            seams.back().fileOffset = extent.fileOffset;
            at += extent.size;
        }
        CHECK( at == to );
        CHECK( launchedBits == wantedBits );
        const auto between = seamMatches( pattern.data(), m, seams );
        found.insert( found.end(), between.begin(), between.end() );
        std::sort( found.begin(), found.end() );
        auto expected = matchesIn( file, from - base, to - base, pattern );
        for ( auto& p : expected ) p += base;
        CHECK( found == expected );
        CHECK( std::set<uint64_t>( found.begin(), found.end() ).size() == found.size() );
    }
}

void
planCases()
{
    std::mt19937_64 rng( 0x9A7 );
    const std::vector<std::vector<std::vector<uint64_t> > > layouts{
        { { 900, 900, 900, 417 } },
        { { 2, 1 }, {}, { 3 }, { 1 }, { 3, 2, 1, 1 }, {}, { 700 }, { 1, 1, 1, 1, 1, 1, 1, 5 } },   /* streams without a block */
        { { 300, 1, 299 }, { 1 }, { 1 }, { 600, 600 } },
    };
    for ( const auto& layout : layouts ) {
        uint64_t fileBytes = 0;
        const auto map = makeMap( layout, rng, &fileBytes );
        const uint64_t total = map.back().second;
        for ( const uint32_t m : { 1u, 2u, 3u, 16u, 255u, 256u } ) {
            for ( const size_t period : { (size_t)1, (size_t)3, (size_t)7 } ) {
                Bytes file, pattern;
                periodic( total, period, m, rng, file, pattern );
                for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
                    currentCase = "whole file, and beyond it";
                    planCase( map, fileBytes, file, pattern, 0, total, cap );
                    planCase( map, fileBytes, file, pattern, 0, ~uint64_t( 0 ), cap );
                    currentCase = "empty, shorter than m, exactly m, start beyond the size";
                    planCase( map, fileBytes, file, pattern, 5, 5, cap );
                    planCase( map, fileBytes, file, pattern, 9, 3, cap );
                    planCase( map, fileBytes, file, pattern, 4, 4 + m - 1, cap );
                    planCase( map, fileBytes, file, pattern, 4, 4 + m, cap );
                    planCase( map, fileBytes, file, pattern, total - std::min<uint64_t>( total, m ), total, cap );
                    planCase( map, fileBytes, file, pattern, total, total + 10, cap );
                    planCase( map, fileBytes, file, pattern, total + 1, ~uint64_t( 0 ), cap );
                    currentCase = "seeded ranges that cut the first and the last extent";
                    for ( int k = 0; k < 12; ++k ) {
                        const uint64_t a = rng() % total, b = rng() % ( total + 3 );
                        planCase( map, fileBytes, file, pattern, std::min( a, b ), std::max( a, b ), cap );
                    }
                }
            }
        }
    }
    /* the layouts behind a front block of 2^32 - k bytes: k inside the first block, at its end, in a later block */
    const uint64_t cut = uint64_t( 1 ) << 32;
    for ( const auto& layout : layouts ) {
        for ( const uint64_t k : { (uint64_t)1, (uint64_t)2, (uint64_t)300, (uint64_t)600 } ) {
            uint64_t fileBytes = 0;
            const uint64_t base = cut - k;
            const auto map = makeMap( layout, rng, &fileBytes, base, cut - 8 * ( 5 + rng() % 100 ) );
            const uint64_t total = map.back().second;
            for ( const uint32_t m : { 1u, 2u, 16u, 256u } ) {
                Bytes file, pattern;
                periodic( total - base, m == 16 ? 7 : 3, m, rng, file, pattern );
                for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
                    currentCase = "high: everything behind the front, and beyond the size";
                    planCase( map, fileBytes, file, pattern, base, total, cap, base );
                    planCase( map, fileBytes, file, pattern, base, ~uint64_t( 0 ), cap, base );
                    currentCase = "high: ranges that end and start at 2^32 and next to it";
                    for ( const uint64_t edge : { cut - 1, cut, cut + 1, cut + m - 1, cut + m } ) {
                        planCase( map, fileBytes, file, pattern, base, edge, cap, base );
                        planCase( map, fileBytes, file, pattern, edge, total, cap, base );
                        planCase( map, fileBytes, file, pattern, edge > base + m ? edge - m : base, edge, cap, base );
                    }
                    currentCase = "high: seeded ranges";
                    for ( int r = 0; r < 8; ++r ) {
                        const uint64_t a = base + rng() % ( total - base ), b = base + rng() % ( total - base + 3 );
                        planCase( map, fileBytes, file, pattern, std::min( a, b ), std::max( a, b ), cap, base );
                    }
                }
            }
        }
    }
    currentCase = "an empty file";
    const Map empty{ { 32, 0 }, { 80, 0 } };
    const Bytes pattern{ 'a' };
    planCase( empty, 14, {}, pattern, 0, 10, 4 );
    planCase( {}, 0, {}, pattern, 0, ~uint64_t( 0 ), 4 );
    currentCase = "pattern sizes that are refused";
    for ( const uint32_t bad : { 0u, 257u } ) {
        bool thrown = false;
        try {
            (void)planSearch( empty, 0, 10, bad, 4, false, 14 );
        } catch ( const std::invalid_argument& ) {
            thrown = true;
        }
        CHECK( thrown );
    }
}
}  // namespace

int
main()
{
    seamCases();
    planCases();
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "search ok\n" );
    return 0;
}
