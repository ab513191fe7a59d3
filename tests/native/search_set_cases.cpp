/* The planner and the seam matches of a search for a SET of patterns (bz2_search.hpp) against a byte-by-byte restatement.
 *
 * seamMatchesSet: a text is cut into extents back to back, every extent gives its first and last min(m_max - 1, size)
 * bytes and nothing else, and the result must be exactly the pairs (p, i) of the whole text that do not lie inside a single
 * extent, in (p, i) order and once each.  Extent sizes 0, 1, 2, 3, m_max - 1, m_max, m_max + 1 and large, in seeded orders
 * and in rows of tiny ones; sets with equal patterns, prefix chains, and lengths 1 and 256 together; periodic text, so that
 * the patterns overlap themselves and each other; and one pair that crosses three extents, asserted by name.
 *
 * planSearchSet: ranges shorter than m_min have no launches, ranges between m_min and m_max have them, and the plan is
 * planSearch's for m_min.  The plan is then executed on the CPU as the reader executes it: the pairs inside every extent
 * from a scan of it, merged with seamMatchesSet's, must be the pairs of the file in [start, end) with the end rule applied
 * per pattern.
 *
 * The limit: safePairs against its restatement, and the rule itself -- cutting the launches off behind the first front
 * that holds `limit` safe pairs gives the first `limit` pairs of the whole result -- for every limit of a case in which
 * a long pattern crosses a boundary in front of a short one inside.
 *
 * Offsets at and across 2^32: seamCase with the extents' file offsets shifted so that two of them meet at 2^32 and next to
 * it; planCase on maps whose blocks lie behind a front block of 2^32 - k bytes that no range touches (`base`: the file
 * offset of the bytes held), the bit offsets of what follows from just below 2^32 on; and the limit rule with the first
 * front's end exactly at 2^32 -- the long pattern crosses it -- and with the limit reached above it.
 *
 * writeSetImage: every pattern is found again through the first-byte table, the buckets in id order.  patternSetError:
 * every limit.  Prints "search set ok". */
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
using Patterns = std::vector<Bytes>;

PatternSet
setOf( const Patterns& patterns )
{
    Bytes all;
    std::vector<uint32_t> sizes;
    for ( const auto& pattern : patterns ) {
        all.insert( all.end(), pattern.begin(), pattern.end() );
        sizes.push_back( (uint32_t)pattern.size() );
    }
    return makePatternSet( all.data(), sizes.data(), sizes.size() );
}

/* every (p, i) with from <= p, p + m_i <= to and text[p : p + m_i] == pattern i, in (p, i) order */
std::vector<SetMatch>
pairsIn( const Bytes& text, uint64_t from, uint64_t to, const Patterns& patterns )
{
    std::vector<SetMatch> found;
    for ( uint64_t p = from; p < to; ++p ) {
        for ( uint32_t i = 0; i < patterns.size(); ++i ) {
            const size_t m = patterns[i].size();
            if ( p + m <= to && std::memcmp( text.data() + p, patterns[i].data(), m ) == 0 ) found.push_back( { p, i } );
        }
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

Bytes
periodic( size_t size, size_t period, std::mt19937_64& rng )
{
    Bytes text( size );
    for ( size_t i = 0; i < size; ++i ) text[i] = (uint8_t)( 'a' + i % period );
    for ( size_t k = 0; k < size / 97; ++k ) text[rng() % size] = '#';
    return text;
}

Bytes
slice( const Bytes& text, size_t at, size_t n )
{
    return Bytes( text.begin() + at, text.begin() + at + n );
}

size_t mostCrossed = 0;

/* `shift`: added to every extent's file offset, and so to every expected pair's position */
void
seamCase( const Bytes& text, const Patterns& patterns, const std::vector<uint64_t>& sizes, uint64_t from, uint64_t shift = 0 )
{
    const auto set = setOf( patterns );
    std::vector<ExtentSeam> seams;
    uint64_t at = from;
    for ( const auto size : sizes ) {
        seams.push_back( seamOf( text, at, size, set.mMax ) );
        at += size;
    }
    CHECK( at <= text.size() );
    if ( at > text.size() ) return;
    std::vector<SetMatch> expected;
    for ( const auto& pair : pairsIn( text, from, at, patterns ) ) {
        const uint64_t p = pair.first, m = patterns[pair.second].size();
        size_t crossed = 0;
        bool inside = false;
        for ( const auto& seam : seams ) {
            const uint64_t end = seam.fileOffset + seam.size;
            if ( seam.size > 0 && end > p && end < p + m ) ++crossed;
            if ( seam.fileOffset <= p && p + m <= end ) inside = true;
        }
        CHECK( inside == ( crossed == 0 ) );
        if ( !inside ) {
            expected.push_back( pair );
            mostCrossed = std::max( mostCrossed, crossed );
        }
    }
    for ( auto& seam : seams ) seam.fileOffset += shift;
    for ( auto& pair : expected ) pair.first += shift;
    const auto got = seamMatchesSet( set, seams );
    CHECK( got == expected );
}

void
seamCases()
{
    std::mt19937_64 rng( 0x5E75 );
    for ( const size_t period : { (size_t)1, (size_t)2, (size_t)3, (size_t)5, (size_t)255 } ) {
        const Bytes text = periodic( 60000, period, rng );
        const std::vector<Patterns> sets{
            { slice( text, 0, 1 ) },
            { slice( text, 0, 3 ), slice( text, 0, 3 ) },                                                  /* equal patterns */
            { slice( text, 0, 256 ), slice( text, 0, 1 ) },                                                /* 256 and 1 */
            { slice( text, 0, 5 ), slice( text, 0, 2 ), slice( text, 0, 17 ), slice( text, 0, 3 ), slice( text, 0, 16 ) },   /* a prefix chain */
            { slice( text, 1, 2 ), slice( text, 0, 256 ), slice( text, 1, 2 ), slice( text, 2, 33 ), { '#' }, slice( text, 1, 255 ) },
        };
        for ( const auto& patterns : sets ) {
            uint64_t mMax = 0;
            for ( const auto& pattern : patterns ) mMax = std::max<uint64_t>( mMax, pattern.size() );
            std::vector<uint64_t> kinds{ 0, 1, 2, 3, mMax, mMax + 1, 3 * mMax + 17, 1000 };
            if ( mMax >= 2 ) kinds.push_back( mMax - 1 );
            currentCase = "seeded extent sizes";
            for ( int round = 0; round < 4; ++round ) {
                std::vector<uint64_t> sizes;
                for ( int k = 0; k < 14; ++k ) sizes.push_back( kinds[rng() % kinds.size()] );
                seamCase( text, patterns, sizes, rng() % 300 );
            }
            currentCase = "every size next to every size";
            std::vector<uint64_t> pairs;
            for ( const auto a : kinds ) {
                for ( const auto b : kinds ) {
                    pairs.push_back( a );
                    pairs.push_back( b );
                }
            }
            seamCase( text, patterns, pairs, 7 );
            currentCase = "rows of tiny extents";
            seamCase( text, patterns, { 1000, 1, 1, 1, 1, 1, 1, 1000, 2, 3, 1000, 1, 0, 0, 1, 1000, 0, 1, 2, 1, 0 }, 11 );
            seamCase( text, patterns, std::vector<uint64_t>( 600, 1 ), 0 );
            seamCase( text, patterns, std::vector<uint64_t>( 300, 3 ), 5 );
            currentCase = "two extents that meet at 2^32, and next to it";
            for ( const uint64_t first : { (uint64_t)1000, mMax, (uint64_t)1 } ) {
                const uint64_t cut = uint64_t( 1 ) << 32;
                for ( const uint64_t meet : { cut - 1, cut, cut + 1, cut + mMax - 1 } ) {
                    seamCase( text, patterns, { first, 1000, 1, 1, mMax, 2, 1000, 0, 1, 3 * mMax + 17 }, 13, meet - 13 - first );
                }
            }
            currentCase = "one extent, no extent, empty extents only";
            seamCase( text, patterns, { 5000 }, 3 );
            seamCase( text, patterns, {}, 0 );
            seamCase( text, patterns, { 0, 0, 0 }, 9 );
        }
    }
    currentCase = "coverage";
    CHECK( mostCrossed >= 5 );

    currentCase = "a pair that crosses three extents";
    {
        const char* const words = "....abcdefgh....";
        const Bytes text( words, words + 16 );
        const Patterns patterns{ { 'c', 'd' }, { 'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h' }, { 'd', 'e' }, { 'a' } };
        const auto set = setOf( patterns );
        /* extents [0,6) [6,8) [8,9) [9,16): "abcdefgh" at 4 has bytes of all four and crosses three ends; "cd" at 6 lies
         * inside the second extent, "de" at 7 crosses one end, "a" lies inside the first */
        std::vector<ExtentSeam> seams{ seamOf( text, 0, 6, 8 ), seamOf( text, 6, 2, 8 ), seamOf( text, 8, 1, 8 ), seamOf( text, 9, 7, 8 ) };
        const std::vector<SetMatch> expected{ { 4, 1 }, { 7, 2 } };
        CHECK( seamMatchesSet( set, seams ) == expected );
    }

    currentCase = "argument checks";
    const Bytes text( 100, 'x' );
    const auto set = setOf( { slice( text, 0, 4 ), slice( text, 0, 2 ) } );
    bool thrown = false;
    try {
        (void)seamMatchesSet( set, { seamOf( text, 0, 10, 4 ), seamOf( text, 11, 10, 4 ) } );   /* a gap */
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
    thrown = false;
    try {
        (void)seamMatchesSet( set, { seamOf( text, 0, 10, 2 ) } );   /* head and tail of m_min, not m_max */
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
    thrown = false;
    try {
        (void)seamMatchesSet( PatternSet{}, {} );
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

/* pairsIn over file offsets [from, to) of a file whose bytes are held from file offset `base` on */
std::vector<SetMatch>
pairsAt( const Bytes& file, uint64_t base, uint64_t from, uint64_t to, const Patterns& patterns )
{
    auto found = pairsIn( file, from - base, to - base, patterns );
    for ( auto& pair : found ) pair.first += base;
    return found;
}

/* The merged result of a plan, as the reader computes it.  With a limit: the launches are taken in order until the front
 * holds `limit` safe pairs, the rest is skipped, and the merge is cut.  `base`: `file` holds the decoded bytes from file
 * offset `base` on (a high map's front block is not held, and no range of such a case starts below `base`). */
std::vector<SetMatch>
execute( const SearchPlan& plan, const Bytes& file, const Patterns& patterns, const PatternSet& set, uint64_t limit, size_t* used,
         uint64_t base = 0 )
{
    std::vector<ExtentSeam> seams;
    std::vector<SetMatch> inside;
    uint64_t safe = 0;
    size_t l = 0;
    for ( ; l < plan.extents.size() && ( limit == 0 || safe < limit ); ++l ) {
        const auto& extent = plan.extents[l];
        const auto own = pairsAt( file, base, extent.fileOffset, extent.fileOffset + extent.size, patterns );
        std::vector<uint64_t> positions;
        for ( const auto& pair : own ) positions.push_back( pair.first );
        safe += safePairs( positions.data(), positions.size(), extent.fileOffset + extent.size, set.mMax );
        inside.insert( inside.end(), own.begin(), own.end() );
        seams.push_back( seamOf( file, extent.fileOffset - base, extent.size, set.mMax ) );
        seams.back().fileOffset = extent.fileOffset;
    }
    *used = l;
    const auto between = seamMatchesSet( set, seams );
    std::vector<SetMatch> merged( inside.size() + between.size() );
    std::merge( inside.begin(), inside.end(), between.begin(), between.end(), merged.begin() );
    if ( limit > 0 && merged.size() > limit ) merged.resize( limit );
    return merged;
}

void
planCase( const Map& map, uint64_t fileBytes, const Bytes& file, const Patterns& patterns, uint64_t start, uint64_t end, size_t cap,
          uint64_t base = 0 )
{
    const auto set = setOf( patterns );
    const uint64_t total = base + file.size();
    const uint64_t to = std::min( end, total ), from = std::min( start, to );
    for ( const bool packed : { false, true } ) {
        const auto plan = planSearchSet( map, start, end, set, cap, packed, fileBytes );
        CHECK( plan.extents.size() == plan.launches.size() );
        if ( to - from < set.mMin ) {
            CHECK( plan.launches.empty() && plan.start == plan.end );
            continue;
        }
        CHECK( !plan.launches.empty() && plan.start == from && plan.end == to );
        /* the launches and extents are planSearch's for m_min */
        const auto single = planSearch( map, start, end, set.mMin, cap, packed, fileBytes );
        CHECK( single.extents.size() == plan.extents.size() );
        uint64_t at = from;
        for ( size_t l = 0; l < plan.extents.size() && l < single.extents.size(); ++l ) {
            CHECK( plan.extents[l].fileOffset == at && plan.extents[l].size == single.extents[l].size
                   && plan.extents[l].src == single.extents[l].src && plan.launches[l].bits == single.launches[l].bits );
            at += plan.extents[l].size;
        }
        CHECK( at == to );
        size_t used = 0;
        const auto all = execute( plan, file, patterns, set, 0, &used, base );
        CHECK( used == plan.extents.size() );
        CHECK( all == pairsAt( file, base, from, to, patterns ) );
        CHECK( std::set<SetMatch>( all.begin(), all.end() ).size() == all.size() );
    }
}

void
planCases()
{
    std::mt19937_64 rng( 0x9A75 );
    const std::vector<std::vector<std::vector<uint64_t> > > layouts{
        { { 900, 900, 900, 417 } },
        { { 2, 1 }, {}, { 3 }, { 1 }, { 3, 2, 1, 1 }, {}, { 700 }, { 1, 1, 1, 1, 1, 1, 1, 5 } },   /* streams without a block */
        { { 300, 1, 299 }, { 1 }, { 1 }, { 600, 600 } },
    };
    for ( const auto& layout : layouts ) {
        uint64_t fileBytes = 0;
        const auto map = makeMap( layout, rng, &fileBytes );
        const uint64_t total = map.back().second;
        for ( const size_t period : { (size_t)1, (size_t)3, (size_t)7 } ) {
            const Bytes file = periodic( total, period, rng );
            const std::vector<Patterns> sets{
                { slice( file, 0, 3 ), slice( file, 0, 16 ), slice( file, 0, 3 ), slice( file, 1, 2 ) },      /* m_min 2, m_max 16 */
                { slice( file, 0, 256 ), slice( file, 0, 5 ), slice( file, 0, 255 ) },                        /* m_min 5, m_max 256 */
                { slice( file, 0, 1 ), slice( file, 0, 256 ) },
            };
            for ( const auto& patterns : sets ) {
                const auto set = setOf( patterns );
                const uint64_t mMin = set.mMin, mMax = set.mMax;
                for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
                    currentCase = "whole file, and beyond it";
                    planCase( map, fileBytes, file, patterns, 0, total, cap );
                    planCase( map, fileBytes, file, patterns, 0, ~uint64_t( 0 ), cap );
                    currentCase = "shorter than m_min";
                    planCase( map, fileBytes, file, patterns, 5, 5, cap );
                    planCase( map, fileBytes, file, patterns, 9, 3, cap );
                    planCase( map, fileBytes, file, patterns, 4, 4 + mMin - 1, cap );
                    planCase( map, fileBytes, file, patterns, total, total + 10, cap );
                    planCase( map, fileBytes, file, patterns, total + 1, ~uint64_t( 0 ), cap );
                    currentCase = "between m_min and m_max";
                    planCase( map, fileBytes, file, patterns, 4, 4 + mMin, cap );
                    planCase( map, fileBytes, file, patterns, 4, 4 + ( mMin + mMax ) / 2, cap );
                    planCase( map, fileBytes, file, patterns, 4, 4 + mMax - 1, cap );
                    planCase( map, fileBytes, file, patterns, 4, 4 + mMax, cap );
                    planCase( map, fileBytes, file, patterns, total - std::min<uint64_t>( total, mMax - 1 ), total, cap );
                    currentCase = "seeded ranges that cut the first and the last extent";
                    for ( int k = 0; k < 8; ++k ) {
                        const uint64_t a = rng() % total, b = rng() % ( total + 3 );
                        planCase( map, fileBytes, file, patterns, std::min( a, b ), std::max( a, b ), cap );
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
            const Bytes file = periodic( total - base, 3, rng );
            const std::vector<Patterns> sets{
                { slice( file, 0, 3 ), slice( file, 0, 16 ), slice( file, 0, 3 ), slice( file, 1, 2 ) },
                { slice( file, 0, 1 ), slice( file, 0, 256 ) },
            };
            for ( const auto& patterns : sets ) {
                const uint64_t mMax = setOf( patterns ).mMax;
                for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
                    currentCase = "high: everything behind the front, and beyond the size";
                    planCase( map, fileBytes, file, patterns, base, total, cap, base );
                    planCase( map, fileBytes, file, patterns, base, ~uint64_t( 0 ), cap, base );
                    currentCase = "high: ranges that end and start at 2^32 and next to it";
                    for ( const uint64_t edge : { cut - 1, cut, cut + 1, cut + mMax - 1, cut + mMax } ) {
                        planCase( map, fileBytes, file, patterns, base, edge, cap, base );
                        planCase( map, fileBytes, file, patterns, edge, total, cap, base );
                        planCase( map, fileBytes, file, patterns, edge > base + mMax ? edge - mMax : base, edge, cap, base );
                    }
                    currentCase = "high: seeded ranges";
                    for ( int r = 0; r < 6; ++r ) {
                        const uint64_t a = base + rng() % ( total - base ), b = base + rng() % ( total - base + 3 );
                        planCase( map, fileBytes, file, patterns, std::min( a, b ), std::max( a, b ), cap, base );
                    }
                }
            }
        }
    }
    currentCase = "an empty file";
    const Map empty{ { 32, 0 }, { 80, 0 } };
    planCase( empty, 14, {}, { { 'a' } }, 0, 10, 4 );
    planCase( {}, 0, {}, { { 'a' } }, 0, ~uint64_t( 0 ), 4 );
    currentCase = "not a set";
    bool thrown = false;
    try {
        (void)planSearchSet( empty, 0, 10, PatternSet{}, 4, false, 14 );
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
}

/* The limit rule on blocks of 1000 bytes, one per launch, that start at decoded offset `base` (0, or behind a front block that
 * ends there): L (200 bytes) crosses the first boundary from base + 900, S = L[50:52] lies inside the first extent at
 * base + 950 and elsewhere: (base + 900, L) sorts in front of (base + 950, S) but only the second launch shows it. */
void
limitRule( uint64_t base, std::mt19937_64& rng )
{
    const uint64_t cut = uint64_t( 1 ) << 32;
    uint64_t fileBytes = 0;
    const auto map = base == 0 ? makeMap( { { 1000, 1000, 1000, 1000, 500 } }, rng, &fileBytes )
                               : makeMap( { { 1000, 1000, 1000, 1000, 500 } }, rng, &fileBytes, base, cut - 8 * 9 );
    Bytes file( 4500 );
    for ( size_t i = 0; i < file.size(); ++i ) file[i] = (uint8_t)( 'a' + ( i * 7 + i / 13 ) % 23 );
    Bytes big( 200 );
    for ( size_t i = 0; i < big.size(); ++i ) big[i] = (uint8_t)( 'A' + i % 26 );
    std::copy( big.begin(), big.end(), file.begin() + 900 );
    std::copy( big.begin(), big.end(), file.begin() + 2950 );
    const Bytes tiny = slice( big, 50, 2 );
    for ( const size_t at : { (size_t)100, (size_t)200, (size_t)300, (size_t)700, (size_t)1500, (size_t)1700, (size_t)2500, (size_t)3990 } ) std::copy( tiny.begin(), tiny.end(), file.begin() + at );
    for ( const bool longFirst : { true, false } ) {
        const Patterns patterns = longFirst ? Patterns{ big, tiny } : Patterns{ tiny, big };
        const auto set = setOf( patterns );
        for ( const size_t cap : { (size_t)1, (size_t)2 } ) {
            const auto plan = planSearchSet( map, base, ~uint64_t( 0 ), set, cap, false, fileBytes );
            size_t used = 0;
            const auto all = execute( plan, file, patterns, set, 0, &used, base );
            CHECK( all == pairsAt( file, base, base, base + file.size(), patterns ) && all.size() >= 10 );
            CHECK( base == 0 || ( all.front().first < cut && all.back().first > cut ) );
            bool skipped = false;
            for ( uint64_t limit = 1; limit <= all.size() + 1; ++limit ) {
                const auto some = execute( plan, file, patterns, set, limit, &used, base );
                const auto n = (size_t)std::min<uint64_t>( limit, all.size() );
                CHECK( some == std::vector<SetMatch>( all.begin(), all.begin() + n ) );
                skipped = skipped || used < plan.extents.size();
            }
            CHECK( skipped );    /* the rule does stop launches */
        }
    }
}

void
limitCases()
{
    currentCase = "safePairs";
    std::mt19937_64 rng( 0x11417 );
    for ( int round = 0; round < 200; ++round ) {
        std::vector<uint64_t> positions;
        uint64_t p = rng() % 50;
        for ( int k = 0; k < (int)( rng() % 40 ); ++k ) positions.push_back( p += rng() % 3 );   /* repeats: several ids at one p */
        const uint64_t end = rng() % 120;
        const uint32_t mMax = 1 + rng() % 60;
        uint64_t expected = 0;
        for ( const auto q : positions ) expected += q + mMax <= end ? 1 : 0;
        CHECK( safePairs( positions.data(), positions.size(), end, mMax ) == expected );
    }

    currentCase = "the limit rule";
    /* base 0, and behind a front block: the first block ends exactly at 2^32 (L crosses 2^32 from 2^32 - 100), the third
     * does (the second L crosses it, and limits are reached above it), and 2^32 lies inside the first block */
    const uint64_t cut = uint64_t( 1 ) << 32;
    for ( const uint64_t base : { (uint64_t)0, cut - 1000, cut - 3000, cut - 500 } ) limitRule( base, rng );
}

void
imageAndLimits()
{
    currentCase = "writeSetImage";
    std::mt19937_64 rng( 0x1A6E );
    for ( int round = 0; round < 20; ++round ) {
        Patterns patterns;
        size_t sum = 0;
        const size_t k = round == 0 ? 1 : round == 1 ? 1024 : 1 + rng() % 300;
        for ( size_t i = 0; i < k; ++i ) {
            const size_t m = round == 1 ? 16 : 1 + rng() % ( i % 7 == 0 ? 256 : 20 );
            if ( sum + m > SET_MAX_BYTES ) break;
            Bytes pattern( m );
            for ( auto& byte : pattern ) byte = (uint8_t)( round == 2 ? rng() % 3 : rng() );
            if ( round == 3 && i < 256 ) pattern[0] = (uint8_t)i;    /* every first byte */
            patterns.push_back( pattern );
            sum += m;
        }
        const auto set = setOf( patterns );
        std::vector<uint32_t> image( SET_IMAGE_BYTES / 4 + 1, 0xDEADBEEFu );
        auto* const bytes = reinterpret_cast<uint8_t*>( image.data() );
        writeSetImage( set, bytes );
        CHECK( image.back() == 0xDEADBEEFu );
        const uint32_t* const table = image.data() + SET_TABLE_AT / 4;
        const uint32_t* const first = image.data() + SET_FIRST_AT / 4;
        std::vector<int> seen( patterns.size(), 0 );
        size_t entries = 0;
        for ( uint32_t byte = 0; byte < 256; ++byte ) {
            const uint32_t begin = first[byte] & 0xFFFFu, length = first[byte] >> 16;
            CHECK( ( first[byte] == 0 ) == ( length == 0 ) );
            CHECK( begin == ( length == 0 ? 0 : entries ) );    /* the buckets lie back to back in byte order */
            entries += length;
            uint32_t lastId = 0;
            for ( uint32_t e = begin; e < begin + length; ++e ) {
                const uint32_t offset = table[e] & ( SET_MAX_BYTES - 1 ), m = ( ( table[e] >> SET_ENTRY_SIZE_SHIFT ) & 0xFFu ) + 1;
                const uint32_t id = table[e] >> SET_ENTRY_ID_SHIFT;
                CHECK( id < patterns.size() );
                if ( id >= patterns.size() ) continue;
                CHECK( e == begin || id > lastId );
                lastId = id;
                ++seen[id];
                CHECK( m == patterns[id].size() && patterns[id][0] == byte && offset + m <= SET_MAX_BYTES
                       && std::memcmp( bytes + offset, patterns[id].data(), m ) == 0 );
            }
        }
        CHECK( entries == patterns.size() );
        for ( const auto n : seen ) CHECK( n == 1 );
    }

    currentCase = "the limits";
    std::vector<uint32_t> sizes( 1025, 16 );
    CHECK( patternSetError( sizes.data(), 1024 ).empty() );                                  /* 1024 x 16 = 16384 */
    CHECK( patternSetError( sizes.data(), 0 ).find( "1 to 1024 patterns" ) != std::string::npos );
    CHECK( patternSetError( sizes.data(), 1025 ).find( "1 to 1024 patterns" ) != std::string::npos );
    sizes[7] = 17;
    CHECK( patternSetError( sizes.data(), 1024 ).find( "at most 16384 bytes" ) != std::string::npos );
    sizes[7] = 0;
    CHECK( patternSetError( sizes.data(), 1024 ).find( "1 to 256 bytes, pattern 7" ) != std::string::npos );
    sizes[7] = 257;
    CHECK( patternSetError( sizes.data(), 10 ).find( "1 to 256 bytes, pattern 7" ) != std::string::npos );
    sizes[7] = 256;
    CHECK( patternSetError( sizes.data(), 10 ).empty() );
    bool thrown = false;
    try {
        const Bytes bytes( 300, 'x' );
        const uint32_t bad = 257;
        (void)makePatternSet( bytes.data(), &bad, 1 );
    } catch ( const std::invalid_argument& ) {
        thrown = true;
    }
    CHECK( thrown );
}
}  // namespace

int
main()
{
    seamCases();
    planCases();
    limitCases();
    imageAndLimits();
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "search set ok\n" );
    return 0;
}
