/* planLineNumbers (bz2_lines.hpp) against a byte-by-byte restatement.
 *
 * The plan is executed on the CPU the way the reader executes it on the GPU: every launch's ragged output is laid out from
 * the plan's own launches, every query's rank is counted byte by byte in its span of that output, and the answers put
 * together from the ranks must be L(p) = the number of delimiters in file[0 : min( p, size )], counted byte by byte in the
 * file.  Beside the answers: every block appears in one launch only and only blocks that need a query are launched, in
 * file order, at most `cap` per launch; queries are distinct, lie in their block's span, come launch by launch; an offset
 * at a block's first byte, at or beyond the size, or in an empty file has none; and every queried block carries exactly
 * one query at its span's end whose expected rank is the block's count in the index.  Offsets: block starts and the bytes
 * around them, the size and beyond, duplicates, seeded unsorted ones; blocks without delimiters, streams without blocks,
 * an empty file; caps 1, 3 and 512; plain and packed launches.
 *
 * Offsets at and across 2^32 (highCases): the same layouts behind a front block of 2^32 - k bytes without a delimiter,
 * whose bytes are never held in memory (File::front), the bit offsets of what follows starting just below 2^32.  With an
 * offset inside the front block that block is launched, and every span offset and position behind it in that launch
 * lies above 2^32; the line index has entries on both sides.  Prints "linenum ok". */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_lines.hpp"

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
constexpr uint8_t NL = '\n';

/* the decoded file: `front` bytes 'x' that are not held in memory, then `tail` */
struct File
{
    uint64_t front{ 0 };
    Bytes tail;
    uint64_t size() const { return front + tail.size(); }
    uint8_t operator[]( uint64_t p ) const { return p < front ? (uint8_t)'x' : tail[p - front]; }
};

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

/* byte by byte, but for the front, which holds no delimiter */
uint64_t
countIn( const File& file, uint64_t from, uint64_t to )
{
    uint64_t count = 0;
    for ( uint64_t p = std::max( from, file.front ); p < to; ++p ) count += file[p] == NL ? 1 : 0;
    return count;
}

void
planCase( const Map& map, uint64_t fileBytes, const File& file, const std::vector<uint64_t>& offsets, size_t cap )
{
    /* the data blocks and the line index, from the map and the file alone */
    std::vector<uint64_t> starts, lengths, blockBits, indexBytes, indexLines;
    for ( size_t i = 0; i + 1 < map.size(); ++i ) {
        if ( map[i + 1].second > map[i].second ) {
            starts.push_back( map[i].second );
            lengths.push_back( map[i + 1].second - map[i].second );
            blockBits.push_back( map[i].first );
        }
    }
    const uint64_t total = file.size();
    for ( const auto start : starts ) {
        indexBytes.push_back( start );
        indexLines.push_back( countIn( file, 0, start ) );
    }
    indexBytes.push_back( total );
    indexLines.push_back( countIn( file, 0, total ) );

    for ( const bool packed : { false, true } ) {
        const auto plan = planLineNumbers( map, indexBytes.data(), indexLines.data(), indexBytes.size(), offsets.data(),
                                           offsets.size(), cap, packed, fileBytes );
        CHECK( plan.answers.size() == offsets.size() );

        /* the blocks that hold an offset which is not their first byte */
        std::set<size_t> wanted;
        for ( const auto p : offsets ) {
            if ( p >= total ) continue;
            const size_t b = (size_t)( std::upper_bound( starts.begin(), starts.end(), p ) - starts.begin() ) - 1;
            if ( p != starts[b] ) wanted.insert( b );
        }
        std::vector<uint64_t> wantedBits;
        for ( const auto b : wanted ) wantedBits.push_back( blockBits[b] );

        /* the launches' outputs; each block once, in file order */
        std::vector<uint64_t> launchedBits;
        std::vector<uint64_t> outputs;      /* their sizes: block b's bytes in a launch are file[starts[b], +lengths[b]) */
        std::map<std::pair<uint32_t, uint64_t>, size_t> blockAt;   /* {launch, span offset} -> block */
        for ( size_t l = 0; l < plan.launches.size(); ++l ) {
            const auto& launch = plan.launches[l];
            CHECK( !launch.bits.empty() && launch.bits.size() <= cap );
            CHECK( packed == !launch.windows.empty() );
            uint64_t output = 0;
            for ( size_t k = 0; k < launch.bits.size(); ++k ) {
                const size_t b = (size_t)( std::find( blockBits.begin(), blockBits.end(), launch.bits[k] ) - blockBits.begin() );
                CHECK( b < blockBits.size() );
                if ( b >= blockBits.size() ) return;
                launchedBits.push_back( launch.bits[k] );
                CHECK( launch.outOffsets[k] == output && launch.sizes[k] == lengths[b] );
                blockAt[{ (uint32_t)l, output }] = b;
                output += lengths[b];
            }
            CHECK( launch.outBytes == output );
            outputs.push_back( output );
        }
        CHECK( launchedBits == wantedBits );
        CHECK( plan.distinctBlocks == wanted.size() );

        /* the queries: distinct, inside their spans, launch by launch; their ranks byte by byte */
        std::vector<uint64_t> ranks( plan.queries.size(), 0 );
        std::set<std::pair<size_t, uint64_t> > seen;
        std::map<size_t, int> endQueries;
        for ( size_t q = 0; q < plan.queries.size(); ++q ) {
            const auto& query = plan.queries[q];
            CHECK( query.launch < outputs.size() );
            if ( query.launch >= outputs.size() ) return;
            CHECK( q == 0 || plan.queries[q - 1].launch <= query.launch );
            const uint64_t output = outputs[query.launch];
            const auto at = blockAt.find( { query.launch, query.spanOffset } );
            CHECK( at != blockAt.end() );
            if ( at == blockAt.end() ) return;
            const size_t b = at->second;
            CHECK( query.spanSize == lengths[b] && query.blockStart == starts[b] );
            CHECK( query.spanOffset + query.spanSize <= output );
            CHECK( query.position > query.spanOffset && query.position <= query.spanOffset + query.spanSize );
            if ( query.position > output ) return;
            CHECK( seen.insert( { b, query.position - query.spanOffset } ).second || query.expected != NOT_FOUND );
            /* the launch's bytes [spanOffset, position) are the block's first position - spanOffset bytes */
            ranks[q] = countIn( file, starts[b], starts[b] + ( query.position - query.spanOffset ) );
            if ( query.expected != NOT_FOUND ) {
                ++endQueries[b];
                CHECK( query.position == query.spanOffset + query.spanSize );
                CHECK( query.expected == indexLines[b + 1] - indexLines[b] );
                CHECK( ranks[q] == query.expected );
            }
        }
        /* every queried block carries exactly one end-of-span query */
        CHECK( endQueries.size() == wanted.size() );
        for ( const auto b : wanted ) CHECK( endQueries[b] == 1 );

        /* the answers */
        for ( size_t i = 0; i < offsets.size(); ++i ) {
            const auto& answer = plan.answers[i];
            const uint64_t p = offsets[i];
            const bool needsNone = p >= total || std::binary_search( starts.begin(), starts.end(), p );
            CHECK( needsNone == ( answer.query == NO_QUERY ) );
            CHECK( answer.query == NO_QUERY || answer.query < plan.queries.size() );
            if ( answer.query != NO_QUERY && answer.query >= plan.queries.size() ) return;
            if ( answer.query != NO_QUERY ) {
                const auto& query = plan.queries[answer.query];
                CHECK( query.expected == NOT_FOUND );   /* an offset inside the file never lies at a span's end */
                CHECK( query.blockStart + ( query.position - query.spanOffset ) == p );
            }
            CHECK( lineNumberOf( answer, ranks.data() ) == countIn( file, 0, std::min( p, total ) ) );
        }
    }
}

File
makeFile( uint64_t total, const std::vector<std::pair<uint64_t, uint64_t> >& bare, std::mt19937_64& rng, uint64_t front = 0 )
{
    File file{ front, Bytes( total - front ) };
    for ( auto& byte : file.tail ) byte = rng() % 7 == 0 ? NL : (uint8_t)( 'a' + rng() % 26 );
    for ( const auto& [from, to] : bare ) {
        for ( uint64_t p = std::max( from, front ); p < to && p < total; ++p ) file.tail[p - front] = 'x';   /* no delimiter */
    }
    return file;
}

void
planCases()
{
    std::mt19937_64 rng( 0x11E5 );
    const std::vector<std::vector<std::vector<uint64_t> > > layouts{
        { { 900, 900, 900, 417 } },
        { { 2, 1 }, {}, { 3 }, { 1 }, { 3, 2, 1, 1 }, {}, { 700 }, { 1, 1, 1, 1, 1, 1, 1, 5 } },   /* streams without a block */
        { { 300, 1, 299 }, { 1 }, { 1 }, { 600, 600 } },
    };
    for ( const auto& layout : layouts ) {
        uint64_t fileBytes = 0;
        const auto map = makeMap( layout, rng, &fileBytes );
        const uint64_t total = map.back().second;
        std::vector<uint64_t> starts;
        for ( size_t i = 0; i + 1 < map.size(); ++i ) {
            if ( map[i + 1].second > map[i].second ) starts.push_back( map[i].second );
        }
        /* blocks 1 and 2 (where there are that many bytes) without a delimiter */
        const auto file = makeFile( total, { { starts[1], starts.size() > 3 ? starts[3] : total } }, rng );
        for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
            currentCase = "no offsets";
            planCase( map, fileBytes, file, {}, cap );
            currentCase = "block starts, their neighbours, the size and beyond";
            std::vector<uint64_t> offsets;
            for ( const auto start : starts ) {
                offsets.push_back( start );
                if ( start > 0 ) offsets.push_back( start - 1 );
                offsets.push_back( start + 1 );
            }
            for ( const uint64_t p : { (uint64_t)0, total - 1, total, total + 5, ~uint64_t( 0 ) } ) offsets.push_back( p );
            planCase( map, fileBytes, file, offsets, cap );
            currentCase = "only block starts and offsets beyond the size: no launch";
            {
                std::vector<uint64_t> fixed( starts );
                fixed.push_back( total );
                fixed.push_back( total + 1 );
                planCase( map, fileBytes, file, fixed, cap );
            }
            currentCase = "every offset, ascending and descending";
            std::vector<uint64_t> all( total + 2 );
            for ( uint64_t p = 0; p < all.size(); ++p ) all[p] = p;
            planCase( map, fileBytes, file, all, cap );
            std::reverse( all.begin(), all.end() );
            planCase( map, fileBytes, file, all, cap );
            currentCase = "seeded offsets, unsorted, with duplicates";
            for ( int round = 0; round < 8; ++round ) {
                std::vector<uint64_t> seeded;
                const size_t n = 1 + rng() % 40;
                for ( size_t k = 0; k < n; ++k ) seeded.push_back( rng() % ( total + 3 ) );
                for ( size_t k = 0; k < n / 3; ++k ) seeded.push_back( seeded[rng() % seeded.size()] );
                std::shuffle( seeded.begin(), seeded.end(), rng );
                planCase( map, fileBytes, file, seeded, cap );
            }
            currentCase = "one block's last byte only";
            planCase( map, fileBytes, file, { starts[1] - 1 }, cap );
            planCase( map, fileBytes, file, { total - 1, total - 1 }, cap );
        }
    }
    currentCase = "an empty file";
    const Map empty{ { 32, 0 }, { 80, 0 } };
    planCase( empty, 14, File{}, { 0, 1, 7, ~uint64_t( 0 ) }, 4 );
    planCase( empty, 14, File{}, {}, 4 );
    currentCase = "a line index that does not fit the map is refused";
    {
        uint64_t fileBytes = 0;
        const auto map = makeMap( { { 10, 10 } }, rng, &fileBytes );
        const uint64_t bytes[] = { 0, 10, 20 }, lines[] = { 0, 11, 12 }, offsets[] = { 3 };
        bool thrown = false;
        try {
            (void)planLineNumbers( map, bytes, lines, 3, offsets, 1, 4, false, fileBytes );
        } catch ( const std::invalid_argument& ) {
            thrown = true;
        }
        CHECK( thrown );
    }
}

/* the layouts behind a front block of 2^32 - k bytes: offsets, index entries, span offsets and positions on both sides */
void
highCases()
{
    std::mt19937_64 rng( 0x41E5 );
    const uint64_t cut = uint64_t( 1 ) << 32;
    const std::vector<std::vector<std::vector<uint64_t> > > layouts{
        { { 900, 900, 900, 417 } },
        { { 2, 1 }, {}, { 3 }, { 1 }, { 3, 2, 1, 1 }, {}, { 700 }, { 1, 1, 1, 1, 1, 1, 1, 5 } },
        { { 300, 1, 299 }, { 1 }, { 1 }, { 600, 600 } },
    };
    for ( const auto& layout : layouts ) {
        for ( const uint64_t k : { (uint64_t)1, (uint64_t)450, (uint64_t)900 } ) {
            uint64_t fileBytes = 0;
            const uint64_t front = cut - k;
            const auto map = makeMap( layout, rng, &fileBytes, front, cut - 8 * ( 5 + rng() % 100 ) );
            const uint64_t total = map.back().second;
            std::vector<uint64_t> starts;
            for ( size_t i = 0; i + 1 < map.size(); ++i ) {
                if ( map[i + 1].second > map[i].second ) starts.push_back( map[i].second );
            }
            if ( total <= cut ) continue;      /* the layout has fewer than k bytes */
            currentCase = "high: the layout";
            CHECK( starts[0] == 0 && starts[1] == front && map.back().first > cut );
            const auto file = makeFile( total, { { starts[2], starts.size() > 4 ? starts[4] : total } }, rng, front );
            for ( const size_t cap : { (size_t)1, (size_t)3, (size_t)512 } ) {
                for ( const bool touchFront : { false, true } ) {
                    /* an offset inside the front block launches it: what follows it in a launch lies above 2^32 */
                    const std::vector<uint64_t> inFront = touchFront ? std::vector<uint64_t>{ 1, front - 1, cut / 2 }
                                                                    : std::vector<uint64_t>{ 0 };
                    currentCase = touchFront ? "high, front launched: block starts and their neighbours"
                                             : "high: block starts and their neighbours";
                    std::vector<uint64_t> offsets( inFront );
                    for ( size_t b = 1; b < starts.size(); ++b ) {
                        offsets.push_back( starts[b] );
                        if ( b > 1 ) offsets.push_back( starts[b] - 1 );
                        offsets.push_back( starts[b] + 1 );
                    }
                    for ( const uint64_t p : { cut - 1, cut, cut + 1, total - 1, total, total + 5, ~uint64_t( 0 ) } ) {
                        if ( p >= front ) offsets.push_back( p );
                    }
                    planCase( map, fileBytes, file, offsets, cap );
                    currentCase = touchFront ? "high, front launched: every offset behind the front" : "high: every offset behind the front";
                    std::vector<uint64_t> all( inFront );
                    for ( uint64_t p = front; p < total + 2; ++p ) all.push_back( p );
                    planCase( map, fileBytes, file, all, cap );
                    std::reverse( all.begin(), all.end() );
                    planCase( map, fileBytes, file, all, cap );
                    currentCase = touchFront ? "high, front launched: seeded offsets" : "high: seeded offsets";
                    for ( int round = 0; round < 4; ++round ) {
                        std::vector<uint64_t> seeded( inFront );
                        const size_t n = 1 + rng() % 40;
                        for ( size_t i = 0; i < n; ++i ) seeded.push_back( front + rng() % ( total - front + 3 ) );
                        for ( size_t i = 0; i < n / 3; ++i ) seeded.push_back( seeded[rng() % seeded.size()] );
                        std::shuffle( seeded.begin(), seeded.end(), rng );
                        planCase( map, fileBytes, file, seeded, cap );
                    }
                }
            }
        }
    }
}

/* millions of ascending offsets must not take quadratic time: this finishes in a blink or not at all */
void
largeCase()
{
    currentCase = "two million ascending offsets";
    std::mt19937_64 rng( 7 );
    uint64_t fileBytes = 0;
    std::vector<uint64_t> blocks( 400, 900000 );
    const auto map = makeMap( { blocks }, rng, &fileBytes );
    const uint64_t total = map.back().second;
    std::vector<uint64_t> indexBytes, indexLines;
    for ( size_t b = 0; b <= blocks.size(); ++b ) {
        indexBytes.push_back( b * 900000 );
        indexLines.push_back( b * 1000 );
    }
    std::vector<uint64_t> offsets( 2000000 );
    for ( size_t i = 0; i < offsets.size(); ++i ) offsets[i] = i * ( total / offsets.size() ) + 1;
    const auto plan = planLineNumbers( map, indexBytes.data(), indexLines.data(), indexBytes.size(), offsets.data(),
                                       offsets.size(), 512, true, fileBytes );
    CHECK( plan.launches.size() == 1 && plan.distinctBlocks == 400 );
    CHECK( plan.queries.size() == offsets.size() + 400 );
    CHECK( plan.answers.back().query != NO_QUERY );
}
}  // namespace

int
main()
{
    planCases();
    highCases();
    largeCase();
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "linenum ok\n" );
    return 0;
}
