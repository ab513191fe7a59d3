/* The line planner (bz2_lines.hpp) against a byte-by-byte restatement.  A file is a vector of bytes with delimiters where
 * the case wants them; the line index is counted from it block by block; the expected bytes of a range come from a scan
 * of the whole file (s(k) = 1 + position of the k-th delimiter).  The plan is then executed on the CPU the way the reader
 * executes it on the GPU: every launch's ragged output is laid out from the plan's own launches, every query is answered
 * by a scan of its span in that output, every segment is resolved with those answers, and the pieces of a range, in
 * order, must be the expected bytes.  The blocks launched must be exactly those from the block that holds the first-th
 * delimiter (the first block for first == 0) through the one that holds the (first + count)-th (the last block when
 * there is none), each once, in launches of at most the cap.
 * Maps: hand-written ones with end-of-stream entries and two streams, an empty file, and seeded ones.  Cases: blocks
 * without any delimiter, a line spanning several blocks and a launch boundary, a delimiter on a block's last byte, first
 * equal to N and greater than N, count 0 and huge, cap 1, a file that ends with a delimiter, a file of delimiters only.
 * Also: line_starts plans, the checks of an imported index, and an index that lies.
 *
 * Offsets at and across 2^32: the hand-written and some seeded cases once more behind a front block of 2^32 - k bytes
 * without a delimiter.  Those bytes are never held in memory: a File knows its front, a launch's output is the list of the
 * file's stretches it holds, and a range's bytes are compared as stretches of the file (every block is launched once, so
 * equal stretches are equal bytes).  Line 0 then spans the front block, a launch that holds it puts every later span,
 * query position and segment above 2^32, and the line index has entries on both sides.  Prints "lines ok". */
#include <algorithm>
#include <cstdio>
#include <cstdlib>
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
constexpr uint8_t NL = '\n';

/* the decoded file: `front` bytes 'x' that are not held in memory, then `tail` */
struct File
{
    uint64_t front{ 0 };
    std::vector<uint8_t> tail;
    File() = default;
    File( std::vector<uint8_t> bytes, uint64_t frontBytes = 0 ) : front( frontBytes ), tail( std::move( bytes ) ) {}
    uint64_t size() const { return front + tail.size(); }
    uint8_t operator[]( uint64_t p ) const { return p < front ? (uint8_t)'x' : tail[p - front]; }
};

using Stretches = std::vector<std::pair<uint64_t, uint64_t> >;   /* [from, to) of the file, in order; neighbours joined */

void
append( Stretches& stretches, uint64_t from, uint64_t to )
{
    if ( from == to ) return;
    if ( !stretches.empty() && stretches.back().second == from ) {
        stretches.back().second = to;
    } else {
        stretches.push_back( { from, to } );
    }
}

/* a launch's ragged output: block by block, the stretch of the file it holds */
struct Output
{
    std::vector<uint64_t> at, from, length;
    uint64_t bytes{ 0 };
    uint64_t size() const { return bytes; }
    void add( uint64_t fileFrom, uint64_t n ) { at.push_back( bytes ); from.push_back( fileFrom ); length.push_back( n ); bytes += n; }
    /* the part holding output byte x (x < size()) */
    size_t partOf( uint64_t x ) const { return (size_t)( std::upper_bound( at.begin(), at.end(), x ) - at.begin() ) - 1; }
    uint64_t fileOffset( uint64_t x ) const { const size_t k = partOf( x ); return from[k] + ( x - at[k] ); }
    /* output bytes [src, src + n) as stretches of the file */
    void stretches( uint64_t src, uint64_t n, Stretches& out ) const
    {
        while ( n > 0 ) {
            const size_t k = partOf( src );
            const uint64_t take = std::min( n, at[k] + length[k] - src );
            append( out, from[k] + ( src - at[k] ), from[k] + ( src - at[k] ) + take );
            src += take;
            n -= take;
        }
    }
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

struct Blocks
{
    std::vector<uint64_t> bits, starts, lengths;
};

Blocks
blocksOf( const Map& map )
{
    Blocks blocks;
    for ( size_t i = 0; i + 1 < map.size(); ++i ) {
        if ( map[i + 1].second > map[i].second ) {
            blocks.bits.push_back( map[i].first );
            blocks.starts.push_back( map[i].second );
            blocks.lengths.push_back( map[i + 1].second - map[i].second );
        }
    }
    return blocks;
}

void
indexOf( const Map& map, const File& file, std::vector<uint64_t>& bytes, std::vector<uint64_t>& lines )
{
    const auto blocks = blocksOf( map );
    bytes = blocks.starts;
    bytes.push_back( file.size() );
    lines.assign( 1, 0 );
    for ( size_t b = 0; b < blocks.starts.size(); ++b ) {
        uint64_t count = 0;
        for ( uint64_t x = std::max( blocks.starts[b], file.front ); x < blocks.starts[b] + blocks.lengths[b]; ++x ) {
            count += file[x] == NL;      /* (the front holds no delimiter) */
        }
        lines.push_back( lines.back() + count );
    }
}

/* block (index into Blocks) holding decoded byte x: a brute-force walk */
size_t
blockHolding( const Blocks& blocks, uint64_t x )
{
    for ( size_t b = 0; b < blocks.starts.size(); ++b ) {
        if ( blocks.starts[b] <= x && x < blocks.starts[b] + blocks.lengths[b] ) return b;
    }
    return SIZE_MAX;
}

struct Executed
{
    std::vector<Output> outputs;                  /* per launch */
    std::vector<uint64_t> positions;              /* per query */
    std::vector<uint64_t> launched;               /* bit offsets, in launch order */
};

/* what the GPU does with a plan: decode the launches, answer the queries */
Executed
execute( const LinePlan& plan, const Map& map, const File& file, size_t cap, bool packed )
{
    Executed run;
    for ( size_t l = 0; l < plan.launches.size(); ++l ) {
        const auto& launch = plan.launches[l];
        CHECK( !launch.bits.empty() && launch.bits.size() <= cap );
        if ( l + 1 < plan.launches.size() ) CHECK( launch.bits.size() == cap );
        CHECK( packed ? launch.packedBits.size() == launch.bits.size() && !launch.windows.empty() : launch.windows.empty() );
        Output out;
        for ( size_t k = 0; k < launch.bits.size(); ++k ) {
            if ( !run.launched.empty() ) CHECK( run.launched.back() < launch.bits[k] );
            run.launched.push_back( launch.bits[k] );
            size_t e = 0;
            while ( map[e].first != launch.bits[k] ) ++e;
            CHECK( launch.sizes[k] == map[e + 1].second - map[e].second );
            CHECK( launch.outOffsets[k] == out.size() );
            out.add( map[e].second, map[e + 1].second - map[e].second );
        }
        CHECK( launch.outBytes == out.size() );
        run.outputs.push_back( std::move( out ) );
    }
    CHECK( plan.distinctBlocks == run.launched.size() );
    for ( const auto& q : plan.queries ) {
        uint64_t position = NOT_FOUND;
        CHECK( q.launch < run.outputs.size() && q.rank >= 1 );
        if ( q.launch < run.outputs.size() ) {
            const auto& out = run.outputs[q.launch];
            CHECK( q.spanOffset + q.spanSize <= out.size() );
            uint64_t seen = 0;
            for ( uint64_t x = q.spanOffset; x < q.spanOffset + q.spanSize && x < out.size(); ++x ) {
                const uint64_t p = out.fileOffset( x );
                if ( p < file.front ) {
                    /* no delimiter in the front: on to its end, or to the end of this part of the output */
                    const size_t k = out.partOf( x );
                    x += std::min( file.front - p, out.at[k] + out.length[k] - x ) - 1;
                    continue;
                }
                if ( file[p] == NL && ++seen == q.rank ) {
                    position = x;
                    break;
                }
            }
        }
        run.positions.push_back( position );
    }
    return run;
}

void
checkRanges( const Map& map, uint64_t fileBytes, const File& file, const std::vector<uint64_t>& first,
             const std::vector<uint64_t>& count, size_t cap, bool packed )
{
    std::vector<uint64_t> indexBytes, indexLines;
    indexOf( map, file, indexBytes, indexLines );
    const auto blocks = blocksOf( map );
    const size_t n = first.size();
    const auto plan = planLines( map, indexBytes.data(), indexLines.data(), indexBytes.size(), first.data(), count.data(), n,
                                 false, cap, packed, fileBytes );

    /* s(k) by a scan of the file */
    std::vector<uint64_t> s( 1, 0 );
    for ( uint64_t x = file.front; x < file.size(); ++x ) {
        if ( file[x] == NL ) s.push_back( x + 1 );
    }
    const uint64_t N = s.size() - 1;
    CHECK( indexLines.back() == N );

    /* the blocks the ranges span, by the definition */
    std::set<uint64_t> needed;
    std::set<uint64_t> distinctBoundaries;
    for ( size_t i = 0; i < n; ++i ) {
        if ( first[i] > N || count[i] == 0 || blocks.starts.empty() ) continue;
        const bool toTheEnd = count[i] > N - first[i];
        const size_t from = first[i] == 0 ? 0 : blockHolding( blocks, s[first[i]] - 1 );
        const size_t to = toTheEnd ? blocks.starts.size() - 1 : blockHolding( blocks, s[first[i] + count[i]] - 1 );
        for ( size_t b = from; b <= to; ++b ) needed.insert( blocks.bits[b] );
        if ( first[i] != 0 ) distinctBoundaries.insert( first[i] );
        if ( !toTheEnd ) distinctBoundaries.insert( first[i] + count[i] );
    }
    const auto run = execute( plan, map, file, cap, packed );
    CHECK( std::vector<uint64_t>( needed.begin(), needed.end() ) == run.launched );
    /* one query per distinct boundary that has to be looked for: none for line 0, none beyond the last delimiter */
    CHECK( plan.queries.size() == distinctBoundaries.size() );
    for ( size_t q = 0; q < plan.queries.size(); ++q ) {
        CHECK( run.positions[q] != NOT_FOUND );
        CHECK( plan.queries[q].blockCount >= plan.queries[q].rank );
    }

    /* the ranges' bytes from the segments, in order */
    std::vector<Stretches> got( n );
    uint32_t lastRange = 0;
    for ( const auto& segment : plan.segments ) {
        CHECK( segment.range < n && segment.range >= lastRange && segment.launch < run.outputs.size() );
        if ( segment.range >= n || segment.launch >= run.outputs.size() ) continue;
        lastRange = segment.range;
        uint64_t src = 0, size = 0;
        const bool ok = resolveSegment( plan, segment, run.positions.data(), &src, &size );
        CHECK( ok );
        if ( !ok ) continue;
        const auto& out = run.outputs[segment.launch];
        CHECK( src + size <= out.size() );
        if ( src + size > out.size() ) continue;
        out.stretches( src, size, got[segment.range] );
    }
    for ( size_t i = 0; i < n; ++i ) {
        Stretches want;
        if ( first[i] <= N && count[i] != 0 ) {
            const uint64_t from = s[first[i]];
            const uint64_t to = count[i] > N - first[i] ? file.size() : s[first[i] + count[i]];
            append( want, from, to );
        }
        CHECK( got[i] == want );
    }
}

void
checkStarts( const Map& map, uint64_t fileBytes, const File& file, const std::vector<uint64_t>& lines,
             size_t cap, bool packed )
{
    std::vector<uint64_t> indexBytes, indexLines;
    indexOf( map, file, indexBytes, indexLines );
    const auto blocks = blocksOf( map );
    const auto plan = planLines( map, indexBytes.data(), indexLines.data(), indexBytes.size(), lines.data(), nullptr,
                                 lines.size(), true, cap, packed, fileBytes );
    std::vector<uint64_t> s( 1, 0 );
    for ( uint64_t x = file.front; x < file.size(); ++x ) {
        if ( file[x] == NL ) s.push_back( x + 1 );
    }
    const uint64_t N = s.size() - 1;
    std::set<uint64_t> needed;
    for ( const auto k : lines ) {
        if ( k >= 1 && k <= N ) needed.insert( blocks.bits[blockHolding( blocks, s[k] - 1 )] );
    }
    const auto run = execute( plan, map, file, cap, packed );
    CHECK( std::vector<uint64_t>( needed.begin(), needed.end() ) == run.launched );
    CHECK( plan.segments.empty() && plan.starts.size() == lines.size() );
    for ( size_t i = 0; i < lines.size(); ++i ) {
        const auto& start = plan.starts[i];
        const uint64_t want = lines[i] > N ? file.size() : s[lines[i]];
        if ( start.query == NO_QUERY ) {
            CHECK( lines[i] == 0 || lines[i] > N );
            CHECK( start.fixed == want );
        } else {
            CHECK( start.query < plan.queries.size() && run.positions[start.query] != NOT_FOUND );
            if ( start.query < plan.queries.size() && run.positions[start.query] != NOT_FOUND ) {
                CHECK( lineStartOf( plan.queries[start.query], run.positions[start.query] ) == want );
            }
        }
    }
}

void
runCases( const char* name, const Map& map, uint64_t fileBytes, const File& file, std::mt19937_64& rng )
{
    currentCase = name;
    uint64_t N = 0;
    for ( const auto byte : file.tail ) N += byte == NL;
    std::vector<uint64_t> first, count;
    const auto add = [&] ( uint64_t f, uint64_t c ) { first.push_back( f ); count.push_back( c ); };
    const uint64_t HUGE_COUNT = ~uint64_t( 0 );
    add( 0, 0 );
    add( 0, 1 );
    add( 0, N );
    add( 0, N + 1 );
    add( 0, HUGE_COUNT );
    add( N, 1 );                 /* the unterminated tail */
    add( N, 0 );
    add( N, HUGE_COUNT );
    add( N + 1, 1 );             /* beyond the last line */
    add( N + 7, HUGE_COUNT );
    add( HUGE_COUNT, HUGE_COUNT );
    if ( N > 0 ) {
        add( N - 1, 1 );
        add( N - 1, 2 );
        add( N - 1, 3 );
        add( 1, HUGE_COUNT );       /* first + count wraps */
    }
    for ( uint64_t k = 0; k <= N && k < 40; ++k ) add( k, 1 );     /* every line of a small file on its own */
    for ( int k = 0; k < 40; ++k ) {
        const uint64_t f = rng() % ( N + 3 );
        const uint64_t c = k % 5 == 0 ? 0 : ( k % 5 == 1 ? 1 : rng() % ( N + 2 ) );
        add( f, c );
        if ( k % 7 == 0 ) add( f, c );    /* duplicates: one query serves both */
    }
    for ( const size_t cap : { 1, 2, 3, 512 } ) {
        for ( const bool packed : { false, true } ) {
            checkRanges( map, fileBytes, file, first, count, cap, packed );
            checkStarts( map, fileBytes, file, first, cap, packed );
        }
    }
    /* one range alone: nothing but its own blocks is launched */
    for ( size_t i = 0; i < first.size(); i += 3 ) {
        checkRanges( map, fileBytes, file, { first[i] }, { count[i] }, 2, false );
    }
}

std::vector<uint8_t>
fileWith( uint64_t size, const std::vector<uint64_t>& delimiters )
{
    std::vector<uint8_t> file( size );
    for ( uint64_t x = 0; x < size; ++x ) file[x] = (uint8_t)( 'a' + ( x * 2654435761u >> 7 ) % 26 );
    for ( const auto x : delimiters ) file[x] = NL;
    return file;
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0x11E5 );
    uint64_t fileBytes = 0;

    /* two streams, 3 + 2 blocks of 100, 250, 50 | 300, 1 bytes: blocks [0,100) [100,350) [350,400) | [400,700) [700,701).
     * Delimiters: 99 is block 0's LAST byte (line 1 starts with block 1's first byte); none in block 1 and 2 (the line
     * from 100 spans blocks 1, 2 and reaches into the second stream: with cap 2 it crosses a launch boundary); 400 is a
     * block's FIRST byte; 699 again a last byte; the 1-byte block 700 is no delimiter: an unterminated tail. */
    {
        const auto map = makeMap( { { 100, 250, 50 }, { 300, 1 } }, rng, &fileBytes );
        runCases( "two streams", map, fileBytes, fileWith( 701, { 10, 11, 99, 400, 450, 699 } ), rng );
        /* the same file ending with a delimiter: the last line is empty */
        runCases( "ends with a delimiter", map, fileBytes, fileWith( 701, { 10, 99, 400, 700 } ), rng );
        /* no delimiter at all: one line */
        runCases( "no delimiter", map, fileBytes, fileWith( 701, {} ), rng );
        /* only the very first byte */
        runCases( "first byte", map, fileBytes, fileWith( 701, { 0 } ), rng );
        /* every byte a delimiter */
        runCases( "delimiters only", map, fileBytes, std::vector<uint8_t>( 701, NL ), rng );
    }
    /* the same behind a front block of 2^32 - k bytes without a delimiter (k: inside block 0, its last byte, block 1's first
     * byte, inside the long line, in the second stream), the bit offsets of what follows from just below 2^32 on */
    {
        const uint64_t cut = uint64_t( 1 ) << 32;
        for ( const uint64_t k : { 1, 50, 99, 100, 101, 300, 400, 450, 700 } ) {
            const uint64_t front = cut - k;
            const auto map = makeMap( { { 100, 250, 50 }, { 300, 1 } }, rng, &fileBytes, front, cut - 8 * ( 5 + k % 7 ) );
            currentCase = "high: the layout";
            CHECK( map[2].second == front && map.back().second == front + 701 && map.back().first > cut );
            runCases( "high, two streams", map, fileBytes, File( fileWith( 701, { 10, 11, 99, 400, 450, 699 } ), front ), rng );
            if ( k % 100 != 0 ) continue;
            runCases( "high, ends with a delimiter", map, fileBytes, File( fileWith( 701, { 10, 99, 400, 700 } ), front ), rng );
            runCases( "high, no delimiter", map, fileBytes, File( fileWith( 701, {} ), front ), rng );
            runCases( "high, delimiters only", map, fileBytes, File( std::vector<uint8_t>( 701, NL ), front ), rng );
        }
    }
    /* a single one-byte block: a delimiter, and not */
    {
        const auto map = makeMap( { { 1 } }, rng, &fileBytes );
        runCases( "one byte", map, fileBytes, fileWith( 1, {} ), rng );
        runCases( "one delimiter", map, fileBytes, fileWith( 1, { 0 } ), rng );
    }
    /* an empty file: the index is {0: 0}, every range is empty, nothing is launched */
    {
        const Map map = { { 32, 0 }, { 112, 0 } };
        runCases( "empty file", map, 14, File{}, rng );
        currentCase = "empty file";
        std::vector<uint64_t> indexBytes, indexLines;
        indexOf( map, File{}, indexBytes, indexLines );
        CHECK( indexBytes == std::vector<uint64_t>{ 0 } && indexLines == std::vector<uint64_t>{ 0 } );
        const uint64_t first[2] = { 0, 5 }, count[2] = { 10, 1 };
        const auto plan = planLines( map, indexBytes.data(), indexLines.data(), 1, first, count, 2, false, 4, false, 14 );
        CHECK( plan.launches.empty() && plan.queries.empty() && plan.segments.empty() );
    }
    /* seeded: one to four streams of up to 30 blocks of 1..300 bytes, delimiters every ~40 bytes with gaps of several
     * blocks without any, and delimiters forced onto last and first bytes of blocks */
    for ( int m = 0; m < 16; ++m ) {
        std::vector<std::vector<uint64_t> > streams( 1 + rng() % 4 );
        uint64_t total = 0;
        for ( auto& stream : streams ) {
            stream.resize( 1 + rng() % 30 );
            for ( auto& size : stream ) {
                size = 1 + rng() % 300;
                total += size;
            }
        }
        const auto map = makeMap( streams, rng, &fileBytes );
        std::vector<uint64_t> delimiters;
        const uint64_t gapFrom = rng() % total, gapTo = gapFrom + total / 3;
        for ( uint64_t x = rng() % 40; x < total; x += 1 + rng() % 80 ) {
            if ( x < gapFrom || x >= gapTo ) delimiters.push_back( x );
        }
        const auto blocks = blocksOf( map );
        for ( size_t b = 0; b < blocks.starts.size(); b += 1 + rng() % 4 ) {
            delimiters.push_back( rng() % 2 ? blocks.starts[b] : blocks.starts[b] + blocks.lengths[b] - 1 );
        }
        if ( m % 4 == 0 ) delimiters.push_back( total - 1 );
        runCases( "seeded", map, fileBytes, fileWith( total, delimiters ), rng );
        if ( m % 4 == 1 ) {
            /* the same blocks and delimiters behind a front block that ends a seeded number of bytes below 2^32 */
            const uint64_t front = ( uint64_t( 1 ) << 32 ) - 1 - rng() % total;
            const auto high = makeMap( streams, rng, &fileBytes, front, ( uint64_t( 1 ) << 32 ) - 8 * ( 5 + rng() % 50 ) );
            runCases( "high, seeded", high, fileBytes, File( fileWith( total, delimiters ), front ), rng );
        }
    }

    /* an imported index is checked against the map */
    currentCase = "index checks";
    {
        const auto map = makeMap( { { 100, 250, 50 }, { 300, 1 } }, rng, &fileBytes );
        const std::vector<uint64_t> bytes = { 0, 100, 350, 400, 700, 701 }, lines = { 0, 3, 3, 3, 6, 6 };
        const auto refused = [&] ( std::vector<uint64_t> b, std::vector<uint64_t> l ) {
            try {
                checkLineIndex( map, b.data(), l.data(), b.size() );
            } catch ( const std::invalid_argument& ) {
                return true;
            }
            return false;
        };
        CHECK( !refused( bytes, lines ) );
        CHECK( refused( { 0, 100, 350, 400, 700 }, { 0, 3, 3, 3, 6 } ) );                 /* the end is missing */
        CHECK( refused( { 0, 100, 351, 400, 700, 701 }, lines ) );                        /* not a block start */
        CHECK( refused( { 0, 100, 350, 400, 700, 702 }, lines ) );                        /* not the size */
        CHECK( refused( bytes, { 1, 3, 3, 3, 6, 6 } ) );                                  /* does not start at 0 */
        CHECK( refused( bytes, { 0, 3, 2, 3, 6, 6 } ) );                                  /* decreases */
        CHECK( refused( bytes, { 0, 3, 3, 3, 6, 8 } ) );                                  /* 2 delimiters in a 1-byte block */
        CHECK( refused( bytes, { 0, 101, 101, 101, 101, 101 } ) );                        /* 101 in 100 bytes */
        CHECK( !refused( bytes, { 0, 100, 100, 100, 100, 101 } ) );

        /* an index that lies (one count raised by 1): the query for the promised delimiter finds none, and a segment
         * that needs it does not resolve */
        const auto file = fileWith( 701, { 10, 11, 99, 400, 450, 699 } );
        std::vector<uint64_t> lying = lines;
        for ( size_t i = 1; i < lying.size(); ++i ) lying[i] += 1;    /* block 0 is given 4 */
        const uint64_t first[1] = { 4 }, count[1] = { 1 };
        const auto plan = planLines( map, bytes.data(), lying.data(), bytes.size(), first, count, 1, false, 4, false, fileBytes );
        const auto run = execute( plan, map, file, 4, false );
        CHECK( !plan.queries.empty() && run.positions[plan.segments.front().startQuery] == NOT_FOUND );
        uint64_t src = 0, size = 0;
        CHECK( !resolveSegment( plan, plan.segments.front(), run.positions.data(), &src, &size ) );
    }

    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "lines ok\n" );
    return 0;
}
