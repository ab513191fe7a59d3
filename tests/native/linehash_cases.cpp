/**
 * linehash_cases.cpp -- indexed_bzip2_amd/csrc/bz2_linehash.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: the known answers, mulmod against 128-bit arithmetic, the composition's
 * associativity, summarise against the direct definition and independent of the chunk size, stitchSummaries over random
 * cuts, its refusals, spans beyond 2^32 (synthetic summaries, no bytes), the plan of a range of lines and the places of
 * its stretches in a column (placeLineColumn) against a direct count of the delimiters.
 */
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_linehash.hpp"

using namespace bz2gpu;

#define CHECK( condition )                                                           \
    do {                                                                             \
        if ( !( condition ) ) {                                                      \
            std::fprintf( stderr, "%s:%d: %s\n", __FILE__, __LINE__, #condition );   \
            std::exit( 1 );                                                          \
        }                                                                            \
    } while ( 0 )

namespace
{
using Bytes = std::vector<uint8_t>;

Bytes
bytesOf( const std::string& s )
{
    return Bytes( s.begin(), s.end() );
}

/** The hashes of the lines of `data` by the definition: a non-empty unterminated tail is one more line. */
std::vector<uint64_t>
direct( const Bytes& data, uint8_t nl, uint64_t seed )
{
    std::vector<uint64_t> hashes;
    size_t from = 0;
    for ( size_t at = 0; at < data.size(); ++at ) {
        if ( data[at] != nl ) continue;
        hashes.push_back( lineHash( data.data() + from, at - from, seed ) );
        from = at + 1;
    }
    if ( from < data.size() ) hashes.push_back( lineHash( data.data() + from, data.size() - from, seed ) );
    return hashes;
}

Bytes
randomBytes( std::mt19937_64& rng, size_t size )
{
    static const uint8_t alphabet[] = { 'a', 'b', '\n', 0, 0xFF };
    Bytes data( size );
    for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
    return data;
}

void
knownAnswers()
{
    CHECK( lineHashBase( 0 ) == 0x0220A8397B1DD5B6ull );
    CHECK( lineHashBase( 1 ) == 0x110A2DEC890261C5ull );
    CHECK( lineHash( nullptr, 0, 0 ) == 0 );
    const auto hash = [] ( const std::string& s ) { return lineHash( reinterpret_cast<const uint8_t*>( s.data() ), s.size(), 0 ); };
    CHECK( hash( "a" ) == 98 );
    CHECK( hash( std::string( 2, '\0' ) ) == 153307352162751927ull );
    CHECK( hash( "hello" ) == 951416200074518375ull );
    CHECK( hash( std::string( 1, '\0' ) ) != hash( std::string( 2, '\0' ) ) );
}

void
arithmetic( std::mt19937_64& rng )
{
    const uint64_t edge[] = { 0, 1, 2, 255, 256, LINEHASH_P - 1, LINEHASH_P - 2, uint64_t( 1 ) << 60, ( uint64_t( 1 ) << 60 ) + 1 };
    std::vector<uint64_t> values( edge, edge + sizeof( edge ) / sizeof( edge[0] ) );
    for ( int i = 0; i < 200; ++i ) values.push_back( rng() % LINEHASH_P );
    for ( const auto a : values ) {
        for ( const auto b : values ) {
            CHECK( mulmod( a, b ) == (uint64_t)( (unsigned __int128)a * b % LINEHASH_P ) );
            CHECK( addmod( a, b ) == ( a + b ) % LINEHASH_P );
        }
    }
    /* ( a ; b ) ; c == a ; ( b ; c ), and ( 0, 1 ) is neutral */
    for ( int i = 0; i < 2000; ++i ) {
        const HashPart a{ rng() % LINEHASH_P, rng() % LINEHASH_P }, b{ rng() % LINEHASH_P, rng() % LINEHASH_P },
            c{ rng() % LINEHASH_P, rng() % LINEHASH_P };
        CHECK( followedBy( followedBy( a, b ), c ) == followedBy( a, followedBy( b, c ) ) );
        CHECK( followedBy( a, HashPart{} ) == a && followedBy( HashPart{}, a ) == a );
    }
}

void
summaries( std::mt19937_64& rng )
{
    for ( int round = 0; round < 400; ++round ) {
        const auto data = randomBytes( rng, rng() % 200 );
        const uint64_t seed = rng();
        const uint64_t x = lineHashBase( seed );
        const uint8_t nl = round % 3 == 0 ? 0 : '\n';
        const auto want = direct( data, nl, seed );
        const auto whole = summarise( x, data.data(), data.size(), nl, data.size() + 1 );
        for ( const size_t chunk : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 7 ), size_t( 16 ), size_t( 64 ), size_t( 256 ) } ) {
            const auto s = summarise( x, data.data(), data.size(), nl, chunk );
            CHECK( s.head == whole.head && s.tail == whole.tail && s.hasDelimiter == whole.hasDelimiter );
            CHECK( s.tailNonEmpty == whole.tailNonEmpty && s.count == whole.count && s.hashes == whole.hashes );
        }
        /* one stretch from offset 0 is the file */
        std::vector<HashStretch> one( 1 );
        one[0].size = data.size();
        one[0].summary = whole;
        CHECK( stitchedHashes( one ) == want );
        /* random cuts, each stretch summarised with a chunk size of its own */
        std::vector<size_t> cuts{ 0, data.size() };
        for ( uint64_t k = rng() % 7; k > 0; --k ) cuts.push_back( rng() % ( data.size() + 1 ) );
        std::sort( cuts.begin(), cuts.end() );
        std::vector<HashStretch> stretches;
        for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
            HashStretch stretch;
            stretch.fileOffset = cuts[k];
            stretch.size = cuts[k + 1] - cuts[k];
            stretch.summary = summarise( x, data.data() + cuts[k], stretch.size, nl, 1 + rng() % 64 );
            stretches.push_back( std::move( stretch ) );
        }
        CHECK( stitchedHashes( stretches ) == want );
    }
    try {
        (void)summarise( 256, nullptr, 0, '\n', 0 );
        CHECK( false );
    } catch ( const std::invalid_argument& ) {}
}

template<typename Call>
bool
refused( const Call& call )
{
    try {
        call();
    } catch ( const std::invalid_argument& ) {
        return true;
    }
    return false;
}

void
refusals()
{
    const auto nothing = [] ( uint64_t, uint64_t ) {};
    const Bytes text = bytesOf( "ab\ncd" );
    std::vector<HashStretch> stretches( 2 );
    stretches[0].size = 3;
    stretches[0].summary = summarise( 256, text.data(), 3, '\n', 2 );
    stretches[1].fileOffset = 3;
    stretches[1].size = 2;
    stretches[1].summary = summarise( 256, text.data() + 3, 2, '\n', 2 );
    CHECK( !refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
    stretches[1].fileOffset = 4;    /* a gap */
    CHECK( refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
    stretches[1].fileOffset = 2;    /* an overlap */
    CHECK( refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
    stretches[1].fileOffset = 3;
    std::swap( stretches[0], stretches[1] );    /* the wrong order */
    CHECK( refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
    std::swap( stretches[0], stretches[1] );
    stretches[0].summary.hashes.clear();        /* a count without its hashes cannot be listed */
    CHECK( refused( [&] { (void)stitchedHashes( stretches ); } ) );
    stretches[0].summary.count = 0;             /* a delimiter that closes no line */
    CHECK( refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
    stretches[0].fileOffset = ~uint64_t( 0 ) - 1;   /* the end does not fit 64 bits */
    CHECK( refused( [&] { (void)stitchSummaries( stretches, nothing ); } ) );
}

/** Stretches of 3 GiB that each close 5 * 2^30 lines: nothing is listed, only the seams are patched. */
void
beyondFourGiB()
{
    const uint64_t x = lineHashBase( 7 );
    const uint64_t size = uint64_t( 3 ) << 30, lines = uint64_t( 5 ) << 30;
    const Bytes headBytes = bytesOf( "tail of the last" ), tailBytes = bytesOf( "head of the next" );
    std::vector<HashStretch> stretches( 4 );
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        auto& stretch = stretches[i];
        stretch.fileOffset = i * size;
        stretch.size = size;
        stretch.summary.hasDelimiter = i != 2;      /* stretch 2 is one piece of a line */
        stretch.summary.head = hashPart( x, headBytes.data(), headBytes.size() );
        if ( i == 2 ) continue;
        stretch.summary.tail = hashPart( x, tailBytes.data(), tailBytes.size() );
        stretch.summary.tailNonEmpty = true;
        stretch.summary.count = lines;
    }
    std::vector<std::pair<uint64_t, uint64_t> > patches;
    const auto stitched = stitchSummaries( stretches, [&] ( uint64_t k, uint64_t hash ) { patches.emplace_back( k, hash ); } );
    CHECK( stitched.closed == 3 * lines && stitched.closed > ( uint64_t( 1 ) << 33 ) );
    CHECK( stitched.hasTail && stitched.tailHash == stretches[3].summary.tail.h );
    /* stretch 0 is entered empty: no patch; stretch 1's first line is closed line 5 * 2^30; stretch 3's is 10 * 2^30 and
     * holds the tail of 1, all of 2 and its own head */
    CHECK( patches.size() == 2 );
    Bytes joined = tailBytes;
    joined.insert( joined.end(), headBytes.begin(), headBytes.end() );
    CHECK( patches[0] == std::make_pair( lines, hashPart( x, joined.data(), joined.size() ).h ) );
    joined = tailBytes;
    joined.insert( joined.end(), headBytes.begin(), headBytes.end() );
    joined.insert( joined.end(), headBytes.begin(), headBytes.end() );
    CHECK( patches[1] == std::make_pair( 2 * lines, hashPart( x, joined.data(), joined.size() ).h ) );
}

/** Four blocks of 100 bytes with 3, 0, 2 and 1 delimiters; the file ends in an unterminated tail or not, nobody knows. */
void
plans()
{
    const std::vector<std::pair<uint64_t, uint64_t> > map{ { 32, 0 }, { 1000, 100 }, { 2000, 200 }, { 3000, 300 }, { 4000, 400 } };
    const uint64_t lineBytes[] = { 0, 100, 200, 300, 400 }, lineLines[] = { 0, 3, 3, 5, 6 };
    const auto plan = [&] ( uint64_t first, uint64_t count ) {
        return planLineHashes( map, lineBytes, lineLines, 5, first, count, 64, false, 4100 );
    };
    const auto covered = [] ( const LineHashPlan& p ) {
        uint64_t begin = p.stretches.empty() ? 0 : p.stretches.front().fileOffset, end = begin;
        for ( const auto& piece : p.stretches ) {
            CHECK( piece.fileOffset == end );
            end += piece.size;
        }
        return std::make_pair( begin, end );
    };
    auto p = plan( 0, ~uint64_t( 0 ) );
    CHECK( p.count == 7 && p.reachesEnd && p.firstClosed == 0 && p.N == 6 && covered( p ) == std::make_pair( uint64_t( 0 ), uint64_t( 400 ) ) );
    p = plan( 1, 1 );      /* inside block 0 */
    CHECK( p.count == 1 && !p.reachesEnd && p.firstClosed == 0 && covered( p ) == std::make_pair( uint64_t( 0 ), uint64_t( 100 ) ) );
    p = plan( 3, 1 );      /* line 3 starts behind block 0's last delimiter and is closed in block 2 */
    CHECK( p.count == 1 && p.firstClosed == 0 && covered( p ) == std::make_pair( uint64_t( 0 ), uint64_t( 300 ) ) );
    p = plan( 4, 2 );      /* lines 4 and 5: from block 2, which closes line 3, through block 3 */
    CHECK( p.count == 2 && !p.reachesEnd && p.firstClosed == 3 && covered( p ) == std::make_pair( uint64_t( 200 ), uint64_t( 400 ) ) );
    p = plan( 5, 100 );    /* clipped: line 5 and the tail */
    CHECK( p.count == 2 && p.reachesEnd && p.firstClosed == 3 && covered( p ) == std::make_pair( uint64_t( 200 ), uint64_t( 400 ) ) );
    p = plan( 6, 1 );      /* the tail alone: from the block with the last delimiter */
    CHECK( p.count == 1 && p.reachesEnd && p.firstClosed == 5 && covered( p ) == std::make_pair( uint64_t( 300 ), uint64_t( 400 ) ) );
    p = plan( 7, 1 );      /* beyond the last line, and nothing asked for */
    CHECK( p.count == 0 && p.launches.empty() && p.stretches.empty() );
    p = plan( 2, 0 );
    CHECK( p.count == 0 && p.launches.empty() && p.stretches.empty() );
    /* every block once */
    p = plan( 0, ~uint64_t( 0 ) );
    size_t blocks = 0;
    for ( const auto& launch : p.launches ) blocks += launch.bits.size();
    CHECK( blocks == 4 );
}

/** placeLineColumn against a direct count of the delimiters in the bytes: a text in blocks of 150 to 400 bytes, a long line
 * through three of them, with and without an unterminated tail, planned with caps that give one to many launches. */
void
places( std::mt19937_64& rng )
{
    const uint8_t nl = '\n';
    for ( const bool tail : { true, false } ) {
        Bytes text;
        std::vector<uint64_t> lineBytes{ 0 }, lineLines{ 0 };
        std::vector<std::pair<uint64_t, uint64_t> > map{ { 32, 0 } };
        for ( size_t block = 0; block < 12; ++block ) {
            const size_t size = 150 + rng() % 251;
            for ( size_t i = 0; i < size; ++i ) {
                const bool inLongLine = block >= 4 && block <= 6;       /* blocks 4 to 6 close no line */
                text.push_back( !inLongLine && rng() % 40 == 0 ? nl : uint8_t( 'a' + rng() % 3 ) );
            }
            if ( block == 11 ) text.back() = tail ? 'x' : nl;
            lineBytes.push_back( text.size() );
            lineLines.push_back( (uint64_t)std::count( text.begin(), text.end(), nl ) );
            map.emplace_back( 32 + 1000 * ( block + 1 ), text.size() );
        }
        const uint64_t N = lineLines.back();
        const auto delimitersIn = [&] ( uint64_t from, uint64_t to ) {
            return (uint64_t)std::count( text.begin() + (ptrdiff_t)from, text.begin() + (ptrdiff_t)to, nl );
        };
        CHECK( N > 20 && delimitersIn( lineBytes[4], lineBytes[7] ) == 0 );
        /* the line that runs through blocks 4 to 6, and a block that closes at least three lines */
        const uint64_t longLine = lineLines[4];
        size_t busy = 0;
        while ( lineLines[busy + 1] - lineLines[busy] < 3 ) ++busy;
        const std::vector<std::pair<uint64_t, uint64_t> > ranges{
            { 0, ~uint64_t( 0 ) }, { 0, N }, { 0, N + 1 }, { 0, 1 }, { lineLines[busy] + 1, 1 }, { lineLines[busy] + 1, 2 },
            { longLine, 1 }, { longLine + 1, 3 }, { longLine - 1, 4 }, { lineLines[8] + 1, 5 }, { 3, N - 5 }, { N - 2, 2 },
            { N - 2, 3 }, { N - 2, 1000 }, { N - 1, ~uint64_t( 0 ) }, { N, 1 }, { N, 0 }, { N + 1, 1 }, { N + 7, ~uint64_t( 0 ) }, { 5, 0 } };
        bool sawInsideOneStretch = false, sawEarlierBlock = false, sawNoLine = false, sawLaunches = false, sawTail = false;
        for ( const size_t cap : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 5 ), size_t( 64 ) } ) {
            for ( const auto& [first, count] : ranges ) {
                const auto plan = planLineHashes( map, lineBytes.data(), lineLines.data(), lineBytes.size(), first, count, cap, false,
                                                  ( 32 + 1000 * 12 ) / 8 + 100 );
                const auto placed = placeLineColumn( plan, lineBytes.data(), lineLines.data(), lineBytes.size() );
                /* count clipped at N + 1 - first, nothing for first > N; the tail is wanted where the range goes past line N - 1 */
                CHECK( plan.N == N && plan.first == first );
                CHECK( plan.count == ( first > N ? 0 : std::min( count, N + 1 - first ) ) );
                CHECK( plan.reachesEnd == ( plan.count > 0 && plan.count > N - first ) );
                const uint64_t wanted = plan.count - ( plan.reachesEnd ? 1 : 0 );
                CHECK( plan.wantedClosed() == wanted );
                CHECK( placed.size() == plan.stretches.size() && ( plan.count > 0 ) == !placed.empty() );
                if ( placed.empty() ) continue;
                CHECK( plan.firstClosed == delimitersIn( 0, plan.stretches.front().fileOffset ) && plan.firstClosed <= first );
                uint64_t closedBefore = plan.firstClosed, next = 0, taking = 0;
                for ( size_t k = 0; k < placed.size(); ++k ) {
                    const auto& piece = plan.stretches[k];
                    const uint64_t closed = delimitersIn( piece.fileOffset, piece.fileOffset + piece.size );
                    CHECK( placed[k].closed == closed );
                    /* from the delimiters themselves: the one at text[p] closes line number( p ) = the delimiters in front
                     * of it; of those inside the stretch, the wanted ones are lines [first, first + wanted) */
                    uint64_t skip = 0, take = 0, at = 0;
                    for ( uint64_t p = piece.fileOffset; p < piece.fileOffset + piece.size; ++p ) {
                        if ( text[p] != nl ) continue;
                        const uint64_t line = delimitersIn( 0, p );
                        if ( line < first ) ++skip;
                        if ( line >= first && line - first < wanted && take++ == 0 ) at = line - first;
                    }
                    if ( take > 0 ) {
                        CHECK( placed[k].skip == skip && placed[k].take == take && placed[k].at == at );
                        CHECK( placed[k].at == next );         /* the places tile the column without gap or overlap */
                        next += placed[k].take;
                        ++taking;
                        if ( placed[k].skip > 0 && placed[k].skip + placed[k].take < closed && placed[k].take == wanted ) sawInsideOneStretch = true;
                    } else {
                        CHECK( placed[k].take == 0 );
                    }
                    if ( closed == 0 ) sawNoLine = true;
                    closedBefore += closed;
                }
                CHECK( next == wanted );
                /* the last stretch reaches the delimiter that closes the last wanted line, or the end of the file */
                CHECK( closedBefore >= first + wanted );
                if ( plan.reachesEnd ) CHECK( plan.stretches.back().fileOffset + plan.stretches.back().size == text.size() );
                if ( first > plan.firstClosed && first == longLine + 1 ) sawEarlierBlock = true;
                if ( plan.launches.size() > 2 && taking > 2 ) sawLaunches = true;
                if ( plan.reachesEnd && wanted > 0 ) sawTail = true;
            }
        }
        CHECK( sawInsideOneStretch && sawEarlierBlock && sawNoLine && sawLaunches && sawTail );
    }
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0x11E5 );
    knownAnswers();
    arithmetic( rng );
    summaries( rng );
    refusals();
    beyondFourGiB();
    plans();
    places( rng );
    std::puts( "linehash cases ok" );
    return 0;
}
