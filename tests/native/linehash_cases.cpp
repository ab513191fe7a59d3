/**
 * linehash_cases.cpp -- indexed_bzip2_amd/csrc/bz2_linehash.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: the known answers, mulmod against 128-bit arithmetic, the composition's
 * associativity, summarise against the direct definition and independent of the chunk size, stitchSummaries over random
 * cuts, its refusals, spans beyond 2^32 (synthetic summaries, no bytes) and the plan of a range of lines.
 */
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
    std::puts( "linehash cases ok" );
    return 0;
}
