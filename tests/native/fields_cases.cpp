/**
 * fields_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fields.hpp on the CPU, as a program of its own that the test suite builds
 * with -fsanitize=address,undefined: known answers, summariseFields against a naive split and independent of the chunk
 * size, stitchFields over random cuts, the saturation of the delimiter count, a line through several stretches with its
 * field's start in one and its end in another, its refusals, stretches beyond 2^32 (synthetic summaries, no bytes) and
 * the plan of a range of lines.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fields.hpp"

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

/** Field j of one content that starts at offset s, by splitting it naively into its parts first. */
FieldSpan
naiveField( const Bytes& data, size_t s, size_t end, uint8_t dl, uint32_t j )
{
    std::vector<std::pair<size_t, size_t> > parts;   /* begin, size */
    size_t from = s;
    for ( size_t at = s; at < end; ++at ) {
        if ( data[at] != dl ) continue;
        parts.emplace_back( from, at - from );
        from = at + 1;
    }
    parts.emplace_back( from, end - from );
    if ( j >= parts.size() ) return { end, -1 };
    return { parts[j].first, (int64_t)parts[j].second };
}

/** Field j of every line of `data` by the definition: a non-empty unterminated tail is one more line. */
std::vector<FieldSpan>
direct( const Bytes& data, uint8_t nl, uint8_t dl, uint32_t j )
{
    std::vector<FieldSpan> fields;
    size_t from = 0;
    for ( size_t at = 0; at < data.size(); ++at ) {
        if ( data[at] != nl ) continue;
        fields.push_back( naiveField( data, from, at, dl, j ) );
        from = at + 1;
    }
    if ( from < data.size() ) fields.push_back( naiveField( data, from, data.size(), dl, j ) );
    return fields;
}

Bytes
randomBytes( std::mt19937_64& rng, size_t size, uint8_t nl, uint8_t dl )
{
    const uint8_t alphabet[] = { 'a', dl, nl, 0, 0xFF, dl, 'b' };
    Bytes data( size );
    for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
    return data;
}

bool
same( const FieldSummary& a, const FieldSummary& b )
{
    return a.size == b.size && a.hasDelimiter == b.hasDelimiter && a.tailNonEmpty == b.tailNonEmpty && a.count == b.count
           && a.firstNl == b.firstNl && a.headPositions == b.headPositions && a.tailStart == b.tailStart
           && a.tailDelims == b.tailDelims && a.tailFieldStart == b.tailFieldStart && a.tailFieldEnd == b.tailFieldEnd
           && a.starts == b.starts && a.sizes == b.sizes;
}

void
knownAnswers()
{
    const Bytes text = bytesOf( "a\tbc\t\n\nx\n\t\ty" );
    /* lines: "a\tbc\t" at 0, "" at 6, "x" at 7, "\t\ty" at 9 */
    const auto fields = [&] ( uint32_t j ) { return direct( text, '\n', '\t', j ); };
    CHECK( ( fields( 0 ) == std::vector<FieldSpan>{ { 0, 1 }, { 6, 0 }, { 7, 1 }, { 9, 0 } } ) );
    CHECK( ( fields( 1 ) == std::vector<FieldSpan>{ { 2, 2 }, { 6, -1 }, { 8, -1 }, { 10, 0 } } ) );
    CHECK( ( fields( 2 ) == std::vector<FieldSpan>{ { 5, 0 }, { 6, -1 }, { 8, -1 }, { 11, 1 } } ) );
    CHECK( ( fields( 3 ) == std::vector<FieldSpan>{ { 5, -1 }, { 6, -1 }, { 8, -1 }, { 12, -1 } } ) );
    for ( uint32_t j = 0; j < 5; ++j ) {
        std::vector<FieldStretch> one( 1 );
        one[0].summary = summariseFields( text.data(), text.size(), '\n', '\t', j, 3 );
        CHECK( stitchedFields( one, j ) == fields( j ) );
    }
    CHECK( fieldArgumentsError( '\n', '\t', 1023 ).empty() && !fieldArgumentsError( '\n', '\t', 1024 ).empty() );
    CHECK( !fieldArgumentsError( 9, 9, 0 ).empty() );
}

void
summaries( std::mt19937_64& rng )
{
    const uint32_t fieldsTried[] = { 0, 1, 2, 5, 1023 };
    const uint8_t delimiters[] = { '\t', ',', 0xFF, 1 };
    for ( int round = 0; round < 600; ++round ) {
        const uint8_t nl = round % 3 == 0 ? 0 : '\n', dl = delimiters[round % 4];
        const uint32_t j = fieldsTried[round % 5];
        const auto data = randomBytes( rng, rng() % 200, nl, dl );
        const auto want = direct( data, nl, dl, j );
        const auto whole = summariseFieldChunk( data.data(), data.size(), nl, dl, j );
        for ( const size_t chunk : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 7 ), size_t( 16 ), size_t( 64 ), size_t( 256 ) } ) {
            CHECK( same( summariseFields( data.data(), data.size(), nl, dl, j, chunk ), whole ) );
        }
        CHECK( whole.headDelims() <= j + 1 && whole.tailDelims <= j + 1 );
        /* one stretch from offset 0 is the file */
        std::vector<FieldStretch> one( 1 );
        one[0].summary = whole;
        CHECK( stitchedFields( one, j ) == want );
        /* random cuts, each stretch summarised with a chunk size of its own */
        std::vector<size_t> cuts{ 0, data.size() };
        for ( uint64_t k = rng() % 7; k > 0; --k ) cuts.push_back( rng() % ( data.size() + 1 ) );
        std::sort( cuts.begin(), cuts.end() );
        std::vector<FieldStretch> stretches;
        for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
            FieldStretch stretch;
            stretch.fileOffset = cuts[k];
            stretch.summary = summariseFields( data.data() + cuts[k], cuts[k + 1] - cuts[k], nl, dl, j, 1 + rng() % 64 );
            stretches.push_back( std::move( stretch ) );
        }
        CHECK( stitchedFields( stretches, j ) == want );
    }
    try {
        (void)summariseFields( nullptr, 0, '\n', '\t', 0, 0 );
        CHECK( false );
    } catch ( const std::invalid_argument& ) {}
}

/** A count that saturates: 5000 delimiters in one line and a field in front of, at and behind the cap. */
void
saturation()
{
    Bytes line;
    for ( int i = 0; i < 5000; ++i ) {
        line.push_back( 'a' + i % 3 );
        line.push_back( ',' );
    }
    line.push_back( '\n' );
    for ( const uint32_t j : { 0u, 1u, 255u, 256u, 1023u } ) {
        for ( const size_t chunk : { size_t( 1 ), size_t( 5 ), size_t( 256 ), size_t( 4096 ) } ) {
            const auto s = summariseFields( line.data(), line.size(), '\n', ',', j, chunk );
            CHECK( s.headDelims() == j + 1 && s.count == 1 && s.tailDelims == 0 );
            CHECK( s.starts[0] == 2 * j && s.sizes[0] == 1 );
        }
    }
    /* the same line without its nl: the tail saturates, and both ends of the field are known */
    line.pop_back();
    const auto open = summariseFields( line.data(), line.size(), '\n', ',', 7, 33 );
    CHECK( !open.hasDelimiter && open.tailDelims == 8 && open.tailFieldStart == 14 && open.tailFieldEnd == 15 && open.tailNonEmpty );
}

/** One line through five stretches: field 2 starts in the second and ends in the fourth. */
void
longLine()
{
    const std::vector<std::string> pieces{ "x\nab,c", "d,efg", "hij", "kl,m", "no\nq,r" };
    Bytes text;
    std::vector<FieldStretch> stretches;
    for ( const auto& piece : pieces ) {
        FieldStretch stretch;
        stretch.fileOffset = text.size();
        const auto bytes = bytesOf( piece );
        stretch.summary = summariseFields( bytes.data(), bytes.size(), '\n', ',', 2, 2 );
        stretches.push_back( std::move( stretch ) );
        text.insert( text.end(), bytes.begin(), bytes.end() );
    }
    /* "ab,cd,efghijkl,mno": field 2 is "efghijkl" at 8 */
    std::vector<std::pair<uint64_t, FieldSpan> > patches;
    const auto stitched = stitchFields( stretches, 2, [&] ( uint64_t k, const FieldSpan& field ) { patches.emplace_back( k, field ); } );
    CHECK( stitched.closed == 2 && stitched.hasTail && ( stitched.tail == FieldSpan{ 24, -1 } ) );
    CHECK( patches.size() == 1 && patches[0].first == 1 && ( patches[0].second == FieldSpan{ 8, 8 } ) );
    CHECK( stitchedFields( stretches, 2 ) == direct( text, '\n', ',', 2 ) );
    for ( const uint32_t j : { 0u, 1u, 3u, 4u } ) {
        for ( size_t k = 0; k < pieces.size(); ++k ) {
            const auto bytes = bytesOf( pieces[k] );
            stretches[k].summary = summariseFields( bytes.data(), bytes.size(), '\n', ',', j, 3 );
        }
        CHECK( stitchedFields( stretches, j ) == direct( text, '\n', ',', j ) );
    }
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
    const auto nothing = [] ( uint64_t, const FieldSpan& ) {};
    const Bytes text = bytesOf( "a,,\ncd" );
    std::vector<FieldStretch> stretches( 2 );
    stretches[0].summary = summariseFields( text.data(), 4, '\n', ',', 1, 2 );
    stretches[1].fileOffset = 4;
    stretches[1].summary = summariseFields( text.data() + 4, 2, '\n', ',', 1, 2 );
    CHECK( !refused( [&] { (void)stitchFields( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 5;    /* a gap */
    CHECK( refused( [&] { (void)stitchFields( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 3;    /* an overlap */
    CHECK( refused( [&] { (void)stitchFields( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 4;
    CHECK( refused( [&] { (void)stitchFields( stretches, 0, nothing ); } ) );    /* summaries of another field: too many positions */
    stretches[0].summary.starts.clear();        /* a count without its lines cannot be listed */
    CHECK( refused( [&] { (void)stitchedFields( stretches, 1 ); } ) );
    stretches[0].summary.count = 0;             /* a delimiter that closes no line */
    CHECK( refused( [&] { (void)stitchFields( stretches, 1, nothing ); } ) );
    stretches[0].fileOffset = ~uint64_t( 0 ) - 1;   /* the end does not fit 64 bits */
    CHECK( refused( [&] { (void)stitchFields( stretches, 1, nothing ); } ) );
    /* summaries that break the invariants (an unknown start behind enough delimiters) are read within bounds */
    FieldCarry carry{ 5, FIELD_UNKNOWN, FIELD_UNKNOWN };
    const uint64_t position = 3;
    fieldContinue( carry, 2, &position, 1, 0 );
    CHECK( carry.start == FIELD_UNKNOWN && fieldClose( carry, 9 ).size == -1 );
}

/** Stretches of 3 GiB that each close 5 * 2^30 lines: nothing is listed, only the seams are patched. */
void
beyondFourGiB()
{
    const uint64_t size = uint64_t( 3 ) << 30, lines = uint64_t( 5 ) << 30;
    const uint32_t j = 1;
    std::vector<FieldStretch> stretches( 4 );
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        auto& s = stretches[i].summary;
        stretches[i].fileOffset = i * size;
        s = emptyFieldSummary( j );
        s.size = size;
        if ( i == 2 ) {                 /* one piece of a line, with the dl that ends field 1 */
            s.headPositions = { 1000 };
            s.tailDelims = 1;
            s.tailNonEmpty = true;
            continue;
        }
        s.hasDelimiter = true;
        s.count = lines;
        s.firstNl = 500;
        if ( i == 3 ) s.headPositions = { 100, 200 };
        s.tailStart = size - 50;        /* "....,......" : one dl 40 bytes in front of the end */
        s.tailDelims = 1;
        s.tailFieldStart = size - 39;
        s.tailNonEmpty = true;
    }
    std::vector<std::pair<uint64_t, FieldSpan> > patches;
    const auto stitched = stitchFields( stretches, j, [&] ( uint64_t k, const FieldSpan& field ) { patches.emplace_back( k, field ); } );
    CHECK( stitched.closed == 3 * lines && stitched.closed > ( uint64_t( 1 ) << 33 ) );
    CHECK( stitched.hasTail && ( stitched.tail == FieldSpan{ 4 * size - 39, 39 } ) );
    /* stretch 0 is entered empty: no patch; stretch 1's first line is closed line 5 * 2^30, field 1 from the tail of 0 to
     * stretch 1's first nl; stretch 3's is 10 * 2^30, field 1 from the tail of 1 to the dl of 2 */
    CHECK( patches.size() == 2 );
    CHECK( patches[0].first == lines && ( patches[0].second == FieldSpan{ size - 39, 39 + 500 } ) );
    CHECK( patches[1].first == 2 * lines && ( patches[1].second == FieldSpan{ 2 * size - 39, 39 + 1000 } ) );
    CHECK( patches[1].second.start > ( uint64_t( 1 ) << 32 ) );
    /* a missing field beyond 2^32: field 3 of a line with two delimiters */
    for ( auto& stretch : stretches ) {
        auto& s = stretch.summary;
        s.tailFieldStart = FIELD_UNKNOWN;
    }
    patches.clear();
    (void)stitchFields( stretches, 3, [&] ( uint64_t k, const FieldSpan& field ) { patches.emplace_back( k, field ); } );
    CHECK( patches.size() == 2 && ( patches[0].second == FieldSpan{ size + 500, -1 } ) );
    /* tail of 1 has one dl, stretch 2 one, stretch 3's head two: the third dl is at 3 * size + 100 and starts field 3 */
    CHECK( ( patches[1].second == FieldSpan{ 3 * size + 101, 99 } ) );
}

/** Four blocks of 100 bytes with 3, 0, 2 and 1 delimiters: the blocks are those of planLineHashes. */
void
plans()
{
    const std::vector<std::pair<uint64_t, uint64_t> > map{ { 32, 0 }, { 1000, 100 }, { 2000, 200 }, { 3000, 300 }, { 4000, 400 } };
    const uint64_t lineBytes[] = { 0, 100, 200, 300, 400 }, lineLines[] = { 0, 3, 3, 5, 6 };
    const auto plan = [&] ( uint64_t first, uint64_t count ) {
        return planFields( map, lineBytes, lineLines, 5, first, count, 64, false, 4100 );
    };
    const auto covered = [] ( const FieldPlan& p ) {
        uint64_t begin = p.stretches.empty() ? 0 : p.stretches.front().fileOffset, end = begin;
        for ( const auto& piece : p.stretches ) {
            CHECK( piece.fileOffset == end );
            end += piece.size;
        }
        return std::make_pair( begin, end );
    };
    auto p = plan( 0, ~uint64_t( 0 ) );
    CHECK( p.count == 7 && p.reachesEnd && p.firstClosed == 0 && p.N == 6 && covered( p ) == std::make_pair( uint64_t( 0 ), uint64_t( 400 ) ) );
    size_t blocks = 0;
    for ( const auto& launch : p.launches ) blocks += launch.bits.size();
    CHECK( blocks == 4 );
    p = plan( 3, 1 );      /* line 3 starts behind block 0's last delimiter and is closed in block 2 */
    CHECK( p.count == 1 && p.firstClosed == 0 && covered( p ) == std::make_pair( uint64_t( 0 ), uint64_t( 300 ) ) );
    p = plan( 4, 2 );
    CHECK( p.count == 2 && !p.reachesEnd && p.firstClosed == 3 && covered( p ) == std::make_pair( uint64_t( 200 ), uint64_t( 400 ) ) );
    p = plan( 6, 1 );      /* the tail alone */
    CHECK( p.count == 1 && p.reachesEnd && p.firstClosed == 5 && covered( p ) == std::make_pair( uint64_t( 300 ), uint64_t( 400 ) ) );
    p = plan( 7, 1 );
    CHECK( p.count == 0 && p.launches.empty() && p.stretches.empty() );
    p = plan( 2, 0 );
    CHECK( p.count == 0 && p.launches.empty() && p.stretches.empty() );
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0xF1E1D );
    knownAnswers();
    summaries( rng );
    saturation();
    longLine();
    refusals();
    beyondFourGiB();
    plans();
    std::puts( "fields cases ok" );
    return 0;
}
