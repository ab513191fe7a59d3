/**
 * fieldnum_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldnum.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: known answers of the definition, FieldText and its saturating concatenation,
 * summariseFieldNumbers against the direct definition and independent of the chunk size, stitchFieldNumbers over random
 * cuts, a number that crosses three stretches, its refusals, and the layout of the launcher's lists
 * (bz2_query_layout.hpp: layFieldNumbers) region by region.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fieldnum.hpp"
#include "../../indexed_bzip2_amd/csrc/bz2_query_layout.hpp"

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

int64_t
parse( const std::string& s )
{
    /* from a buffer of exactly the field's size: a read beyond it is the sanitizer's to find */
    const Bytes bytes = bytesOf( s );
    return parseFieldNumber( bytes.data(), bytes.size() );
}

/** The definition once more, as a state machine over the bytes: sign?, then 1 to 18 digits, then the end. */
int64_t
naiveNumber( const Bytes& data, size_t from, size_t size )
{
    size_t at = 0;
    bool negative = false;
    if ( at < size && ( data[from] == '+' || data[from] == '-' ) ) negative = data[from + at++] == '-';
    const size_t digits = size - at;
    if ( digits < 1 || digits > 18 ) return FIELD_NOT_A_NUMBER;
    unsigned long long value = 0;
    for ( ; at < size; ++at ) {
        if ( data[from + at] < '0' || data[from + at] > '9' ) return FIELD_NOT_A_NUMBER;
        value = value * 10 + ( data[from + at] - '0' );
    }
    return negative ? -(int64_t)value : (int64_t)value;
}

/** Number and span of field j of the content data[s, end), by splitting it naively into its parts first. */
FieldNumber
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
    if ( j >= parts.size() ) return { FIELD_NUMBER_MISSING, { end, -1 } };
    return { naiveNumber( data, parts[j].first, parts[j].second ), { parts[j].first, (int64_t)parts[j].second } };
}

/** Every line of `data` by the definition: a non-empty unterminated tail is one more line. */
std::vector<FieldNumber>
direct( const Bytes& data, uint8_t nl, uint8_t dl, uint32_t j )
{
    std::vector<FieldNumber> numbers;
    size_t from = 0;
    for ( size_t at = 0; at < data.size(); ++at ) {
        if ( data[at] != nl ) continue;
        numbers.push_back( naiveField( data, from, at, dl, j ) );
        CHECK( numbers.back().number == fieldNumber( data.data() + from, at - from, dl, j ) );
        from = at + 1;
    }
    if ( from < data.size() ) numbers.push_back( naiveField( data, from, data.size(), dl, j ) );
    return numbers;
}

Bytes
randomBytes( std::mt19937_64& rng, size_t size, uint8_t nl, uint8_t dl )
{
    const uint8_t alphabet[] = { '0', '9', '-', '+', 'a', nl, dl, dl, 0xFF, '1', '7' };
    Bytes data( size );
    for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
    return data;
}

bool
sameFields( const FieldSummary& a, const FieldSummary& b )
{
    return a.size == b.size && a.hasDelimiter == b.hasDelimiter && a.tailNonEmpty == b.tailNonEmpty && a.count == b.count
           && a.firstNl == b.firstNl && a.headPositions == b.headPositions && a.tailStart == b.tailStart
           && a.tailDelims == b.tailDelims && a.tailFieldStart == b.tailFieldStart && a.tailFieldEnd == b.tailFieldEnd
           && a.starts == b.starts && a.sizes == b.sizes;
}

bool
same( const FieldNumberSummary& a, const FieldNumberSummary& b )
{
    return sameFields( a.fields, b.fields ) && a.headTexts == b.headTexts && a.tailText == b.tailText && a.numbers == b.numbers;
}

void
knownAnswers()
{
    CHECK( FIELD_NOT_A_NUMBER == INT64_MIN && FIELD_NUMBER_MISSING == INT64_MIN + 1 );
    CHECK( parse( "" ) == FIELD_NOT_A_NUMBER && parse( "+" ) == FIELD_NOT_A_NUMBER && parse( "-" ) == FIELD_NOT_A_NUMBER );
    CHECK( parse( "-0" ) == 0 && parse( "+0" ) == 0 && parse( "0" ) == 0 && parse( "007" ) == 7 && parse( "-12" ) == -12 && parse( "+12" ) == 12 );
    CHECK( parse( "999999999999999999" ) == 999999999999999999ll && parse( "-999999999999999999" ) == -999999999999999999ll );
    CHECK( parse( "+999999999999999999" ) == 999999999999999999ll && parse( "000000000000000001" ) == 1 );
    CHECK( parse( "1000000000000000000" ) == FIELD_NOT_A_NUMBER && parse( "0000000000000000001" ) == FIELD_NOT_A_NUMBER );
    CHECK( parse( "-1000000000000000000" ) == FIELD_NOT_A_NUMBER && parse( "12345678901234567890" ) == FIELD_NOT_A_NUMBER );
    for ( const char* const text : { "1 ", " 1", "1_0", "/", ":", "\xb1", "+-1", "1-", "1/", "1:", "0x10", "1.5", "1e3", "--1", "1+" } ) {
        CHECK( parse( text ) == FIELD_NOT_A_NUMBER );
    }
    /* no value takes a sentinel */
    CHECK( parse( "-999999999999999999" ) > FIELD_NUMBER_MISSING );

    /* texts: 19 bytes are kept, the size saturates at 20, concatenation saturates */
    const Bytes digits = bytesOf( "1234567890123456789012345" );
    for ( size_t n = 0; n <= digits.size(); ++n ) {
        const FieldText text = fieldText( digits.data(), n );
        CHECK( text.size == std::min<size_t>( n, 20 ) );
        for ( size_t i = 0; i < 19; ++i ) CHECK( text.bytes[i] == ( i < n ? digits[i] : 0 ) );
        for ( size_t cut = 0; cut <= n; ++cut ) {
            CHECK( followedBy( fieldText( digits.data(), cut ), fieldText( digits.data() + cut, n - cut ) ) == text );
        }
        CHECK( parseFieldNumber( text ) == ( n >= 1 && n <= 18 ? parseFieldNumber( digits.data(), n ) : FIELD_NOT_A_NUMBER ) );
    }

    const Bytes text = bytesOf( "a\t12\t\n\n-7\n\t\t+3" );
    /* lines: "a\t12\t", "", "-7", "\t\t+3" */
    const auto numbers = [&] ( uint32_t j ) {
        std::vector<int64_t> result;
        for ( const auto& number : direct( text, '\n', '\t', j ) ) result.push_back( number.number );
        return result;
    };
    const int64_t nan = FIELD_NOT_A_NUMBER, none = FIELD_NUMBER_MISSING;
    CHECK( ( numbers( 0 ) == std::vector<int64_t>{ nan, nan, -7, nan } ) );
    CHECK( ( numbers( 1 ) == std::vector<int64_t>{ 12, none, none, nan } ) );
    CHECK( ( numbers( 2 ) == std::vector<int64_t>{ nan, none, none, 3 } ) );
    CHECK( ( numbers( 3 ) == std::vector<int64_t>( 4, none ) ) );
    for ( uint32_t j = 0; j < 5; ++j ) {
        std::vector<FieldNumberStretch> one( 1 );
        one[0].summary = summariseFieldNumbers( text.data(), text.size(), '\n', '\t', j, 3 );
        CHECK( stitchedFieldNumbers( one, j ) == direct( text, '\n', '\t', j ) );
    }
}

void
summaries( std::mt19937_64& rng )
{
    const uint32_t fieldsTried[] = { 0, 1, 2, 5, 1023 };
    const uint8_t delimiters[] = { '\t', ',', 0xFF, 1 };
    for ( int round = 0; round < 4000; ++round ) {
        const uint8_t nl = round % 3 == 0 ? 0 : '\n', dl = delimiters[round % 4];
        const uint32_t j = fieldsTried[round % 7 != 0 ? round % 5 : rng() % 5];
        const auto data = randomBytes( rng, rng() % 200, nl, dl );
        const auto want = direct( data, nl, dl, j );
        const auto whole = summariseFieldNumberChunk( data.data(), data.size(), nl, dl, j );
        CHECK( sameFields( whole.fields, summariseFieldChunk( data.data(), data.size(), nl, dl, j ) ) );
        CHECK( whole.headTexts.size() == headTextCount( whole.fields.headDelims(), j ) && whole.numbers.size() == whole.fields.count );
        for ( const size_t chunk : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 7 ), size_t( 16 ), size_t( 19 ), size_t( 20 ), size_t( 64 ), size_t( 256 ) } ) {
            CHECK( same( whole, summariseFieldNumbers( data.data(), data.size(), nl, dl, j, chunk ) ) );
        }
        std::vector<FieldNumberStretch> one( 1 );
        one[0].summary = whole;
        CHECK( stitchedFieldNumbers( one, j ) == want );
        /* 0 to 6 random cuts, each stretch summarised with a chunk size of its own */
        std::vector<size_t> cuts{ 0, data.size() };
        for ( uint64_t k = rng() % 7; k > 0; --k ) cuts.push_back( rng() % ( data.size() + 1 ) );
        std::sort( cuts.begin(), cuts.end() );
        std::vector<FieldNumberStretch> stretches;
        for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
            FieldNumberStretch stretch;
            stretch.fileOffset = cuts[k];
            stretch.summary = summariseFieldNumbers( data.data() + cuts[k], cuts[k + 1] - cuts[k], nl, dl, j, 1 + rng() % 64 );
            stretches.push_back( std::move( stretch ) );
        }
        CHECK( stitchedFieldNumbers( stretches, j ) == want );
    }
    try {
        (void)summariseFieldNumbers( nullptr, 0, '\n', '\t', 0, 0 );
        CHECK( false );
    } catch ( const std::invalid_argument& ) {}
}

/** Long digit strings cut everywhere: 17, 18, 19 and 20 digits with and without a sign, every cut position, so that the
 * texts saturate on either side of a seam. */
void
longNumbers()
{
    std::string text;
    for ( const size_t digits : { size_t( 17 ), size_t( 18 ), size_t( 19 ), size_t( 20 ) } ) {
        for ( const char* const sign : { "", "-", "+" } ) text += "k," + std::string( sign ) + std::string( digits, '9' ) + ",x\n";
    }
    text += "k,-,\nk,,\nk\nk,12";
    const Bytes data = bytesOf( text );
    for ( const uint32_t j : { 0u, 1u, 2u } ) {
        const auto want = direct( data, '\n', ',', j );
        for ( size_t cut = 0; cut <= data.size(); ++cut ) {
            std::vector<FieldNumberStretch> stretches( 2 );
            stretches[0].summary = summariseFieldNumbers( data.data(), cut, '\n', ',', j, 5 );
            stretches[1].fileOffset = cut;
            stretches[1].summary = summariseFieldNumbers( data.data() + cut, data.size() - cut, '\n', ',', j, 7 );
            CHECK( stitchedFieldNumbers( stretches, j ) == want );
        }
        for ( size_t piece = 1; piece < 24; ++piece ) {
            std::vector<FieldNumberStretch> stretches;
            for ( size_t at = 0; at < data.size(); at += piece ) {
                FieldNumberStretch stretch;
                stretch.fileOffset = at;
                stretch.summary = summariseFieldNumbers( data.data() + at, std::min( piece, data.size() - at ), '\n', ',', j, 3 );
                stretches.push_back( std::move( stretch ) );
            }
            CHECK( stitchedFieldNumbers( stretches, j ) == want );
        }
    }
    const auto second = direct( data, '\n', ',', 1 );
    CHECK( second[0].number == 99999999999999999ll && second[1].number == -99999999999999999ll && second[3].number == 999999999999999999ll );
    CHECK( second[4].number == -999999999999999999ll && second[6].number == FIELD_NOT_A_NUMBER && second[7].number == FIELD_NOT_A_NUMBER );
    CHECK( second[12].number == FIELD_NOT_A_NUMBER && second[13].number == FIELD_NOT_A_NUMBER && second[14].number == FIELD_NUMBER_MISSING );
    CHECK( second[15].number == 12 && second.size() == 16 );
}

/** One line through five stretches: field 2 starts in the second, crosses the third and ends in the fourth. */
void
longLine()
{
    const std::vector<std::string> pieces{ "x\nab,c", "d,123", "456", "78,m", "no\nq,r" };
    Bytes text;
    std::vector<FieldNumberStretch> stretches;
    for ( const auto& piece : pieces ) {
        FieldNumberStretch stretch;
        stretch.fileOffset = text.size();
        const auto bytes = bytesOf( piece );
        stretch.summary = summariseFieldNumbers( bytes.data(), bytes.size(), '\n', ',', 2, 2 );
        stretches.push_back( std::move( stretch ) );
        text.insert( text.end(), bytes.begin(), bytes.end() );
    }
    std::vector<std::pair<uint64_t, FieldNumber> > patches;
    const auto stitched = stitchFieldNumbers( stretches, 2, [&] ( uint64_t k, int64_t number, const FieldSpan& field ) {
        patches.push_back( { k, { number, field } } );
    } );
    CHECK( stitched.closed == 2 && stitched.hasTail && stitched.tailNumber == FIELD_NUMBER_MISSING && ( stitched.tail == FieldSpan{ 24, -1 } ) );
    CHECK( patches.size() == 1 && patches[0].first == 1 && ( patches[0].second == FieldNumber{ 12345678, { 8, 8 } } ) );
    for ( const uint32_t j : { 0u, 1u, 2u, 3u, 4u } ) {
        for ( size_t k = 0; k < pieces.size(); ++k ) {
            const auto bytes = bytesOf( pieces[k] );
            stretches[k].summary = summariseFieldNumbers( bytes.data(), bytes.size(), '\n', ',', j, 3 );
        }
        CHECK( stitchedFieldNumbers( stretches, j ) == direct( text, '\n', ',', j ) );
    }
    /* from a line start that is not offset 0, beyond 2^33: the numbers stay, the spans move */
    const uint64_t far = ( uint64_t( 1 ) << 33 ) + 5;
    for ( auto& stretch : stretches ) stretch.fileOffset += far;
    auto moved = direct( text, '\n', ',', 4 );
    for ( auto& number : moved ) number.field.start += far;
    CHECK( stitchedFieldNumbers( stretches, 4 ) == moved );
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
    const auto nothing = [] ( uint64_t, int64_t, const FieldSpan& ) {};
    const Bytes text = bytesOf( "a,,\ncd" );
    std::vector<FieldNumberStretch> stretches( 2 );
    stretches[0].summary = summariseFieldNumbers( text.data(), 4, '\n', ',', 1, 2 );
    stretches[1].fileOffset = 4;
    stretches[1].summary = summariseFieldNumbers( text.data() + 4, 2, '\n', ',', 1, 2 );
    CHECK( !refused( [&] { (void)stitchFieldNumbers( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 5;    /* a gap */
    CHECK( refused( [&] { (void)stitchFieldNumbers( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 4;
    CHECK( refused( [&] { (void)stitchFieldNumbers( stretches, 0, nothing ); } ) );    /* too many positions */
    stretches[0].summary.headTexts.pop_back();  /* a head without all its texts */
    CHECK( refused( [&] { (void)stitchFieldNumbers( stretches, 1, nothing ); } ) );
    stretches[0].summary = summariseFieldNumbers( text.data(), 4, '\n', ',', 1, 2 );
    stretches[0].summary.numbers.clear();       /* a count without its lines cannot be listed */
    CHECK( refused( [&] { (void)stitchedFieldNumbers( stretches, 1 ); } ) );
    stretches[0].summary.fields.count = 0;      /* a delimiter that closes no line */
    CHECK( refused( [&] { (void)stitchFieldNumbers( stretches, 1, nothing ); } ) );
    stretches[0].fileOffset = ~uint64_t( 0 ) - 1;
    CHECK( refused( [&] { (void)stitchFieldNumbers( stretches, 1, nothing ); } ) );
}

/** layFieldNumbers: the regions in their order, each aligned as its loads need, none overlapping the next. */
void
layout()
{
    /* the record sizes and constants that bz2_queries.hip.h pins */
    const QuerySizes sizes{ 16, 16, 16, 256, 24, 21504, 256, 8, 64, 16, 48, 64, 16, 24, 56, 16 };
    for ( const uint64_t nTiles : { uint64_t( 0 ), uint64_t( 1 ), uint64_t( 7 ), uint64_t( 6554 ) } ) {
        for ( const uint64_t n : { uint64_t( 1 ), uint64_t( 3 ), uint64_t( 600 ) } ) {
            for ( const uint64_t field : { uint64_t( 0 ), uint64_t( 2 ), uint64_t( 1023 ) } ) {
                const auto l = layFieldNumbers( sizes, nTiles, n, field );
                const uint64_t slots = nTiles * 256;
                const auto up = [] ( uint64_t at, uint64_t alignment ) { return ( at + alignment - 1 ) / alignment * alignment; };
                uint64_t at = 0;
                CHECK( l.tilesAt == at );
                at = up( at + nTiles * 16, 16 );
                CHECK( l.spansAt == at );
                at = up( at + n * 24, 16 );
                CHECK( l.extentsAt == at );
                at = up( at + n * 16, 16 );
                CHECK( l.resultsAt == at );
                at = up( at + n * 56, 16 );
                CHECK( l.headsAt == at );
                at = up( at + n * ( field + 1 ) * 8, 16 );
                CHECK( l.headTextsAt == at );
                at = up( at + n * ( field + 1 ) * 20, 16 );
                CHECK( l.tailTextsAt == at );
                at = up( at + n * 20, 16 );
                CHECK( l.tileSummariesAt == at );
                at = up( at + nTiles * 16, 16 );
                CHECK( l.placesAt == at );
                at += slots * 8;
                CHECK( l.prefixesAt == at && l.countsAt == at + slots * 4 && l.bytes == at + slots * 8 );
            }
        }
    }
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0xF1E1D );
    knownAnswers();
    summaries( rng );
    longNumbers();
    longLine();
    refusals();
    layout();
    std::puts( "fieldnum cases ok" );
    return 0;
}
