/**
 * fieldmatch_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldmatch.hpp on the CPU, as a program of its own that the test
 * suite builds with -fsanitize=address,undefined: buildValueTable against the plain model valueMatches on seeded random
 * sets and probes, the image the kernel reads re-read field by field, duplicates, the sets of 1, 2, 1 023 and 1 024 values,
 * the sizes 0, 1, 255 and 256, the caps, forged equal keys for two different values (refused) and for two equal ones
 * (accepted), the clipping of a range, and the launcher's layout (bz2_query_layout.hpp: layFieldMatch).
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fieldmatch.hpp"
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
using Values = std::vector<std::string>;

std::vector<uint64_t>
keysOf( const Values& values, uint64_t seed )
{
    std::vector<uint64_t> keys;
    for ( const auto& value : values ) keys.push_back( lineHash( reinterpret_cast<const uint8_t*>( value.data() ), value.size(), seed ) );
    return keys;
}

/** What k_field_match does with the image alone: the search, the size and the bytes, from exactly sized buffers. */
bool
imageHolds( const ValueTable& table, uint64_t key, const std::string& field, bool present )
{
    if ( !present ) return false;
    const uint32_t k = table.count();
    const std::vector<uint8_t> image = table.image;      /* a copy of exactly its size: a read beyond it is the sanitizer's */
    CHECK( image.size() % 4 == 0 && image.size() <= FIELDMATCH_IMAGE_MAX && image.size() >= (size_t)k * 12 + 4 );
    const auto keyAt = [&] ( uint32_t i ) { uint64_t v; std::memcpy( &v, image.data() + (size_t)i * 8, 8 ); return v; };
    const auto offsetAt = [&] ( uint32_t i ) { uint32_t v; std::memcpy( &v, image.data() + (size_t)k * 8 + (size_t)i * 4, 4 ); return v; };
    const uint8_t* const bytes = image.data() + (size_t)k * 12 + 4;
    uint32_t lo = 0, hi = k, steps = 0;
    while ( hi - lo > 1 ) {
        const uint32_t mid = ( lo + hi ) / 2;
        if ( keyAt( mid ) <= key ) lo = mid; else hi = mid;
        ++steps;
    }
    CHECK( steps <= 10 );
    if ( keyAt( lo ) != key ) return false;
    const uint32_t from = offsetAt( lo ), length = offsetAt( lo + 1 ) - from;
    CHECK( (size_t)k * 12 + 4 + from + length <= image.size() );
    return length == field.size() && std::memcmp( bytes + from, field.data(), length ) == 0;
}

bool
tableHolds( const ValueTable& table, uint64_t seed, const std::string& field, bool present )
{
    const std::vector<uint8_t> exact( field.begin(), field.end() );
    const uint64_t key = lineHash( exact.data(), exact.size(), seed );
    const bool held = table.holds( key, exact.data(), present ? (int64_t)exact.size() : -1 );
    CHECK( held == imageHolds( table, key, field, present ) );
    return held;
}

std::string
refusal( const Values& values, const std::vector<uint64_t>& keys )
{
    try {
        (void)buildValueTable( values, keys );
    } catch ( const std::invalid_argument& refused ) {
        return refused.what();
    }
    return {};
}

void
knownAnswers()
{
    const Values values{ "GET", "", "GE", "GET", "a\tb", std::string( "\0x", 2 ), "\x80\xff" };
    const auto table = buildValueTable( values, keysOf( values, 0 ) );
    CHECK( table.count() == 6 );                                  /* "GET" twice counts once */
    for ( uint32_t i = 1; i < table.count(); ++i ) CHECK( table.keys[i - 1] < table.keys[i] );
    CHECK( tableHolds( table, 0, "GET", true ) && tableHolds( table, 0, "GE", true ) && tableHolds( table, 0, "", true ) );
    CHECK( !tableHolds( table, 0, "G", true ) && !tableHolds( table, 0, "GETS", true ) && !tableHolds( table, 0, "get", true ) );
    CHECK( !tableHolds( table, 0, "", false ) && !tableHolds( table, 0, "GET", false ) );     /* a missing field matches nothing */
    CHECK( tableHolds( table, 0, std::string( "\0x", 2 ), true ) && !tableHolds( table, 0, std::string( "\0y", 2 ), true ) );
    CHECK( tableHolds( table, 0, "\x80\xff", true ) && !tableHolds( table, 0, "\x80", true ) );
    CHECK( valueMatches( values, nullptr, 0 ) && !valueMatches( values, nullptr, -1 ) );
    const Values none{ "x" };
    const auto one = buildValueTable( none, keysOf( none, 0 ) );
    CHECK( !tableHolds( one, 0, "", true ) && tableHolds( one, 0, "x", true ) );                 /* no empty value: no empty field */
    /* the answer does not depend on the seed */
    for ( const uint64_t seed : { 1ull, 2ull, ~0ull } ) {
        const auto other = buildValueTable( values, keysOf( values, seed ) );
        CHECK( other.count() == 6 && tableHolds( other, seed, "GE", true ) && !tableHolds( other, seed, "G", true ) );
    }
}

void
randomSets()
{
    std::mt19937_64 rng( 0xF1E1DA7C );
    const std::string alphabet( "ab\0\xff\t0", 6 );
    uint64_t hits = 0, misses = 0;
    for ( int round = 0; round < 2000; ++round ) {
        const uint64_t seed = round % 3;
        const size_t n = 1 + rng() % ( round % 50 == 0 ? 300 : 12 );
        Values values( n );
        for ( auto& value : values ) {
            value.resize( rng() % 5 );
            for ( auto& c : value ) c = alphabet[rng() % alphabet.size()];
        }
        const auto table = buildValueTable( values, keysOf( values, seed ) );
        CHECK( table.count() <= n && table.count() >= 1 );
        for ( int probe = 0; probe < 30; ++probe ) {
            std::string field( rng() % 5, 'a' );
            for ( auto& c : field ) c = alphabet[rng() % alphabet.size()];
            if ( probe % 3 == 0 ) field = values[rng() % n];
            const bool present = probe % 7 != 6;
            const std::vector<uint8_t> exact( field.begin(), field.end() );
            const bool want = valueMatches( values, exact.data(), present ? (int64_t)exact.size() : -1 );
            CHECK( tableHolds( table, seed, field, present ) == want );
            ( want ? hits : misses ) += 1;
        }
    }
    CHECK( hits > 10000 && misses > 10000 );
}

void
sizesAndCaps()
{
    for ( const size_t n : { size_t( 1 ), size_t( 2 ), size_t( 1023 ), size_t( 1024 ) } ) {
        Values values( n );
        for ( size_t i = 0; i < n; ++i ) values[i] = "v" + std::to_string( i );
        const auto table = buildValueTable( values, keysOf( values, 0 ) );
        CHECK( table.count() == n );
        CHECK( tableHolds( table, 0, "v0", true ) && tableHolds( table, 0, "v" + std::to_string( n - 1 ), true ) );
        CHECK( !tableHolds( table, 0, "v" + std::to_string( n ), true ) && !tableHolds( table, 0, "v", true ) );
        for ( size_t i = 0; i < n; i += 37 ) CHECK( tableHolds( table, 0, values[i], true ) );
    }
    Values tooMany( 1025, "x" );
    CHECK( refusal( tooMany, keysOf( tooMany, 0 ) ).find( "1 to 1024 values, not 1025" ) != std::string::npos );
    CHECK( refusal( {}, {} ).find( "1 to 1024 values, not 0" ) != std::string::npos );
    CHECK( !refusal( { "a" }, {} ).empty() );

    const Values sizes{ "", "a", std::string( 255, 'p' ), std::string( 256, 'q' ) };
    const auto table = buildValueTable( sizes, keysOf( sizes, 0 ) );
    CHECK( table.count() == 4 );
    for ( const auto& value : sizes ) CHECK( tableHolds( table, 0, value, true ) );
    CHECK( !tableHolds( table, 0, std::string( 257, 'q' ), true ) && !tableHolds( table, 0, std::string( 255, 'q' ), true ) );
    CHECK( !tableHolds( table, 0, std::string( 254, 'p' ) + "q", true ) );
    const Values tooLong{ std::string( 257, 'q' ) };
    CHECK( refusal( tooLong, keysOf( tooLong, 0 ) ).find( "value 0 has 257 bytes" ) != std::string::npos );

    /* the total: 64 values of 256 bytes are 16 384 bytes and the largest image; one byte more is refused */
    Values full( 64 );
    for ( size_t i = 0; i < full.size(); ++i ) full[i] = std::string( 255, 'a' ) + (char)( 1 + i );
    const auto fullTable = buildValueTable( full, keysOf( full, 0 ) );
    CHECK( fullTable.count() == 64 && fullTable.image.size() == 64 * 12 + 4 + 16384 );
    CHECK( tableHolds( fullTable, 0, full[63], true ) && !tableHolds( fullTable, 0, std::string( 256, 'a' ), true ) );
    full.push_back( "x" );
    CHECK( refusal( full, keysOf( full, 0 ) ).find( "at most 16384 bytes in total, not 16385" ) != std::string::npos );
    Values many( 1024 );
    for ( size_t i = 0; i < many.size(); ++i ) many[i] = std::string( 12, 'a' ) + std::to_string( 1000 + i );
    CHECK( buildValueTable( many, keysOf( many, 0 ) ).image.size() == 1024 * 12 + 4 + 16384 );
    static_assert( FIELDMATCH_IMAGE_MAX == 1024 * 12 + 4 + 16384 );
}

void
forgedKeys()
{
    /* two different values under one key are refused, and the message names both and the way out */
    const auto why = refusal( { "alpha", "be\"ta\x01" }, { 77, 77 } );
    CHECK( why.find( "\"alpha\"" ) != std::string::npos && why.find( "\"be\\x22ta\\x01\"" ) != std::string::npos );
    CHECK( why.find( "pass another seed" ) != std::string::npos );
    CHECK( !refusal( { "a", "b", "c" }, { 5, 9, 5 } ).empty() );
    /* two equal values under one key are one value */
    const auto table = buildValueTable( { "same", "other", "same" }, { 77, 12, 77 } );
    CHECK( table.count() == 2 && table.keys[0] == 12 && table.keys[1] == 77 && table.values[1] == "same" );
    /* a forged key alone does not match: the bytes decide */
    const std::string field = "samf";
    CHECK( !table.holds( 77, reinterpret_cast<const uint8_t*>( field.data() ), 4 ) && !imageHolds( table, 77, field, true ) );
    CHECK( table.holds( 77, reinterpret_cast<const uint8_t*>( "same" ), 4 ) && imageHolds( table, 77, "same", true ) );
    CHECK( table.candidateValue( 77, 4 ) == 1 && table.candidateValue( 77, 5 ) == 2 && table.candidateValue( 78, 4 ) == 2 );
    CHECK( table.candidateValue( 77, -1 ) == 2 );
}

void
ranges()
{
    const int64_t most = FIELDMATCH_NUMBER_MAX;
    CHECK( most == 999999999999999999ll );
    const auto all = clipNumberRange( false, 0, false, 0 );
    CHECK( all.lo == -most && all.hi == most && all.holds( 0 ) && all.holds( most ) && all.holds( -most ) );
    CHECK( !all.holds( FIELD_NOT_A_NUMBER ) && !all.holds( FIELD_NUMBER_MISSING ) );
    const auto one = clipNumberRange( true, 5, true, 5 );
    CHECK( one.holds( 5 ) && !one.holds( 4 ) && !one.holds( 6 ) );
    const auto empty = clipNumberRange( true, 6, true, 5 );
    CHECK( !empty.holds( 5 ) && !empty.holds( 6 ) );
    const auto clipped = clipNumberRange( true, INT64_MIN, true, INT64_MAX );
    CHECK( clipped.lo == -most && clipped.hi == most && !clipped.holds( FIELD_NOT_A_NUMBER ) && !clipped.holds( FIELD_NUMBER_MISSING ) );
    const auto low = clipNumberRange( false, 0, true, -3 );
    CHECK( low.holds( -3 ) && low.holds( -most ) && !low.holds( -2 ) && !low.holds( FIELD_NUMBER_MISSING ) );
    const auto high = clipNumberRange( true, -3, false, 0 );
    CHECK( high.holds( -3 ) && high.holds( most ) && !high.holds( -4 ) );
}

void
layout()
{
    const auto l = layFieldMatch( 28676 );
    CHECK( l.imageAt == 0 && l.bytes == 28676 );
    CHECK( layFieldMatch( 16 ).bytes == 16 );
}
}  // namespace

int
main()
{
    knownAnswers();
    randomSets();
    sizesAndCaps();
    forgedKeys();
    ranges();
    layout();
    std::printf( "fieldmatch cases ok\n" );
    return 0;
}
