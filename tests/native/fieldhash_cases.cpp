/**
 * fieldhash_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldhash.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: known answers, the prefix-difference key against split-then-hash,
 * summariseFieldHashes against the direct definition and independent of the chunk size, stitchFieldHashes over random
 * cuts, a field that crosses three stretches, its refusals, stretches beyond 2^33 (synthetic summaries, no bytes), and the
 * layout of the launcher's lists (bz2_query_layout.hpp: layFieldHashes) against the same arithmetic region by region.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fieldhash.hpp"
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

/** Key and span of field j of the content data[s, end), by splitting it naively into its parts first. */
FieldKey
naiveKey( const Bytes& data, size_t s, size_t end, uint8_t dl, uint32_t j, uint64_t seed )
{
    std::vector<std::pair<size_t, size_t> > parts;   /* begin, size */
    size_t from = s;
    for ( size_t at = s; at < end; ++at ) {
        if ( data[at] != dl ) continue;
        parts.emplace_back( from, at - from );
        from = at + 1;
    }
    parts.emplace_back( from, end - from );
    if ( j >= parts.size() ) return { FIELD_MISSING, { end, -1 } };
    return { lineHash( data.data() + parts[j].first, parts[j].second, seed ), { parts[j].first, (int64_t)parts[j].second } };
}

/** Every line of `data` by the definition: a non-empty unterminated tail is one more line. */
std::vector<FieldKey>
direct( const Bytes& data, uint8_t nl, uint8_t dl, uint32_t j, uint64_t seed )
{
    std::vector<FieldKey> keys;
    size_t from = 0;
    for ( size_t at = 0; at < data.size(); ++at ) {
        if ( data[at] != nl ) continue;
        keys.push_back( naiveKey( data, from, at, dl, j, seed ) );
        CHECK( keys.back().key == fieldHash( data.data() + from, at - from, dl, j, seed ) );
        from = at + 1;
    }
    if ( from < data.size() ) keys.push_back( naiveKey( data, from, data.size(), dl, j, seed ) );
    return keys;
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
sameFields( const FieldSummary& a, const FieldSummary& b )
{
    return a.size == b.size && a.hasDelimiter == b.hasDelimiter && a.tailNonEmpty == b.tailNonEmpty && a.count == b.count
           && a.firstNl == b.firstNl && a.headPositions == b.headPositions && a.tailStart == b.tailStart
           && a.tailDelims == b.tailDelims && a.tailFieldStart == b.tailFieldStart && a.tailFieldEnd == b.tailFieldEnd
           && a.starts == b.starts && a.sizes == b.sizes;
}

bool
same( const FieldHashSummary& a, const FieldHashSummary& b )
{
    /* the prefixes at the tail's field are compared where they are reached */
    const bool startReached = a.fields.tailFieldStart != FIELD_UNKNOWN, endReached = a.fields.tailFieldEnd != FIELD_UNKNOWN;
    return sameFields( a.fields, b.fields ) && a.head == b.head && a.tail == b.tail && a.headHashes == b.headHashes
           && ( !startReached || a.tailStartHash == b.tailStartHash ) && ( !endReached || a.tailEndHash == b.tailEndHash )
           && a.keys == b.keys;
}

void
knownAnswers()
{
    const uint64_t seed = 0, x = lineHashBase( seed );
    CHECK( FIELD_MISSING == ( uint64_t( 1 ) << 61 ) - 1 && (int64_t)FIELD_MISSING > 0 );
    CHECK( powmod( x, 0 ) == 1 && powmod( x, 1 ) == x && powmod( x, 5 ) == mulmod( mulmod( mulmod( x, x ), mulmod( x, x ) ), x ) );
    CHECK( submod( 3, 5 ) == LINEHASH_P - 2 && submod( 5, 3 ) == 2 && submod( 0, 0 ) == 0 );
    const Bytes text = bytesOf( "a\tbc\t\n\nx\n\t\ty" );
    /* lines: "a\tbc\t", "", "x", "\t\ty" */
    const auto hashOf = [&] ( const std::string& s ) { return lineHash( reinterpret_cast<const uint8_t*>( s.data() ), s.size(), seed ); };
    const auto keys = [&] ( uint32_t j ) {
        std::vector<uint64_t> result;
        for ( const auto& key : direct( text, '\n', '\t', j, seed ) ) result.push_back( key.key );
        return result;
    };
    CHECK( hashOf( "" ) == 0 && hashOf( "a" ) == 'a' + 1 );
    CHECK( ( keys( 0 ) == std::vector<uint64_t>{ hashOf( "a" ), 0, hashOf( "x" ), 0 } ) );
    CHECK( ( keys( 1 ) == std::vector<uint64_t>{ hashOf( "bc" ), FIELD_MISSING, FIELD_MISSING, 0 } ) );
    CHECK( ( keys( 2 ) == std::vector<uint64_t>{ 0, FIELD_MISSING, FIELD_MISSING, hashOf( "y" ) } ) );
    CHECK( ( keys( 3 ) == std::vector<uint64_t>( 4, FIELD_MISSING ) ) );
    /* "\0" and "\0\0" differ, as fields too */
    const Bytes zeros{ 'k', ',', 0, '\n', 'k', ',', 0, 0, '\n' };
    const auto z = direct( zeros, '\n', ',', 1, seed );
    CHECK( z.size() == 2 && z[0].key == 1 && z[1].key == addmod( x, 1 ) && z[0].key != z[1].key );
    for ( uint32_t j = 0; j < 5; ++j ) {
        std::vector<FieldHashStretch> one( 1 );
        one[0].summary = summariseFieldHashes( x, text.data(), text.size(), '\n', '\t', j, 3 );
        CHECK( stitchedFieldHashes( one, x, '\t', j ) == direct( text, '\n', '\t', j, seed ) );
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
        const uint64_t seed = round % 2 == 0 ? 0 : rng(), x = lineHashBase( seed );
        const auto data = randomBytes( rng, rng() % 200, nl, dl );
        const auto want = direct( data, nl, dl, j, seed );
        const auto whole = summariseFieldHashChunk( x, data.data(), data.size(), nl, dl, j );
        CHECK( sameFields( whole.fields, summariseFieldChunk( data.data(), data.size(), nl, dl, j ) ) );
        const auto lines = summariseChunk( x, data.data(), data.size(), nl );
        CHECK( whole.head == lines.head && whole.tail == lines.tail );
        for ( const size_t chunk : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 7 ), size_t( 16 ), size_t( 64 ), size_t( 256 ) } ) {
            CHECK( same( whole, summariseFieldHashes( x, data.data(), data.size(), nl, dl, j, chunk ) ) );
        }
        CHECK( whole.headHashes.size() == whole.fields.headPositions.size() );
        std::vector<FieldHashStretch> one( 1 );
        one[0].summary = whole;
        CHECK( stitchedFieldHashes( one, x, dl, j ) == want );
        /* 0 to 6 random cuts, each stretch summarised with a chunk size of its own */
        std::vector<size_t> cuts{ 0, data.size() };
        for ( uint64_t k = rng() % 7; k > 0; --k ) cuts.push_back( rng() % ( data.size() + 1 ) );
        std::sort( cuts.begin(), cuts.end() );
        std::vector<FieldHashStretch> stretches;
        for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
            FieldHashStretch stretch;
            stretch.fileOffset = cuts[k];
            stretch.summary = summariseFieldHashes( x, data.data() + cuts[k], cuts[k + 1] - cuts[k], nl, dl, j, 1 + rng() % 64 );
            stretches.push_back( std::move( stretch ) );
        }
        CHECK( stitchedFieldHashes( stretches, x, dl, j ) == want );
    }
    try {
        (void)summariseFieldHashes( 300, nullptr, 0, '\n', '\t', 0, 0 );
        CHECK( false );
    } catch ( const std::invalid_argument& ) {}
}

/** One line through five stretches: field 2 starts in the second, crosses the third and ends in the fourth. */
void
longLine()
{
    const uint64_t seed = 7, x = lineHashBase( seed );
    const std::vector<std::string> pieces{ "x\nab,c", "d,efg", "hij", "kl,m", "no\nq,r" };
    Bytes text;
    std::vector<FieldHashStretch> stretches;
    for ( const auto& piece : pieces ) {
        FieldHashStretch stretch;
        stretch.fileOffset = text.size();
        const auto bytes = bytesOf( piece );
        stretch.summary = summariseFieldHashes( x, bytes.data(), bytes.size(), '\n', ',', 2, 2 );
        stretches.push_back( std::move( stretch ) );
        text.insert( text.end(), bytes.begin(), bytes.end() );
    }
    std::vector<std::pair<uint64_t, FieldKey> > patches;
    const auto stitched = stitchFieldHashes( stretches, x, ',', 2, [&] ( uint64_t k, const FieldKey& key ) { patches.emplace_back( k, key ); } );
    CHECK( stitched.closed == 2 && stitched.hasTail && stitched.tail.key == FIELD_MISSING && ( stitched.tail.field == FieldSpan{ 24, -1 } ) );
    const std::string field = "efghijkl";
    CHECK( patches.size() == 1 && patches[0].first == 1 && ( patches[0].second.field == FieldSpan{ 8, 8 } ) );
    CHECK( patches[0].second.key == lineHash( reinterpret_cast<const uint8_t*>( field.data() ), field.size(), seed ) );
    for ( const uint32_t j : { 0u, 1u, 2u, 3u, 4u } ) {
        for ( size_t k = 0; k < pieces.size(); ++k ) {
            const auto bytes = bytesOf( pieces[k] );
            stretches[k].summary = summariseFieldHashes( x, bytes.data(), bytes.size(), '\n', ',', j, 3 );
        }
        CHECK( stitchedFieldHashes( stretches, x, ',', j ) == direct( text, '\n', ',', j, seed ) );
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
    const uint64_t x = lineHashBase( 0 );
    const auto nothing = [] ( uint64_t, const FieldKey& ) {};
    const Bytes text = bytesOf( "a,,\ncd" );
    std::vector<FieldHashStretch> stretches( 2 );
    stretches[0].summary = summariseFieldHashes( x, text.data(), 4, '\n', ',', 1, 2 );
    stretches[1].fileOffset = 4;
    stretches[1].summary = summariseFieldHashes( x, text.data() + 4, 2, '\n', ',', 1, 2 );
    CHECK( !refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 1, nothing ); } ) );
    stretches[1].fileOffset = 5;    /* a gap */
    CHECK( refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 1, nothing ); } ) );
    stretches[1].fileOffset = 4;
    CHECK( refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 0, nothing ); } ) );    /* too many positions */
    stretches[0].summary.headHashes.clear();    /* positions without their hashes */
    CHECK( refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 1, nothing ); } ) );
    stretches[0].summary = summariseFieldHashes( x, text.data(), 4, '\n', ',', 1, 2 );
    stretches[0].summary.keys.clear();          /* a count without its lines cannot be listed */
    CHECK( refused( [&] { (void)stitchedFieldHashes( stretches, x, ',', 1 ); } ) );
    stretches[0].summary.fields.count = 0;      /* a delimiter that closes no line */
    CHECK( refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 1, nothing ); } ) );
    stretches[0].fileOffset = ~uint64_t( 0 ) - 1;
    CHECK( refused( [&] { (void)stitchFieldHashes( stretches, x, ',', 1, nothing ); } ) );
}

/** Stretches of 3 GiB: nothing is listed, only the seams are patched, and the powers are of offsets beyond 2^32.  The
 * bytes are runs of 'a', so the wanted hashes are sums of a geometric series computed with powmod. */
void
beyondEightGiB()
{
    const uint64_t seed = 3, x = lineHashBase( seed );
    const uint64_t size = uint64_t( 3 ) << 30, lines = uint64_t( 5 ) << 30;
    const uint32_t j = 1;
    /* run( n ) = the hash of n bytes 'a' */
    const auto run = [x] ( uint64_t n ) {
        HashPart part, unit{ uint64_t( 'a' ) + 1, x };
        for ( uint64_t bit = uint64_t( 1 ) << 40; bit != 0; bit >>= 1 ) {
            part = followedBy( part, part );
            if ( ( n & bit ) != 0 ) part = followedBy( part, unit );
        }
        return part;
    };
    const HashPart comma{ uint64_t( ',' ) + 1, x };
    std::vector<FieldHashStretch> stretches( 4 );
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        auto& s = stretches[i].summary;
        stretches[i].fileOffset = i * size;
        s = emptyFieldHashSummary( j );
        s.fields.size = size;
        if ( i == 2 ) {                 /* one piece of a line, all 'a' but the dl at 1000 that ends field 1 */
            s.fields.headPositions = { 1000 };
            s.headHashes = { run( 1000 ).h };
            s.head = followedBy( followedBy( run( 1000 ), comma ), run( size - 1001 ) );
            s.fields.tailDelims = 1;
            s.fields.tailNonEmpty = true;
            continue;
        }
        s.fields.hasDelimiter = true;
        s.fields.count = lines;
        s.fields.firstNl = 500;
        s.head = run( 500 );
        if ( i == 3 ) {
            s.fields.headPositions = { 100, 200 };
            s.headHashes = { run( 100 ).h, followedBy( followedBy( run( 100 ), comma ), run( 99 ) ).h };
            s.head = followedBy( followedBy( followedBy( followedBy( run( 100 ), comma ), run( 99 ) ), comma ), run( 299 ) );
        }
        s.fields.tailStart = size - 50;        /* "aaaaaaaaaa,aaa..." : one dl 40 bytes in front of the end */
        s.fields.tailDelims = 1;
        s.fields.tailFieldStart = size - 39;
        s.tail = followedBy( followedBy( run( 10 ), comma ), run( 39 ) );
        s.tailStartHash = followedBy( run( 10 ), comma ).h;
        s.fields.tailNonEmpty = true;
    }
    std::vector<std::pair<uint64_t, FieldKey> > patches;
    const auto stitched = stitchFieldHashes( stretches, x, ',', j, [&] ( uint64_t k, const FieldKey& key ) { patches.emplace_back( k, key ); } );
    CHECK( stitched.closed == 3 * lines && stitched.closed > ( uint64_t( 1 ) << 33 ) );
    CHECK( stitched.hasTail && ( stitched.tail.field == FieldSpan{ 4 * size - 39, 39 } ) && stitched.tail.key == run( 39 ).h );
    CHECK( 4 * size - 39 > ( uint64_t( 1 ) << 33 ) );
    CHECK( patches.size() == 2 );
    /* field 1 from the tail of 0 to stretch 1's first nl: 39 + 500 bytes 'a' */
    CHECK( patches[0].first == lines && ( patches[0].second.field == FieldSpan{ size - 39, 39 + 500 } ) );
    CHECK( patches[0].second.key == run( 539 ).h );
    /* field 1 from the tail of 1 to the dl of 2: 39 + 1000 */
    CHECK( patches[1].first == 2 * lines && ( patches[1].second.field == FieldSpan{ 2 * size - 39, 39 + 1000 } ) );
    CHECK( patches[1].second.key == run( 1039 ).h );
    /* field 3: tail of 1 has one dl, stretch 2 one, stretch 3's head two: the third starts it at 3 * size + 101, the
     * fourth ends it, both a whole stretch of 3 GiB behind the line's start */
    for ( auto& stretch : stretches ) {
        stretch.summary.fields.tailFieldStart = FIELD_UNKNOWN;
    }
    patches.clear();
    (void)stitchFieldHashes( stretches, x, ',', 3, [&] ( uint64_t k, const FieldKey& key ) { patches.emplace_back( k, key ); } );
    CHECK( patches.size() == 2 && ( patches[0].second.field == FieldSpan{ size + 500, -1 } ) && patches[0].second.key == FIELD_MISSING );
    CHECK( ( patches[1].second.field == FieldSpan{ 3 * size + 101, 99 } ) && patches[1].second.key == run( 99 ).h );
}
/** layFieldHashes: the regions in their order, each aligned as its loads need, none overlapping the next. */
void
layout()
{
    /* the record sizes and constants that bz2_queries.hip.h pins */
    const QuerySizes sizes{ 16, 16, 16, 256, 24, 21504, 256, 8, 64, 16, 48, 64, 16, 24, 56, 16 };
    for ( const uint64_t nTiles : { uint64_t( 0 ), uint64_t( 1 ), uint64_t( 7 ), uint64_t( 6554 ) } ) {
        for ( const uint64_t n : { uint64_t( 1 ), uint64_t( 3 ), uint64_t( 600 ) } ) {
            for ( const uint64_t field : { uint64_t( 0 ), uint64_t( 2 ), uint64_t( 1023 ) } ) {
                const auto l = layFieldHashes( sizes, nTiles, n, field );
                const uint64_t slots = nTiles * 256, heads = n * ( field + 1 ) * 8;
                const auto up = [] ( uint64_t at, uint64_t alignment ) { return ( at + alignment - 1 ) / alignment * alignment; };
                uint64_t at = 0;
                CHECK( l.tilesAt == at );
                at = up( at + nTiles * 16, 16 );
                CHECK( l.spansAt == at );
                at = up( at + n * 24, 16 );
                CHECK( l.hashSpansAt == at );
                at = up( at + n * 16, 16 );
                CHECK( l.resultsAt == at );
                at = up( at + n * 56, 16 );
                CHECK( l.hashSummariesAt == at );
                at = up( at + n * 48, 16 );
                CHECK( l.tailsAt == at );
                at = up( at + n * 16, 16 );
                CHECK( l.headsAt == at );
                at = up( at + heads, 16 );
                CHECK( l.headHashesAt == at );
                at = up( at + heads, 16 );
                CHECK( l.tileSummariesAt == at );
                at = up( at + nTiles * 16, 16 );
                CHECK( l.hashTilesAt == at );
                at = up( at + nTiles * 64, 16 );
                CHECK( l.placesAt == at );
                at = up( at + slots * 8, 16 );
                CHECK( l.hashPrefixesAt == at );
                at += slots * 16;
                CHECK( l.prefixesAt == at && l.countsAt == at + slots * 4 && l.hashCountsAt == at + slots * 8 );
                CHECK( l.bytes == at + slots * 12 );
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
    longLine();
    refusals();
    beyondEightGiB();
    layout();
    std::puts( "fieldhash cases ok" );
    return 0;
}
