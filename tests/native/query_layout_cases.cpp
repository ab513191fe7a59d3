/* The arithmetic of the query launchers (bz2_query_layout.hpp).  The tiler: for tiles of 16 384 and 65 536 positions and
 * strings of 1, 2 and 256 bytes, over spans around every boundary, beyond 2^32, empty, given twice and none at all, the
 * tiles of a span are in order, disjoint, at most a tile long and cover exactly the positions at which the string can
 * start, and their number is the closed form.  The layouts: every offset and total equals the expression that the
 * launcher computed by hand before there was a layout function -- written out here as it stood --, and the regions that
 * are read or written with 8- and 16-byte accesses start at such multiples.  Prints "query layout ok". */
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_query_layout.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
char currentCase[96] = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 30 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

/* sizeof of the kernels' records and their constants: bz2_queries.hip.h pins the same values */
constexpr QuerySizes SIZES{ 16, 16, 16, 256, 24, 21504, 256, 8, 64, 16, 48, 64, 16, 24, 56, 16 };

struct Span
{
    uint64_t offset, size;
};

void
checkTiles( const std::vector<Span>& spans, uint64_t tile, uint64_t m )
{
    std::vector<uint64_t> covered( spans.size(), 0 ), tilesOf( spans.size(), 0 );
    size_t lastSpan = 0;
    const uint64_t count = forEachTile( spans.data(), spans.size(), tile, m, [&] ( size_t s, uint64_t at, uint64_t length ) {
        CHECK( s < spans.size() && s >= lastSpan );             /* spans in order */
        if ( s >= spans.size() ) return;
        lastSpan = s;
        CHECK( at == covered[s] );                              /* ascending, no gap, no overlap */
        CHECK( length >= 1 && length <= tile );
        CHECK( at % tile == 0 );
        covered[s] += length;
        ++tilesOf[s];
    } );
    uint64_t expected = 0;
    const auto first = firstTiles( spans.data(), spans.size(), tile, m );
    CHECK( first.size() == spans.size() + 1 && first[0] == 0 );
    for ( size_t s = 0; s < spans.size(); ++s ) {
        const uint64_t starts = spans[s].size >= m ? spans[s].size - m + 1 : 0;
        CHECK( covered[s] == starts );                          /* exactly the start positions */
        CHECK( tilesOf[s] == ( starts + tile - 1 ) / tile );
        CHECK( first[s] == expected && first[s + 1] - first[s] == tilesOf[s] );
        expected += ( starts + tile - 1 ) / tile;
    }
    CHECK( count == expected && first.back() == expected );
    CHECK( forEachTile( spans.data(), spans.size(), tile, m, [] ( size_t, uint64_t, uint64_t ) {} ) == expected );
}

uint64_t
aligned( uint64_t at )
{
    return ( at + 15 ) & ~uint64_t( 15 );
}

/* the launchers' arithmetic as it stood in bz2_device.hip, with the sizeofs as numbers */
void
checkLayouts( uint64_t nTiles, uint64_t n, uint64_t k, uint64_t states, uint64_t field, uint64_t nAsked, uint64_t nWork )
{
    std::snprintf( currentCase, sizeof( currentCase ), "%llu tiles, n %llu, k %llu, %llu states, field %llu, %llu asked, %llu work",
                   (unsigned long long)nTiles, (unsigned long long)n, (unsigned long long)k, (unsigned long long)states,
                   (unsigned long long)field, (unsigned long long)nAsked, (unsigned long long)nWork );
    for ( const bool find : { false, true } ) {   /* selectBytes; counting has one result per distinct span, here nWork of them */
        const uint64_t nResults = find ? n : nWork;
        const uint64_t tilesAt = 0, queriesAt = tilesAt + nTiles * 16;
        const uint64_t resultsAt = queriesAt + ( find ? n * 16 : 0 );
        const uint64_t countsAt = resultsAt + nResults * 8, bytes = countsAt + nTiles * 4;
        const SelectLayout l = laySelect( SIZES, nTiles, find ? n : 0, nResults );
        CHECK( l.tilesAt == tilesAt && l.queriesAt == queriesAt && l.resultsAt == resultsAt && l.countsAt == countsAt && l.bytes == bytes );
        CHECK( l.queriesAt % 8 == 0 && l.resultsAt % 8 == 0 && l.countsAt % 4 == 0 );
    }
    {   /* rankBytes */
        const uint64_t tilesAt = 0, workAt = tilesAt + nTiles * 16, endsAt = workAt + nWork * 16;
        const uint64_t resultsAt = endsAt + ( ( nAsked + 1 ) & ~uint64_t( 1 ) ) * 4;
        const uint64_t countsAt = resultsAt + nAsked * 8, bytes = countsAt + nTiles * 4;
        const RankLayout l = layRank( SIZES, nTiles, nWork, nAsked );
        CHECK( l.tilesAt == tilesAt && l.workAt == workAt && l.endsAt == endsAt && l.resultsAt == resultsAt && l.countsAt == countsAt
               && l.bytes == bytes );
        CHECK( l.workAt % 8 == 0 && l.resultsAt % 8 == 0 && l.resultsAt - l.endsAt >= nAsked * 4 );
    }
    {   /* searchBytes */
        const uint64_t patternAt = nTiles * 16, resultsAt = patternAt + 256;
        const uint64_t seamAt = resultsAt + n * 8, countsAt = seamAt + 2 * 256;
        const uint64_t placesAt = countsAt + ( ( nTiles * 4 + 7 ) & ~uint64_t( 7 ) );
        const uint64_t bytes = placesAt + nTiles * 8;
        const SearchLayout l = laySearch( SIZES, nTiles, n );
        CHECK( l.tilesAt == 0 && l.patternAt == patternAt && l.resultsAt == resultsAt && l.seamAt == seamAt && l.countsAt == countsAt
               && l.placesAt == placesAt && l.bytes == bytes );
        CHECK( l.patternAt % 4 == 0 && l.resultsAt % 8 == 0 && l.placesAt % 8 == 0 );
    }
    {   /* searchBytesSet */
        const uint64_t imageAt = ( nTiles * 24 + 15 ) & ~uint64_t( 15 ), resultsAt = imageAt + 21504;
        const uint64_t eachAt = resultsAt + n * 8, seamAt = eachAt + k * 8;
        const uint64_t countsAt = seamAt + 2 * 256;
        const uint64_t placesAt = countsAt + ( ( nTiles * 4 + 7 ) & ~uint64_t( 7 ) );
        const uint64_t bytes = placesAt + nTiles * 8;
        const SearchSetLayout l = laySearchSet( SIZES, nTiles, n, k );
        CHECK( l.tilesAt == 0 && l.imageAt == imageAt && l.resultsAt == resultsAt && l.eachAt == eachAt && l.seamAt == seamAt
               && l.countsAt == countsAt && l.placesAt == placesAt && l.bytes == bytes );
        CHECK( l.imageAt % 16 == 0 && l.resultsAt % 8 == 0 && l.eachAt % 8 == 0 && l.placesAt % 8 == 0 );
    }
    {   /* matchLines */
        const uint64_t slots = nTiles * 256, stride = ( states + 15 ) & ~uint64_t( 15 );
        const uint64_t spansAt = nTiles * 16, tableAt = aligned( spansAt + n * 8 );
        const uint64_t acceptsAt = tableAt + states * 256, resultsAt = aligned( acceptsAt + 64 );
        const uint64_t spanInfoAt = resultsAt + n * 64, spanCountsAt = aligned( spanInfoAt + n * 4 );
        const uint64_t mapsAt = aligned( spanCountsAt + n * 8 ), infoAt = mapsAt + slots * stride;
        const uint64_t countsAt = infoAt + slots * 4, placesAt = aligned( countsAt + slots * 4 );
        const uint64_t bytes = placesAt + slots * 8;
        const RegexLayout l = layRegex( SIZES, nTiles, n, states );
        CHECK( l.tilesAt == 0 && l.spansAt == spansAt && l.tableAt == tableAt && l.acceptsAt == acceptsAt && l.resultsAt == resultsAt );
        CHECK( l.spanInfoAt == spanInfoAt && l.spanCountsAt == spanCountsAt && l.mapsAt == mapsAt && l.infoAt == infoAt );
        CHECK( l.countsAt == countsAt && l.placesAt == placesAt && l.bytes == bytes );
        CHECK( l.tableAt % 16 == 0 && l.acceptsAt % 16 == 0 && l.resultsAt % 16 == 0 && l.spanCountsAt % 16 == 0 && l.mapsAt % 16 == 0
               && l.placesAt % 16 == 0 && l.spansAt % 8 == 0 );
    }
    {   /* hashLines */
        const uint64_t slots = nTiles * 256;
        const uint64_t spansAt = aligned( nTiles * 16 ), resultsAt = aligned( spansAt + n * 16 );
        const uint64_t tilesAt = aligned( resultsAt + n * 48 );
        const uint64_t prefixesAt = aligned( tilesAt + nTiles * 64 );
        const uint64_t placesAt = prefixesAt + slots * 16, countsAt = placesAt + slots * 8;
        const uint64_t bytes = countsAt + slots * 4;
        const LineHashLayout l = layLineHash( SIZES, nTiles, n );
        CHECK( l.tilesAt == 0 && l.spansAt == spansAt && l.resultsAt == resultsAt && l.tileSummariesAt == tilesAt
               && l.prefixesAt == prefixesAt && l.placesAt == placesAt && l.countsAt == countsAt && l.bytes == bytes );
        CHECK( l.spansAt % 16 == 0 && l.resultsAt % 16 == 0 && l.tileSummariesAt % 16 == 0 && l.prefixesAt % 16 == 0 && l.placesAt % 8 == 0 );
    }
    {   /* fieldSpans */
        const uint64_t slots = nTiles * 256, cap = field + 1;
        const uint64_t spansAt = aligned( nTiles * 16 ), resultsAt = aligned( spansAt + n * 24 );
        const uint64_t headsAt = aligned( resultsAt + n * 56 );
        const uint64_t tilesAt = aligned( headsAt + n * cap * 8 );
        const uint64_t placesAt = aligned( tilesAt + nTiles * 16 );
        const uint64_t prefixesAt = placesAt + slots * 8, countsAt = prefixesAt + slots * 4;
        const uint64_t bytes = countsAt + slots * 4;
        const FieldLayout l = layFields( SIZES, nTiles, n, field );
        CHECK( l.tilesAt == 0 && l.spansAt == spansAt && l.resultsAt == resultsAt && l.headsAt == headsAt && l.tileSummariesAt == tilesAt
               && l.placesAt == placesAt && l.prefixesAt == prefixesAt && l.countsAt == countsAt && l.bytes == bytes );
        CHECK( l.spansAt % 16 == 0 && l.resultsAt % 16 == 0 && l.headsAt % 16 == 0 && l.tileSummariesAt % 16 == 0 && l.placesAt % 16 == 0 );
    }
}
}  // namespace

int
main()
{
    int tilerCases = 0;
    for ( const uint64_t tile : { uint64_t( 16384 ), uint64_t( 65536 ) } ) {
        for ( const uint64_t m : { uint64_t( 1 ), uint64_t( 2 ), uint64_t( 256 ) } ) {
            const uint64_t sizes[] = { 0, m - 1, m, m + 1, tile + m - 2, tile + m - 1, tile + m, 3 * tile + 13 };
            for ( const uint64_t size : sizes ) {
                std::snprintf( currentCase, sizeof( currentCase ), "tile %llu, m %llu, size %llu", (unsigned long long)tile,
                               (unsigned long long)m, (unsigned long long)size );
                checkTiles( { { 12345, size } }, tile, m );
                checkTiles( { { ( uint64_t( 5 ) << 32 ) + 7, size } }, tile, m );
                ++tilerCases;
            }
            /* all of them in one call, beyond 2^32, with empty spans between the others and one span given twice */
            std::snprintf( currentCase, sizeof( currentCase ), "tile %llu, m %llu, all sizes", (unsigned long long)tile, (unsigned long long)m );
            std::vector<Span> all;
            uint64_t at = ( uint64_t( 1 ) << 32 ) - 100;
            for ( const uint64_t size : sizes ) {
                all.push_back( { at, size } );
                all.push_back( { at + size, 0 } );
                at += size + 3;
            }
            all.push_back( all[12] );
            all.push_back( all[12] );
            checkTiles( all, tile, m );
            checkTiles( {}, tile, m );
            CHECK( forEachTile( static_cast<const Span*>( nullptr ), 0, tile, m, [] ( size_t, uint64_t, uint64_t ) { CHECK( false ); } ) == 0 );
            tilerCases += 2;
        }
    }
    {   /* what a tile carries: its place in the span, so that offset + place stays exact beyond 2^32 */
        std::snprintf( currentCase, sizeof( currentCase ), "places" );
        const Span span{ ( uint64_t( 3 ) << 32 ) + 1, 2 * 65536 + 5 };
        std::vector<uint64_t> places;
        forEachTile( &span, 1, 65536, 1, [&] ( size_t, uint64_t place, uint64_t ) { places.push_back( span.offset + place ); } );
        CHECK( places == ( std::vector<uint64_t>{ span.offset, span.offset + 65536, span.offset + 131072 } ) );
    }
    {
        std::snprintf( currentCase, sizeof( currentCase ), "Regions" );
        Regions r;
        CHECK( r.size() == 0 && r.add( 0 ) == 0 && r.add( 5 ) == 0 && r.add( 3, 16 ) == 16 && r.size() == 19 && r.add( 0, 8 ) == 24 );
        CHECK( r.size() == 24 && r.add( 1, 8 ) == 24 && r.add( 1 ) == 25 && r.size() == 26 );
    }
    int layoutCases = 0;
    for ( const uint64_t nTiles : { 0, 1, 2, 3, 255, 257 } ) {
        for ( const uint64_t n : { 1, 2, 3, 5 } ) {
            for ( const uint64_t k : { 1, 3, 1024 } ) {
                for ( const uint64_t states : { 2, 17, 64 } ) {
                    for ( const uint64_t field : { 0, 1, 1023 } ) {
                        for ( const uint64_t nAsked : { 1, 2, 7, 1000 } ) {
                            checkLayouts( nTiles, n, k, states, field, nAsked, std::min<uint64_t>( nAsked, nTiles + 1 ) );
                            ++layoutCases;
                        }
                    }
                }
            }
        }
    }
    if ( failures != 0 ) {
        std::printf( "%d failures\n", failures );
        return 1;
    }
    std::printf( "query layout ok (%d tiler cases, %d layout cases)\n", tilerCases, layoutCases );
    return 0;
}
