/**
 * bz2_queries.hip.h -- the host side of the calls that read a finished batch's output: gather, count / find / rank of a
 * byte, search for a string or a set of strings, regular expressions, line hashes, field spans, field columns, field
 * hashes, field numbers, field matches and field matches by a regular expression, their mi355x::*Output forms for the
 * reader and their extern "C" entry points.  Part of bz2_device.hip's
 * translation unit (the context's layout names device record types), included below the context's definition and HIP_TRY.
 *
 * Every launcher but gatherPieces (millions of one-tile pieces, a plain loop) has the same shape: refuseQuery, the tiles
 * of its spans (firstTiles / writeCountTiles), its layout (bz2_query_layout.hpp) and growStaging, one H2D of what goes
 * up, its kernels, one D2H of what comes down and, for the calls that list what they counted, emitListed.
 */
#pragma once

#include <numeric>

#include "bz2_query_layout.hpp"

namespace
{
/* the records and constants that the layouts are given: tests/native/query_layout_cases.cpp uses these values */
constexpr QuerySizes QUERY_SIZES{ sizeof( CountTile ), sizeof( FindQuery ), sizeof( RankTile ), SEARCH_MAX_PATTERN, sizeof( SetTile ),
                                  SET_IMAGE_BYTES, REGEX_THREADS, sizeof( RegexSpan ), REGEX_STATES,
                                  sizeof( LineHashSpan ), sizeof( LineHashSpanSummary ), sizeof( LineHashTile ), sizeof( ulonglong2 ),
                                  sizeof( FieldSpanTiles ), sizeof( FieldSpanSummary ), sizeof( FieldTile ) };
static_assert( sizeof( CountTile ) == 16 && sizeof( FindQuery ) == 16 && sizeof( RankTile ) == 16 );
static_assert( SEARCH_MAX_PATTERN == 256 && sizeof( SetTile ) == 24 && SET_IMAGE_BYTES == 21504 );
static_assert( REGEX_THREADS == 256 && LINEHASH_THREADS == 256 && FIELD_THREADS == 256, "chunksPerTile" );
static_assert( sizeof( RegexSpan ) == 8 && REGEX_STATES == 64 && regexMapStride( 17 ) == 32 );
static_assert( sizeof( LineHashSpan ) == 16 && sizeof( LineHashSpanSummary ) == 48 && sizeof( LineHashTile ) == 64 );
static_assert( sizeof( ulonglong2 ) == 16 );
static_assert( sizeof( FieldSpanTiles ) == 24 && sizeof( FieldSpanSummary ) == 56 && sizeof( FieldTile ) == 16 );

/** lastError = "<what>: <why>"; the status of a call that refuses its arguments. */
int
refuse( mi355x_bz2_ctx* c, const char* what, const std::string& why )
{
    c->lastError = std::string( what ) + ": " + why;
    return MI355X_BZ2_ERR_INVALID_ARGUMENT;
}

bool
outside( const mi355x_bz2_ctx* c, uint64_t offset, uint64_t size )
{
    return size > c->outSize || offset > c->outSize - size;
}

/**
 * The refusals a query begins with, in the order in which they win: a batch in flight; `argumentError`, what the caller
 * found wrong with its other arguments (empty: nothing); the first i of n for which bad( i ) holds: "<item> i <fault>".
 * The caller holds the context's mutex.
 */
template<typename Bad>
int
refuseQuery( mi355x_bz2_ctx* c, const char* what, uint32_t n, Bad bad, const std::string& argumentError = {},
             const char* item = "span", const char* fault = "lies outside the last batch's output" )
{
    if ( c->pendingBlocks != 0 ) return refuse( c, what, "a batch is in flight" );
    if ( !argumentError.empty() ) return refuse( c, what, argumentError );
    for ( uint32_t i = 0; i < n; ++i ) {
        if ( bad( i ) ) return refuse( c, what, std::string( item ) + " " + std::to_string( i ) + " " + fault );
    }
    return MI355X_BZ2_OK;
}

/** refuseQuery for plain spans; counts[i], if given, is zeroed as span i passes. */
int
refuseQuery( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, uint32_t n,
             const std::string& argumentError = {}, uint64_t* counts = nullptr )
{
    return refuseQuery( c, what, n, [c, spans, counts] ( uint32_t i ) {
        if ( outside( c, spans[i].offset, spans[i].size ) ) return true;
        if ( counts != nullptr ) counts[i] = 0;
        return false;
    }, argumentError );
}

/** Room for a call's lists in its page-locked and its device buffer (GrowBuffer::grow, each with its own need and new
 * capacity).  The previous call's lists have been consumed: every call waits for its kernels. */
int
growStaging( mi355x_bz2_ctx* c, GrowBuffer& host, GrowBuffer& device, uint64_t hostNeed, uint64_t hostCapacity, uint64_t deviceNeed,
             uint64_t deviceCapacity )
{
    HIP_TRY( c, host.grow( c, hostNeed, hostCapacity, hostCapacity ) );
    HIP_TRY( c, device.grow( c, deviceNeed, deviceCapacity, deviceCapacity ) );
    return MI355X_BZ2_OK;
}

/** The capacity of most of them: twice the present one, or the need if that is more. */
uint64_t
doubled( const GrowBuffer& buffer, uint64_t need )
{
    return std::max( 2 * buffer.capacity, need );
}

/** growStaging for the three per-line calls: hSearch and dSearch each double on their own need. */
int
growLineStaging( mi355x_bz2_ctx* c, uint64_t hostNeed, uint64_t deviceNeed )
{
    return growStaging( c, c->hSearch, c->dSearch, hostNeed, doubled( c->hSearch, hostNeed ), deviceNeed,
                        doubled( c->dSearch, deviceNeed ) );
}

template<typename T>
T*
at( uint8_t* buffer, uint64_t offset )
{
    return reinterpret_cast<T*>( buffer + offset );
}

/** The CountTiles of forEachTile( spans, n, tileBytes, m ) to tiles[0, ...). */
void
writeCountTiles( CountTile* tiles, const mi355x_bz2_byte_span* spans, size_t n, uint64_t tileBytes, uint64_t m )
{
    forEachTile( spans, n, tileBytes, m, [&tiles, spans] ( size_t s, uint64_t k, uint64_t length ) {
        *tiles++ = { spans[s].offset + k, (uint32_t)length, (uint32_t)s };
    } );
}

/** The distinct spans among those that `spanAt` names, in the order of their first mention, and for each of the n the
 * one it is: a span named several times is counted once. */
template<typename SpanAt>
std::vector<mi355x_bz2_byte_span>
distinctSpans( uint32_t n, SpanAt spanAt, std::vector<uint32_t>* spanOf )
{
    std::map<std::pair<uint64_t, uint64_t>, uint32_t> known;
    std::vector<mi355x_bz2_byte_span> spans;
    spanOf->resize( n );
    for ( uint32_t i = 0; i < n; ++i ) {
        const mi355x_bz2_byte_span span = spanAt( i );
        const auto [entry, isNew] = known.emplace( std::make_pair( span.offset, span.size ), (uint32_t)spans.size() );
        ( *spanOf )[i] = entry->second;
        if ( isNew ) spans.push_back( span );
    }
    return spans;
}

constexpr const char* SEAM_OUTSIDE = "the seam span lies outside the last batch's output";

/** The seam bytes of a search, which come back with its counts: k_seam_bytes puts the first and the last seamN bytes of
 * `seam` at dSeam[0, ...) and dSeam[SEARCH_MAX_PATTERN, ...); copySeam hands them over behind the D2H. */
int
launchSeam( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* seam, uint32_t seamN, uint8_t* dSeam )
{
    if ( seamN == 0 ) return MI355X_BZ2_OK;
    hipLaunchKernelGGL( k_seam_bytes, dim3( 1 ), dim3( 2 * SEARCH_MAX_PATTERN ), 0, c->stream, c->dOut, seam->offset, seam->size,
                        seamN, dSeam );
    HIP_TRY( c, hipGetLastError() );
    return MI355X_BZ2_OK;
}

void
copySeam( const uint8_t* hSeam, uint32_t seamN, uint8_t* seamBytes )
{
    if ( seamN == 0 ) return;   /* seamBytes may be nullptr then */
    std::memcpy( seamBytes, hSeam, seamN );
    std::memcpy( seamBytes + SEARCH_MAX_PATTERN, hSeam + SEARCH_MAX_PATTERN, seamN );
}

/** Where a listing call's positions go -- and, for pairs, the ids behind them: the caller's arrays, or vectors that are
 * resized to their number. */
struct Listed
{
    uint64_t* positions{ nullptr };
    std::vector<uint64_t>* grown{ nullptr };
    uint32_t* ids{ nullptr };
    std::vector<uint32_t>* grownIds{ nullptr };
};

/**
 * The second pass of a call that lists what its first pass counted: min( total, capacity ) of them are made room for,
 * on the host (in the vectors, if given) and in dSearchPositions -- a failure to allocate fails the call --,
 * k_scan_tiles turns dCounts[0, nCounts) into places at dPlaces, emit( wanted, dPositions, dIds ) launches the call's
 * emit kernel, and a D2H brings the positions (and ids) to their place.  Nothing at all with nothing wanted.
 */
template<typename Emit>
int
emitListed( mi355x_bz2_ctx* c, const char* what, uint64_t total, uint64_t capacity, Listed to, const uint32_t* dCounts,
            uint64_t nCounts, uint64_t* dPlaces, Emit emit )
{
    const uint64_t wanted = std::min( total, capacity );
    if ( wanted == 0 ) return MI355X_BZ2_OK;
    const bool pairs = to.ids != nullptr || to.grownIds != nullptr;
    if ( to.grown != nullptr ) {
        try {
            to.grown->resize( wanted );
            if ( pairs ) to.grownIds->resize( wanted );
        } catch ( const std::exception& ) {
            c->lastError = std::string( what ) + ": no host memory for " + std::to_string( wanted ) + ( pairs ? " pairs" : " positions" );
            return MI355X_BZ2_ERR_DEVICE;
        }
        to.positions = to.grown->data();
        if ( pairs ) to.ids = to.grownIds->data();
    }
    /* the positions, then the ids */
    const uint64_t idsAt = wanted * sizeof( uint64_t ), need = idsAt + ( pairs ? wanted * sizeof( uint32_t ) : 0 );
    HIP_TRY( c, c->dSearchPositions.grow( c, need, need + need / 4, need ) );
    auto* const dPositions = at<uint64_t>( c->dSearchPositions.bytes, 0 );
    auto* const dIds = at<uint32_t>( c->dSearchPositions.bytes, idsAt );
    hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)nCounts, dPlaces );
    HIP_TRY( c, hipGetLastError() );
    emit( wanted, dPositions, dIds );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( to.positions, dPositions, idsAt, hipMemcpyDeviceToHost, c->stream ) );
    if ( pairs ) HIP_TRY( c, hipMemcpyAsync( to.ids, dIds, wanted * sizeof( uint32_t ), hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    return MI355X_BZ2_OK;
}

/** k_gather over pieces of the `srcSize` bytes at `src` (device memory of the context), see mi355x_bz2_gather_output.
 * The caller holds the context's lock. */
int
gatherPieces( mi355x_bz2_ctx* c, const uint8_t* src, uint64_t srcSize, const mi355x_bz2_gather_piece* pieces,
              uint32_t nPieces, void* dst, int dstIsDevice )
{
    /* every piece inside the source; tiles of at most GATHER_TILE bytes */
    uint64_t nTiles = 0, total = 0;
    for ( uint32_t i = 0; i < nPieces; ++i ) {
        const auto& p = pieces[i];
        if ( p.size > srcSize || p.src_offset > srcSize - p.size || p.dst_offset > ~uint64_t( 0 ) - p.size ) {
            c->lastError = "gather_output: piece " + std::to_string( i ) + " lies outside the last batch's output";
            return MI355X_BZ2_ERR_INVALID_ARGUMENT;
        }
        nTiles += ( p.size + GATHER_TILE - 1 ) / GATHER_TILE;
        total += p.size;
    }
    if ( total == 0 ) return MI355X_BZ2_OK;
    if ( dst == nullptr || nTiles > 0x7FFFFFFFu ) {
        c->lastError = "gather_output: no destination, or too many pieces";
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    HIP_TRY( c, hipSetDevice( c->device ) );
    /* the previous call's tile list has been consumed (every call waits for its kernel) */
    const uint64_t tileBytes = nTiles * sizeof( GatherTile ), tileCap = std::max( 2 * c->dGatherTiles.capacity, tileBytes );
    HIP_TRY( c, c->hGatherTiles.grow( c, tileBytes, tileCap, tileCap ) );
    HIP_TRY( c, c->dGatherTiles.grow( c, tileBytes, tileCap, tileCap ) );
    const bool toHost = dstIsDevice == 0;
    if ( toHost ) {
        const uint64_t cap = std::max( c->dGatherStage.capacity + c->dGatherStage.capacity / 2, total );
        HIP_TRY( c, c->hGatherStage.grow( c, total, cap, cap ) );
        HIP_TRY( c, c->dGatherStage.grow( c, total, cap, cap ) );
    }
    GatherTile* const hTiles = reinterpret_cast<GatherTile*>( c->hGatherTiles.bytes );
    GatherTile* const dTiles = reinterpret_cast<GatherTile*>( c->dGatherTiles.bytes );
    /* a host destination gets the pieces packed back to back in the staging buffer, one D2H copy of exactly the requested
     * bytes, and then each piece copied to its place: bytes of `dst` between the pieces are never written */
    uint64_t tile = 0, staged = 0;
    for ( uint32_t i = 0; i < nPieces; ++i ) {
        const auto& p = pieces[i];
        const uint64_t at = toHost ? staged : p.dst_offset;
        for ( uint64_t k = 0; k < p.size; k += GATHER_TILE ) {
            hTiles[tile++] = { p.src_offset + k, at + k, std::min<uint64_t>( GATHER_TILE, p.size - k ) };
        }
        staged += p.size;
    }
    HIP_TRY( c, hipMemcpyAsync( dTiles, hTiles, tileBytes, hipMemcpyHostToDevice, c->stream ) );
    hipLaunchKernelGGL( k_gather, dim3( (uint32_t)nTiles ), dim3( GATHER_THREADS ), 0, c->stream, dTiles, src,
                        toHost ? c->dGatherStage.bytes : static_cast<uint8_t*>( dst ) );
    HIP_TRY( c, hipGetLastError() );
    if ( toHost ) {
        HIP_TRY( c, hipMemcpyAsync( c->hGatherStage.bytes, c->dGatherStage.bytes, total, hipMemcpyDeviceToHost, c->stream ) );
    }
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    if ( toHost ) {
        staged = 0;
        for ( uint32_t i = 0; i < nPieces; ++i ) {
            std::memcpy( static_cast<uint8_t*>( dst ) + pieces[i].dst_offset, c->hGatherStage.bytes + staged, pieces[i].size );
            staged += pieces[i].size;
        }
    }
    return MI355X_BZ2_OK;
}

/**
 * Both byte calls: the distinct spans are cut into tiles, k_count_byte counts every tile, and either the spans' sums or
 * (ranks given) the positions k_find_byte finds come back.
 */
int
selectBytes( mi355x_bz2_ctx* c, const char* what, uint8_t value, uint32_t n, const mi355x_bz2_byte_span* asked,
             const uint64_t* ranks, uint64_t* results )
{
    const std::scoped_lock lock( c->mutex );
    const bool find = ranks != nullptr;
    const int refused = refuseQuery( c, what, n, [&] ( uint32_t i ) {
        return outside( c, asked[i].offset, asked[i].size ) || ( find && ranks[i] == 0 );
    }, {}, "span", "lies outside the last batch's output, or its rank is 0" );
    if ( refused != MI355X_BZ2_OK ) return refused;
    std::vector<uint32_t> spanOf;
    const auto spans = distinctSpans( n, [asked] ( uint32_t i ) { return asked[i]; }, &spanOf );
    const auto firstTile = firstTiles( spans.data(), spans.size(), COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back();
    for ( uint32_t i = 0; i < n; ++i ) results[i] = find ? FIND_NONE : 0;
    if ( nTiles == 0 ) return MI355X_BZ2_OK;
    if ( nTiles > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const uint64_t nResults = find ? n : spans.size();
    const SelectLayout l = laySelect( QUERY_SIZES, nTiles, find ? n : 0, nResults );
    const uint64_t cap = doubled( c->dSelect, l.bytes );
    if ( const int status = growStaging( c, c->hSelect, c->dSelect, l.countsAt, cap, l.bytes, cap ) ) return status;
    uint8_t* const h = c->hSelect.bytes;
    uint8_t* const d = c->dSelect.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans.data(), spans.size(), COUNT_TILE, 1 );
    for ( uint32_t i = 0; find && i < n; ++i ) {
        const uint64_t* const first = &firstTile[spanOf[i]];
        at<FindQuery>( h, l.queriesAt )[i] = { ranks[i], (uint32_t)first[0], (uint32_t)( first[1] - first[0] ) };
    }
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( !find ) HIP_TRY( c, hipMemsetAsync( d + l.resultsAt, 0, nResults * sizeof( uint64_t ), c->stream ) );
    const uint32_t pattern = 0x01010101u * value;
    hipLaunchKernelGGL( k_count_byte, dim3( (uint32_t)nTiles ), dim3( COUNT_THREADS ), 0, c->stream,
                        at<const CountTile>( d, l.tilesAt ), c->dOut, pattern, at<uint32_t>( d, l.countsAt ),
                        find ? nullptr : at<unsigned long long>( d, l.resultsAt ) );
    HIP_TRY( c, hipGetLastError() );
    if ( find ) {
        hipLaunchKernelGGL( k_find_byte, dim3( n ), dim3( FIND_THREADS ), 0, c->stream, at<const FindQuery>( d, l.queriesAt ),
                            at<const CountTile>( d, l.tilesAt ), at<const uint32_t>( d, l.countsAt ), c->dOut, pattern,
                            at<uint64_t>( d, l.resultsAt ) );
        HIP_TRY( c, hipGetLastError() );
    }
    const auto* const hResults = at<uint64_t>( h, l.resultsAt );
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, nResults * sizeof( uint64_t ), hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( uint32_t i = 0; i < n; ++i ) results[i] = find ? hResults[i] : hResults[spanOf[i]];
    return MI355X_BZ2_OK;
}

/**
 * mi355x_bz2_rank_byte: the distinct spans are cut into tiles and counted as in selectBytes; the positions are sorted
 * span by span and grouped by tile, and k_rank_byte runs one wave per tile that holds a position.  A position at a
 * span's first byte is answered here (0); a position at a tile's first byte is the end of the tile in front of it, so
 * that a position at the span's end needs no tile behind the span.
 */
constexpr uint64_t RANK_LIST_DOUBLING = 64ull << 20;

int
rankBytes( mi355x_bz2_ctx* c, const mi355x_bz2_rank_query* queries, uint32_t n, uint8_t value, uint64_t* ranks )
{
    const std::scoped_lock lock( c->mutex );
    /* nothing is written before every query has passed */
    const int refused = refuseQuery( c, "rank_byte", n, [&] ( uint32_t i ) {
        const auto& q = queries[i];
        return outside( c, q.offset, q.size ) || q.position < q.offset || q.position - q.offset > q.size;
    }, {}, "query", "names a span outside the last batch's output, or a position outside its span" );
    if ( refused != MI355X_BZ2_OK ) return refused;
    std::vector<uint32_t> spanOf;
    const auto spanAt = [queries] ( uint32_t i ) { return mi355x_bz2_byte_span{ queries[i].offset, queries[i].size }; };
    const auto spans = distinctSpans( n, spanAt, &spanOf );
    const auto firstTile = firstTiles( spans.data(), spans.size(), COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back();
    struct Asked { uint64_t tile; uint32_t end, input; };   /* tile in the list, bytes of it in front of the position */
    std::vector<Asked> asked;
    asked.reserve( n );
    for ( uint32_t i = 0; i < n; ++i ) {
        ranks[i] = 0;
        const uint64_t in = queries[i].position - queries[i].offset;
        if ( in == 0 ) continue;
        asked.push_back( { firstTile[spanOf[i]] + ( in - 1 ) / COUNT_TILE, (uint32_t)( ( in - 1 ) % COUNT_TILE ) + 1, i } );
    }
    if ( asked.empty() ) return MI355X_BZ2_OK;
    if ( nTiles > 0x7FFFFFFFu ) return refuse( c, "rank_byte", "too many spans" );
    std::sort( asked.begin(), asked.end(), [] ( const Asked& a, const Asked& b ) {
        return a.tile != b.tile ? a.tile < b.tile : a.end < b.end;
    } );
    uint64_t nWork = 0;
    for ( size_t k = 0; k < asked.size(); ++k ) nWork += k == 0 || asked[k].tile != asked[k - 1].tile ? 1 : 0;
    HIP_TRY( c, hipSetDevice( c->device ) );

    const uint64_t nAsked = asked.size();
    const RankLayout l = layRank( QUERY_SIZES, nTiles, nWork, nAsked );
    /* the lists of this call can be orders of magnitude larger than the other byte calls' (12 bytes per position, and a
     * search hands over millions): a need of up to RANK_LIST_DOUBLING doubles the device buffer as the other calls do, a
     * larger one gets the need and an eighth.  One capacity for both buffers, derived from the device's, which holds
     * all the host's holds and the tile counts */
    const uint64_t cap = l.bytes <= RANK_LIST_DOUBLING ? doubled( c->dSelect, l.bytes ) : l.bytes + l.bytes / 8;
    if ( const int status = growStaging( c, c->hSelect, c->dSelect, l.countsAt, cap, l.bytes, cap ) ) return status;
    uint8_t* const h = c->hSelect.bytes;
    uint8_t* const d = c->dSelect.bytes;
    auto* const hTiles = at<CountTile>( h, l.tilesAt );
    auto* const hWork = at<RankTile>( h, l.workAt );
    auto* const hEnds = at<uint32_t>( h, l.endsAt );
    writeCountTiles( hTiles, spans.data(), spans.size(), COUNT_TILE, 1 );
    uint64_t work = 0;
    for ( size_t k = 0; k < asked.size(); ++k ) {
        if ( k == 0 || asked[k].tile != asked[k - 1].tile ) {
            hWork[work++] = { (uint32_t)asked[k].tile, (uint32_t)firstTile[hTiles[asked[k].tile].span], (uint32_t)k, 0 };
        }
        ++hWork[work - 1].nQueries;
        hEnds[k] = asked[k].end;
    }
    if ( ( nAsked & 1 ) != 0 ) hEnds[nAsked] = 0;
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    const uint32_t pattern = 0x01010101u * value;
    hipLaunchKernelGGL( k_count_byte, dim3( (uint32_t)nTiles ), dim3( COUNT_THREADS ), 0, c->stream,
                        at<const CountTile>( d, l.tilesAt ), c->dOut, pattern, at<uint32_t>( d, l.countsAt ), nullptr );
    HIP_TRY( c, hipGetLastError() );
    hipLaunchKernelGGL( k_rank_byte, dim3( (uint32_t)nWork ), dim3( FIND_THREADS ), 0, c->stream, at<const RankTile>( d, l.workAt ),
                        at<const CountTile>( d, l.tilesAt ), at<const uint32_t>( d, l.countsAt ), at<const uint32_t>( d, l.endsAt ),
                        c->dOut, pattern, at<uint64_t>( d, l.resultsAt ) );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, nAsked * sizeof( uint64_t ), hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( size_t k = 0; k < asked.size(); ++k ) ranks[asked[k].input] = at<uint64_t>( h, l.resultsAt )[k];
    return MI355X_BZ2_OK;
}

static_assert( SEARCH_IGNORE_CASE == MI355X_BZ2_SEARCH_IGNORE_CASE, "the planner's flag is the C ABI's" );

/** True, with lastError set, if `flags` has a bit that no search knows.  The caller holds the context's mutex. */
bool
unknownSearchFlags( mi355x_bz2_ctx* c, const char* what, uint32_t flags )
{
    if ( ( flags & ~SEARCH_KNOWN_FLAGS ) == 0 ) return false;
    char bits[16];
    std::snprintf( bits, sizeof( bits ), "0x%X", flags & ~SEARCH_KNOWN_FLAGS );
    refuse( c, what, std::string( "unknown flag bits " ) + bits );
    return true;
}

/**
 * Both string calls.  The start positions every span allows are cut into tiles (spans in caller order, a span given twice
 * is searched twice: its positions are wanted twice), k_count_bytes counts every tile and adds to its span's counter, and
 * the counts -- with the seam bytes of `seam`, if given -- come back in one D2H.  With capacity > 0, emitListed and
 * k_emit_bytes bring the positions to `positions`, or to `grown` resized to their number.  With
 * MI355X_BZ2_SEARCH_IGNORE_CASE in `flags` the pattern is uploaded under foldAscii and the folding instantiations of the
 * two kernels run; the seam bytes come back raw.
 */
int
searchBytes( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
             uint32_t m, uint32_t flags, uint64_t capacity, uint64_t* positions, std::vector<uint64_t>* grown, uint64_t* counts,
             const mi355x_bz2_byte_span* seam, uint8_t* seamBytes )
{
    const std::scoped_lock lock( c->mutex );
    if ( unknownSearchFlags( c, what, flags ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    const bool fold = ( flags & SEARCH_IGNORE_CASE ) != 0;
    const bool patternFits = m >= 1 && m <= SEARCH_MAX_PATTERN;
    const std::string patternError = patternFits ? "" : "the pattern must have 1 to " + std::to_string( SEARCH_MAX_PATTERN ) + " bytes";
    const int refused = refuseQuery( c, what, spans, n, patternError, counts );
    if ( refused != MI355X_BZ2_OK ) return refused;
    if ( seam != nullptr && outside( c, seam->offset, seam->size ) ) return refuse( c, what, SEAM_OUTSIDE );
    const uint32_t seamN = seam != nullptr ? seamLength( m, seam->size ) : 0u;
    if ( grown != nullptr ) grown->clear();
    const uint64_t nTiles = forEachTile( spans, n, SEARCH_TILE, m, [] ( size_t, uint64_t, uint64_t ) {} );
    if ( nTiles == 0 && seamN == 0 ) return MI355X_BZ2_OK;
    if ( nTiles > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const SearchLayout l = laySearch( QUERY_SIZES, nTiles, n );
    const uint64_t cap = doubled( c->dSearch, l.bytes );
    if ( const int status = growStaging( c, c->hSearch, c->dSearch, l.countsAt, cap, l.bytes, cap ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, SEARCH_TILE, m );
    std::memset( h + l.patternAt, 0, SEARCH_MAX_PATTERN );
    for ( uint32_t j = 0; j < m; ++j ) h[l.patternAt + j] = fold ? foldAscii( pattern[j] ) : pattern[j];
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    auto* const dTileCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    HIP_TRY( c, hipMemsetAsync( d + l.resultsAt, 0, l.countsAt - l.resultsAt, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( fold ? k_count_bytes<true> : k_count_bytes<false>, dim3( (uint32_t)nTiles ), dim3( SEARCH_THREADS ),
                            0, c->stream, dTiles, c->dOut, d + l.patternAt, m, dTileCounts, at<unsigned long long>( d, l.resultsAt ) );
        HIP_TRY( c, hipGetLastError() );
    }
    if ( const int status = launchSeam( c, seam, seamN, d + l.seamAt ) ) return status;
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.countsAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    std::copy_n( at<const uint64_t>( h, l.resultsAt ), n, counts );
    copySeam( h + l.seamAt, seamN, seamBytes );
    return emitListed( c, what, std::accumulate( counts, counts + n, uint64_t( 0 ) ), capacity, { positions, grown }, dTileCounts, nTiles,
                       at<uint64_t>( d, l.placesAt ), [&] ( uint64_t wanted, uint64_t* dPositions, uint32_t* ) {
        hipLaunchKernelGGL( fold ? k_emit_bytes<true> : k_emit_bytes<false>, dim3( (uint32_t)nTiles ), dim3( SEARCH_THREADS ), 0,
                            c->stream, dTiles, c->dOut, d + l.patternAt, m, at<uint64_t>( d, l.placesAt ), wanted, dPositions );
    } );
}

/**
 * Both set calls: searchBytes for a set of patterns.  The start positions every span allows for the shortest pattern are
 * cut into tiles that carry their span's end, k_count_set counts the pairs of every tile, of every span and of every
 * pattern, and the counts -- with the seam bytes of `seam`, if given: min( m_max - 1, size ) each -- come back in one
 * D2H.  With capacity > 0, emitListed and k_emit_set bring the positions and ids to `to`.  perPattern (may be null)
 * receives the count of every pattern over all spans.  A set made with fold gets its image under foldAscii and the
 * folding instantiations of the two kernels.
 */
int
searchBytesSet( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, uint32_t n, const PatternSet& set,
                uint64_t capacity, Listed to, uint64_t* counts, uint64_t* perPattern, const mi355x_bz2_byte_span* seam,
                uint8_t* seamBytes )
{
    const std::scoped_lock lock( c->mutex );
    if ( const int status = refuseQuery( c, what, spans, n, {}, counts ) ) return status;
    if ( seam != nullptr && outside( c, seam->offset, seam->size ) ) return refuse( c, what, SEAM_OUTSIDE );
    const uint32_t seamN = seam != nullptr ? seamLength( set.mMax, seam->size ) : 0u;
    const uint32_t k = set.count();
    const bool fold = set.fold;
    if ( perPattern != nullptr ) std::fill_n( perPattern, k, uint64_t( 0 ) );
    if ( to.grown != nullptr ) to.grown->clear();
    if ( to.grownIds != nullptr ) to.grownIds->clear();
    const uint64_t nTiles = forEachTile( spans, n, SEARCH_TILE, set.mMin, [] ( size_t, uint64_t, uint64_t ) {} );
    if ( nTiles == 0 && seamN == 0 ) return MI355X_BZ2_OK;
    if ( nTiles > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const SearchSetLayout l = laySearchSet( QUERY_SIZES, nTiles, n, k );
    const uint64_t cap = doubled( c->dSearch, l.bytes );
    if ( const int status = growStaging( c, c->hSearch, c->dSearch, l.countsAt, cap, l.bytes, cap ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    auto* tile = at<SetTile>( h, l.tilesAt );
    forEachTile( spans, n, SEARCH_TILE, set.mMin, [spans, &tile] ( size_t s, uint64_t from, uint64_t length ) {
        *tile++ = { spans[s].offset + from, spans[s].offset + spans[s].size, (uint32_t)length, (uint32_t)s };
    } );
    writeSetImage( set, h + l.imageAt, fold );
    const auto* const dTiles = at<const SetTile>( d, l.tilesAt );
    auto* const dTileCounts = at<uint32_t>( d, l.countsAt );
    const auto nBytes = (uint32_t)set.bytes.size();
    const auto groups = (uint32_t)std::min<uint64_t>( ( nTiles + SET_WAVES - 1 ) / SET_WAVES, SET_MAX_GROUPS );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    HIP_TRY( c, hipMemsetAsync( d + l.resultsAt, 0, l.countsAt - l.resultsAt, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( fold ? k_count_set<true> : k_count_set<false>, dim3( groups ), dim3( SET_THREADS ), 0, c->stream, dTiles,
                            (uint32_t)nTiles, c->dOut, d + l.imageAt, nBytes, k, dTileCounts, at<unsigned long long>( d, l.resultsAt ),
                            at<unsigned long long>( d, l.eachAt ) );
        HIP_TRY( c, hipGetLastError() );
    }
    if ( const int status = launchSeam( c, seam, seamN, d + l.seamAt ) ) return status;
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.countsAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    std::copy_n( at<const uint64_t>( h, l.resultsAt ), n, counts );
    if ( perPattern != nullptr ) std::memcpy( perPattern, h + l.eachAt, k * sizeof( uint64_t ) );
    copySeam( h + l.seamAt, seamN, seamBytes );
    return emitListed( c, what, std::accumulate( counts, counts + n, uint64_t( 0 ) ), capacity, to, dTileCounts, nTiles,
                       at<uint64_t>( d, l.placesAt ), [&] ( uint64_t wanted, uint64_t* dPositions, uint32_t* dIds ) {
        hipLaunchKernelGGL( fold ? k_emit_set<true> : k_emit_set<false>, dim3( groups ), dim3( SET_THREADS ), 0, c->stream, dTiles,
                            (uint32_t)nTiles, c->dOut, d + l.imageAt, nBytes, k, at<uint64_t>( d, l.placesAt ), wanted, dPositions, dIds );
    } );
}

static_assert( REGEX_STATES == REGEX_MAX_STATES && REGEX_CHUNK == REGEX_CHUNK_BYTES, "the kernels' constants are the compiler's" );

/**
 * mi355x_bz2_match_lines and the reader's launches.  Every span is cut into tiles of COUNT_TILE bytes = REGEX_THREADS
 * chunks; k_regex_chunks summarises every chunk, k_regex_link -- one workgroup per span -- gives the chunks their entry
 * states and head hits and writes the spans' summaries and counts, which come back in one D2H.  With capacity > 0,
 * emitListed (over the chunk counts) and k_regex_emit bring the witnesses to `positions`, or to `grown` resized to their
 * number.  An empty span has the identity for its headMap: the link kernel runs for spans that are all empty, too.
 */
int
matchLines( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, uint32_t n, const Regex& regex, uint8_t nl,
            uint8_t* headMaps, uint8_t* hasDelimiter, uint8_t* exitStates, uint64_t capacity, uint64_t* positions,
            std::vector<uint64_t>* grown, uint64_t* counts )
{
    const std::scoped_lock lock( c->mutex );
    const bool compiled = regex.n >= 2 && regex.n <= REGEX_MAX_STATES && regex.transitions.size() == (size_t)regex.n * 256
                          && regex.acceptsAtEnd.size() == regex.n;
    if ( const int status = refuseQuery( c, what, spans, n, compiled ? "" : "not a compiled regular expression" ) ) return status;
    if ( grown != nullptr ) grown->clear();
    if ( n == 0 ) return MI355X_BZ2_OK;
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * REGEX_THREADS;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    /* the host holds what goes up and comes down, not the per-chunk arrays */
    const RegexLayout l = layRegex( QUERY_SIZES, nTiles, n, regex.n );
    if ( const int status = growLineStaging( c, l.mapsAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    for ( uint32_t s = 0; s < n; ++s ) {
        const uint64_t nChunks = ( spans[s].size + REGEX_CHUNK - 1 ) / REGEX_CHUNK;
        at<RegexSpan>( h, l.spansAt )[s] = { (uint32_t)( firstTile[s] * REGEX_THREADS ), (uint32_t)nChunks };
    }
    std::memcpy( h + l.tableAt, regex.transitions.data(), (size_t)regex.n * 256 );
    std::memset( h + l.acceptsAt, 0, l.resultsAt - l.acceptsAt );
    std::memcpy( h + l.acceptsAt, regex.acceptsAtEnd.data(), regex.n );
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    auto* const dInfo = at<uint32_t>( d, l.infoAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_regex_chunks, dim3( (uint32_t)nTiles ), dim3( REGEX_THREADS ), 0, c->stream, dTiles, c->dOut,
                            d + l.tableAt, d + l.acceptsAt, regex.n, (uint32_t)nl, d + l.mapsAt, dInfo, dCounts );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_regex_link, dim3( n ), dim3( REGEX_THREADS ), 0, c->stream, at<const RegexSpan>( d, l.spansAt ),
                        d + l.acceptsAt, regex.n, d + l.mapsAt, dInfo, dCounts, d + l.resultsAt, at<uint32_t>( d, l.spanInfoAt ),
                        at<unsigned long long>( d, l.spanCountsAt ) );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.mapsAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    uint64_t total = 0;
    for ( uint32_t i = 0; i < n; ++i ) {
        const uint32_t info = at<const uint32_t>( h, l.spanInfoAt )[i];
        std::memcpy( headMaps + (size_t)i * REGEX_STATES, h + l.resultsAt + (size_t)i * REGEX_STATES, REGEX_STATES );
        hasDelimiter[i] = ( info & REGEX_HAS_DELIMITER ) != 0 ? 1 : 0;
        exitStates[i] = (uint8_t)( info >> REGEX_EXIT_SHIFT );
        counts[i] = at<const uint64_t>( h, l.spanCountsAt )[i];
        total += counts[i];
    }
    return emitListed( c, what, total, capacity, { positions, grown }, dCounts, slots, at<uint64_t>( d, l.placesAt ),
                       [&] ( uint64_t wanted, uint64_t* dPositions, uint32_t* ) {
        hipLaunchKernelGGL( k_regex_emit, dim3( (uint32_t)nTiles ), dim3( REGEX_THREADS ), 0, c->stream, dTiles, c->dOut, d + l.tableAt,
                            d + l.acceptsAt, regex.n, (uint32_t)nl, dInfo, at<uint64_t>( d, l.placesAt ), wanted, dPositions );
    } );
}

static_assert( LINEHASH_CHUNK == LINEHASH_CHUNK_BYTES && LINEHASH_PRIME == LINEHASH_P, "the kernels' constants are the host's" );

/**
 * mi355x_bz2_hash_lines and the reader's launches.  Every span is cut into tiles of COUNT_TILE bytes = LINEHASH_THREADS
 * chunks; k_linehash_chunks summarises every chunk and scans each tile, k_linehash_link -- one workgroup per span --
 * scans the tiles and writes the spans' summaries and counts, which come back in one D2H.  With hashes wanted,
 * k_scan_tiles turns the chunk counts into places and k_linehash_emit writes the hashes of the closed lines [skip,
 * skip + capacity) -- numbered over all spans in caller order -- to dHashes[0, ...), device memory of the caller's.
 */
int
hashLines( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint64_t x,
           mi355x_bz2_line_hash_summary* summaries, uint64_t skip, uint64_t capacity, uint64_t* dHashes )
{
    const std::scoped_lock lock( c->mutex );
    if ( const int status = refuseQuery( c, what, spans, n ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * LINEHASH_THREADS;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    /* the host holds what goes up and comes down, not the per-tile and per-chunk arrays */
    const LineHashLayout l = layLineHash( QUERY_SIZES, nTiles, n );
    if ( const int status = growLineStaging( c, l.tileSummariesAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    for ( uint32_t s = 0; s < n; ++s ) at<LineHashSpan>( h, l.spansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s] };
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    auto* const dTileSummaries = at<LineHashTile>( d, l.tileSummariesAt );
    auto* const dPrefixes = at<ulonglong2>( d, l.prefixesAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_linehash_chunks, dim3( (uint32_t)nTiles ), dim3( LINEHASH_THREADS ), 0, c->stream, dTiles, c->dOut,
                            x, (uint32_t)nl, dPrefixes, dCounts, dTileSummaries );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_linehash_link, dim3( n ), dim3( LINEHASH_THREADS ), 0, c->stream, at<const LineHashSpan>( d, l.spansAt ),
                        dTileSummaries, at<LineHashSpanSummary>( d, l.resultsAt ) );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.tileSummariesAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    uint64_t total = 0;
    for ( uint32_t i = 0; i < n; ++i ) {
        const auto& from = at<const LineHashSpanSummary>( h, l.resultsAt )[i];
        summaries[i] = { from.headH, from.headXl, from.tailH, from.tailXl, from.count,
                         ( from.info & LINEHASH_HAS_DELIMITER ) != 0 ? 1u : 0u, ( from.info & LINEHASH_TAIL_NON_EMPTY ) != 0 ? 1u : 0u };
        total += from.count;
    }
    if ( capacity == 0 || skip >= total || nTiles == 0 ) return MI355X_BZ2_OK;

    auto* const dPlaces = at<uint64_t>( d, l.placesAt );
    hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)slots, dPlaces );
    HIP_TRY( c, hipGetLastError() );
    hipLaunchKernelGGL( k_linehash_emit, dim3( (uint32_t)nTiles ), dim3( LINEHASH_THREADS ), 0, c->stream, dTiles, c->dOut, x,
                        (uint32_t)nl, dPrefixes, dTileSummaries, dPlaces, skip, capacity, dHashes );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    return MI355X_BZ2_OK;
}

static_assert( FIELD_CHUNK == FIELD_CHUNK_BYTES && FIELD_NOT_REACHED == FIELD_UNKNOWN, "the kernels' constants are the host's" );

/**
 * mi355x_bz2_field_spans and the reader's launches.  The tiling is hashLines'; k_field_chunks gives every chunk its
 * element and scans each tile, k_field_link -- one workgroup per span -- scans the tiles, k_scan_tiles turns the chunk
 * counts into places, k_field_emit writes starts and ends of field `field` in the closed lines [skip, skip + capacity)
 * -- numbered over all spans in caller order -- to dStarts[0, ...) and dSizes[0, ...), device memory of the caller's, and
 * completes the spans' summaries and head positions, and k_field_sizes turns the ends into sizes.  The kernels queue
 * behind one another and the summaries come back in one D2H behind them.  The first byte of span i counts as offset
 * bases[i] (nullptr: its offset in the output).  k_field_emit runs whatever the capacity: the summaries need it.
 */
int
fieldSpans( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, const uint64_t* bases, uint32_t n, uint8_t nl,
            uint8_t dl, uint32_t field, mi355x_bz2_field_summary* summaries, uint64_t* headPositions, uint64_t skip,
            uint64_t capacity, uint64_t* dStarts, int64_t* dSizes )
{
    const std::scoped_lock lock( c->mutex );
    const auto why = fieldArgumentsError( nl, dl, field );
    if ( !why.empty() ) return refuse( c, what, why );
    if ( const int status = refuseQuery( c, what, spans, n ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * FIELD_THREADS, cap = (uint64_t)field + 1;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const FieldLayout l = layFields( QUERY_SIZES, nTiles, n, field );
    if ( const int status = growLineStaging( c, l.tileSummariesAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    uint64_t bytesInSpans = 0;
    for ( uint32_t s = 0; s < n; ++s ) {
        const uint64_t base = bases != nullptr ? bases[s] : spans[s].offset;
        at<FieldSpanTiles>( h, l.spansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s], base };
        bytesInSpans += spans[s].size;
    }
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    const auto* const dSpans = at<const FieldSpanTiles>( d, l.spansAt );
    auto* const dSummaries = at<FieldSpanSummary>( d, l.resultsAt );
    auto* const dTileSummaries = at<FieldTile>( d, l.tileSummariesAt );
    auto* const dPlaces = at<uint64_t>( d, l.placesAt );
    auto* const dPrefixes = at<uint32_t>( d, l.prefixesAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_field_chunks, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, (uint32_t)cap, dPrefixes, dCounts, dTileSummaries );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_field_link, dim3( n ), dim3( FIELD_THREADS ), 0, c->stream, dSpans, dTileSummaries, dSummaries, field );
    HIP_TRY( c, hipGetLastError() );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)slots, dPlaces );
        HIP_TRY( c, hipGetLastError() );
        hipLaunchKernelGGL( k_field_emit, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, field, dSpans, dPrefixes, dTileSummaries, dPlaces, dSummaries,
                            at<uint64_t>( d, l.headsAt ), skip, capacity, dStarts, dSizes );
        HIP_TRY( c, hipGetLastError() );
        /* a span closes at most one line per byte */
        const uint64_t most = std::min( capacity, bytesInSpans );
        if ( most > 0 ) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( most + FIELD_SIZES_THREADS - 1 ) / FIELD_SIZES_THREADS, FIELD_SIZES_BLOCKS );
            hipLaunchKernelGGL( k_field_sizes, dim3( blocks ), dim3( FIELD_SIZES_THREADS ), 0, c->stream, dPlaces, dCounts, slots,
                                skip, capacity, dStarts, dSizes );
            HIP_TRY( c, hipGetLastError() );
        }
    }
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.tileSummariesAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( uint32_t i = 0; i < n; ++i ) {
        const auto& from = at<const FieldSpanSummary>( h, l.resultsAt )[i];
        summaries[i] = { from.count, from.firstNl, from.tailStart, from.tailFieldStart, from.tailFieldEnd, from.headDelims,
                         from.tailDelims, ( from.info & FIELD_HAS_DELIMITER ) != 0 ? 1u : 0u,
                         ( from.info & FIELD_TAIL_NON_EMPTY ) != 0 ? 1u : 0u };
        if ( headPositions != nullptr ) {
            std::copy_n( at<const uint64_t>( h, l.headsAt ) + i * cap, std::min<uint64_t>( from.headDelims, cap ),
                         headPositions + i * cap );
        }
    }
    return MI355X_BZ2_OK;
}

static_assert( sizeof( QuotedFieldSpanSummary ) == 64, "16-byte aligned in layQuotedFields" );

/**
 * mi355x_bz2_field_spans_quoted and the reader's launches: fieldSpans with the quoted twins of its kernels
 * (bz2_fieldquote.hip.h), the head positions of both entry hypotheses, 2 * ( field + 1 ) per span, and k_field_unquote
 * behind k_field_sizes, which turns the raw fields of the closed lines into their contents.
 */
int
fieldSpansQuoted( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, const uint64_t* bases, uint32_t n, uint8_t nl,
                  uint8_t dl, uint8_t quote, uint32_t field, mi355x_bz2_quoted_field_summary* summaries, uint64_t* headPositions,
                  uint64_t skip, uint64_t capacity, uint64_t* dStarts, int64_t* dSizes )
{
    const std::scoped_lock lock( c->mutex );
    const auto why = quotedFieldArgumentsError( nl, dl, quote, field );
    if ( !why.empty() ) return refuse( c, what, why );
    if ( const int status = refuseQuery( c, what, spans, n ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * FIELD_THREADS, cap = (uint64_t)field + 1;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const FieldLayout l = layQuotedFields( QUERY_SIZES, sizeof( QuotedFieldSpanSummary ), nTiles, n, field );
    if ( const int status = growLineStaging( c, l.tileSummariesAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    uint64_t bytesInSpans = 0;
    for ( uint32_t s = 0; s < n; ++s ) {
        const uint64_t base = bases != nullptr ? bases[s] : spans[s].offset;
        at<FieldSpanTiles>( h, l.spansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s], base };
        bytesInSpans += spans[s].size;
    }
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    const auto* const dSpans = at<const FieldSpanTiles>( d, l.spansAt );
    auto* const dSummaries = at<QuotedFieldSpanSummary>( d, l.resultsAt );
    auto* const dTileSummaries = at<FieldTile>( d, l.tileSummariesAt );
    auto* const dPlaces = at<uint64_t>( d, l.placesAt );
    auto* const dPrefixes = at<uint32_t>( d, l.prefixesAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_field_chunks_quoted, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, (uint32_t)quote, (uint32_t)cap, dPrefixes, dCounts, dTileSummaries );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_field_link_quoted, dim3( n ), dim3( FIELD_THREADS ), 0, c->stream, dSpans, dTileSummaries, dSummaries, field );
    HIP_TRY( c, hipGetLastError() );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)slots, dPlaces );
        HIP_TRY( c, hipGetLastError() );
        hipLaunchKernelGGL( k_field_emit_quoted, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, (uint32_t)quote, field, dSpans, dPrefixes, dTileSummaries, dPlaces, dSummaries,
                            at<uint64_t>( d, l.headsAt ), skip, capacity, dStarts, dSizes );
        HIP_TRY( c, hipGetLastError() );
        /* a span closes at most one line per byte */
        const uint64_t most = std::min( capacity, bytesInSpans );
        if ( most > 0 ) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( most + FIELD_SIZES_THREADS - 1 ) / FIELD_SIZES_THREADS, FIELD_SIZES_BLOCKS );
            hipLaunchKernelGGL( k_field_sizes, dim3( blocks ), dim3( FIELD_SIZES_THREADS ), 0, c->stream, dPlaces, dCounts, slots,
                                skip, capacity, dStarts, dSizes );
            HIP_TRY( c, hipGetLastError() );
            static_assert( FIELD_UNQUOTE_THREADS == FIELD_SIZES_THREADS && FIELD_UNQUOTE_BLOCKS == FIELD_SIZES_BLOCKS );
            hipLaunchKernelGGL( k_field_unquote, dim3( blocks ), dim3( FIELD_UNQUOTE_THREADS ), 0, c->stream, dTiles, nTiles, dSpans, n,
                                dPlaces, dCounts, slots, c->dOut, (uint32_t)quote, skip, capacity, dStarts, dSizes );
            HIP_TRY( c, hipGetLastError() );
        }
    }
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.tileSummariesAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( uint32_t i = 0; i < n; ++i ) {
        const auto& from = at<const QuotedFieldSpanSummary>( h, l.resultsAt )[i];
        summaries[i] = { from.count, from.firstNl, from.tailStart, from.tailFieldStart, from.tailFieldEnd,
                         { from.headDelims[0], from.headDelims[1] }, from.tailDelims, ( from.info & FIELD_HAS_DELIMITER ) != 0 ? 1u : 0u,
                         ( from.info & FIELD_TAIL_NON_EMPTY ) != 0 ? 1u : 0u, from.headQuoteParity,
                         ( from.info & FIELD_TAIL_IN_QUOTE ) != 0 ? 1u : 0u, 0u };
        if ( headPositions != nullptr ) {
            for ( uint32_t hypothesis = 0; hypothesis < 2; ++hypothesis ) {
                const uint64_t first = ( 2 * (uint64_t)i + hypothesis ) * cap;
                std::copy_n( at<const uint64_t>( h, l.headsAt ) + first, std::min<uint64_t>( from.headDelims[hypothesis], cap ),
                             headPositions + first );
            }
        }
    }
    return MI355X_BZ2_OK;
}

static_assert( sizeof( FieldColumnCheck ) == 24 && FIELDCOL_TILE == FIELD_COLUMN_TILE_BYTES, "the layout's check; the host's constant" );

/**
 * mi355x_bz2_gather_fields.  The n spans are in device memory already, so nothing goes up and the check that refuseQuery
 * makes on the host is k_fieldcol_sums': the spans' check and the tile sums, k_fieldcol_top for the tiles' prefixes and the
 * total, and the 24 bytes of the check come back -- the one wait of the call before its last.  With an offender the call
 * ends there: no span is read.  Else destination( total, &dst ) names where the bytes go (null: nowhere; false: it found
 * no memory, MI355X_BZ2_ERR_DEVICE), k_fieldcol_offsets writes dOffsets[0, n] and k_field_gather copies the bytes.  A
 * span's start counts from `base`, modulo 2^64: start - base is its offset in the output.  *firstSize, if wanted,
 * receives the bytes of span 0: dOffsets[1].
 */
template<typename Destination>
int
gatherFields( mi355x_bz2_ctx* c, const char* what, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n, uint64_t base,
              uint64_t* dOffsets, const Destination& destination, uint64_t* total, uint64_t* firstSize = nullptr )
{
    const std::scoped_lock lock( c->mutex );
    if ( const int status = refuseQuery( c, what, nullptr, 0 ) ) return status;
    *total = 0;
    if ( firstSize != nullptr ) *firstSize = 0;
    const FieldColumnLayout l = layFieldColumn( n, FIELDCOL_SCAN_TILE );
    if ( l.scanTiles > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );
    if ( n == 0 ) {
        HIP_TRY( c, hipMemsetAsync( dOffsets, 0, sizeof( uint64_t ), c->stream ) );
        HIP_TRY( c, hipStreamSynchronize( c->stream ) );
        return MI355X_BZ2_OK;
    }
    if ( const int status = growLineStaging( c, l.tileSumsAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    auto* const hCheck = at<FieldColumnCheck>( h, l.checkAt );
    auto* const dCheck = at<FieldColumnCheck>( d, l.checkAt );
    auto* const dTileSums = at<uint64_t>( d, l.tileSumsAt );
    auto* const dTilePrefixes = at<uint64_t>( d, l.tilePrefixesAt );
    *hCheck = { 0, FIELDCOL_NONE, 0 };
    HIP_TRY( c, hipMemcpyAsync( dCheck, hCheck, sizeof( FieldColumnCheck ), hipMemcpyHostToDevice, c->stream ) );
    hipLaunchKernelGGL( k_fieldcol_sums, dim3( (uint32_t)l.scanTiles ), dim3( FIELDCOL_THREADS ), 0, c->stream, dStarts, dSizes, n, base,
                        c->outSize, dTileSums, dCheck );
    HIP_TRY( c, hipGetLastError() );
    hipLaunchKernelGGL( k_fieldcol_top, dim3( 1 ), dim3( FIELDCOL_THREADS ), 0, c->stream, dTileSums, l.scanTiles, dTilePrefixes, dCheck );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( hCheck, dCheck, sizeof( FieldColumnCheck ), hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    if ( hCheck->offenders != 0 ) {
        return refuse( c, what, "span " + std::to_string( hCheck->first ) + " lies outside the last batch's output ("
                                + std::to_string( hCheck->offenders ) + " of the spans do)" );
    }
    *total = hCheck->total;
    uint8_t* dst = nullptr;
    if ( !destination( *total, &dst ) ) {
        c->lastError = std::string( what ) + ": no device memory for the " + std::to_string( *total ) + " bytes of the fields";
        return MI355X_BZ2_ERR_DEVICE;
    }
    const uint64_t gatherTiles = fieldGatherTiles( *total, reinterpret_cast<uintptr_t>( dst ) & 15u, FIELDCOL_TILE );
    if ( gatherTiles > 0x7FFFFFFFu ) return refuse( c, what, "too many bytes" );
    hipLaunchKernelGGL( k_fieldcol_offsets, dim3( (uint32_t)l.scanTiles ), dim3( FIELDCOL_THREADS ), 0, c->stream, dSizes, n,
                        dTilePrefixes, dCheck, dOffsets );
    HIP_TRY( c, hipGetLastError() );
    auto* const hFirst = at<uint64_t>( h, sizeof( FieldColumnCheck ) );   /* behind the check, in front of tileSumsAt */
    if ( firstSize != nullptr ) HIP_TRY( c, hipMemcpyAsync( hFirst, dOffsets + 1, sizeof( uint64_t ), hipMemcpyDeviceToHost, c->stream ) );
    if ( dst != nullptr && gatherTiles > 0 ) {
        hipLaunchKernelGGL( k_field_gather, dim3( (uint32_t)gatherTiles ), dim3( FIELDCOL_THREADS ), 0, c->stream, dStarts, dOffsets, n,
                            base, *total, c->dOut, dst );
        HIP_TRY( c, hipGetLastError() );
    }
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    if ( firstSize != nullptr ) *firstSize = *hFirst;
    return MI355X_BZ2_OK;
}

static_assert( sizeof( FieldHashTail ) == 16 && FIELDHASH_MISSING == FIELD_MISSING, "the layout's tail hashes; the host's constant" );
static_assert( FIELD_MISSING == MI355X_BZ2_FIELD_MISSING, "the C ABI's constant" );

/**
 * mi355x_bz2_field_hashes and the reader's launches.  The tiling is fieldSpans'; k_field_chunks / k_field_link and
 * k_linehash_chunks / k_linehash_link run as they are, each with its own lists, and the spans' counts and hash summaries
 * come back: the number of lines says how many prefixes have to be kept.  Then k_scan_tiles, k_fieldhash_emit and
 * k_fieldhash_finish write keys, starts and sizes of the closed lines [skip, skip + capacity) -- numbered over all spans
 * in caller order -- to dKeys, dStarts and dSizes, device memory of the caller's (dStarts and dSizes may both be null:
 * they then lie beside the prefixes in dSearchPositions), and the field summaries, tail hashes, head positions and head
 * hashes come back in one D2H.  The first byte of span i counts as offset bases[i] (nullptr: its offset in the output).
 */
int
fieldHashes( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, const uint64_t* bases, uint32_t n, uint8_t nl,
             uint8_t dl, uint32_t field, uint64_t x, mi355x_bz2_field_hash_summary* summaries, uint64_t* headPositions,
             uint64_t* headHashes, uint64_t skip, uint64_t capacity, uint64_t* dKeys, uint64_t* dStarts, int64_t* dSizes )
{
    const std::scoped_lock lock( c->mutex );
    const auto why = fieldArgumentsError( nl, dl, field );
    if ( !why.empty() ) return refuse( c, what, why );
    if ( const int status = refuseQuery( c, what, spans, n ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * FIELD_THREADS, cap = (uint64_t)field + 1;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const FieldHashLayout l = layFieldHashes( QUERY_SIZES, nTiles, n, field );
    if ( const int status = growLineStaging( c, l.tileSummariesAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    for ( uint32_t s = 0; s < n; ++s ) {
        const uint64_t base = bases != nullptr ? bases[s] : spans[s].offset;
        at<FieldSpanTiles>( h, l.spansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s], base };
        at<LineHashSpan>( h, l.hashSpansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s] };
    }
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    const auto* const dSpans = at<const FieldSpanTiles>( d, l.spansAt );
    auto* const dSummaries = at<FieldSpanSummary>( d, l.resultsAt );
    auto* const dTileSummaries = at<FieldTile>( d, l.tileSummariesAt );
    auto* const dHashTiles = at<LineHashTile>( d, l.hashTilesAt );
    auto* const dPlaces = at<uint64_t>( d, l.placesAt );
    auto* const dHashPrefixes = at<ulonglong2>( d, l.hashPrefixesAt );
    auto* const dPrefixes = at<uint32_t>( d, l.prefixesAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    /* the tail of a span that no event reaches starts, for field 0, at its first byte with hash 0 */
    HIP_TRY( c, hipMemsetAsync( d + l.tailsAt, 0, l.headsAt - l.tailsAt, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_field_chunks, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, (uint32_t)cap, dPrefixes, dCounts, dTileSummaries );
        HIP_TRY( c, hipGetLastError() );
        hipLaunchKernelGGL( k_linehash_chunks, dim3( (uint32_t)nTiles ), dim3( LINEHASH_THREADS ), 0, c->stream, dTiles, c->dOut,
                            x, (uint32_t)nl, dHashPrefixes, at<uint32_t>( d, l.hashCountsAt ), dHashTiles );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_field_link, dim3( n ), dim3( FIELD_THREADS ), 0, c->stream, dSpans, dTileSummaries, dSummaries, field );
    HIP_TRY( c, hipGetLastError() );
    hipLaunchKernelGGL( k_linehash_link, dim3( n ), dim3( LINEHASH_THREADS ), 0, c->stream, at<const LineHashSpan>( d, l.hashSpansAt ),
                        dHashTiles, at<LineHashSpanSummary>( d, l.hashSummariesAt ) );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( h + l.hashSummariesAt, d + l.hashSummariesAt, l.tailsAt - l.hashSummariesAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    uint64_t total = 0;
    for ( uint32_t i = 0; i < n; ++i ) total += at<const LineHashSpanSummary>( h, l.hashSummariesAt )[i].count;
    const uint64_t wanted = total > skip ? std::min( capacity, total - skip ) : 0;

    if ( nTiles > 0 ) {
        /* P( start ) per wanted line, and starts and sizes where the caller wants none */
        const bool ownSpans = dStarts == nullptr || dSizes == nullptr;
        const uint64_t need = wanted * sizeof( uint64_t ) * ( ownSpans ? 3 : 1 );
        HIP_TRY( c, c->dSearchPositions.grow( c, need, need + need / 4, need ) );
        auto* const dPStarts = at<uint64_t>( c->dSearchPositions.bytes, 0 );
        if ( ownSpans ) {
            dStarts = dPStarts + wanted;
            dSizes = reinterpret_cast<int64_t*>( dPStarts + 2 * wanted );
        }
        hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)slots, dPlaces );
        HIP_TRY( c, hipGetLastError() );
        hipLaunchKernelGGL( k_fieldhash_emit, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut, x,
                            (uint32_t)nl, (uint32_t)dl, field, dSpans, dPrefixes, dTileSummaries, dHashPrefixes, dHashTiles, dPlaces,
                            dSummaries, at<FieldHashTail>( d, l.tailsAt ), at<uint64_t>( d, l.headsAt ),
                            at<uint64_t>( d, l.headHashesAt ), skip, wanted, dStarts, dSizes, dPStarts, dKeys );
        HIP_TRY( c, hipGetLastError() );
        if ( wanted > 0 ) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( wanted + FIELD_SIZES_THREADS - 1 ) / FIELD_SIZES_THREADS, FIELD_SIZES_BLOCKS );
            hipLaunchKernelGGL( k_fieldhash_finish, dim3( blocks ), dim3( FIELD_SIZES_THREADS ), 0, c->stream, dPlaces, dCounts, slots,
                                skip, wanted, x, dStarts, dSizes, dPStarts, dKeys );
            HIP_TRY( c, hipGetLastError() );
        }
    }
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.tileSummariesAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( uint32_t i = 0; i < n; ++i ) {
        const auto& from = at<const FieldSpanSummary>( h, l.resultsAt )[i];
        const auto& hashes = at<const LineHashSpanSummary>( h, l.hashSummariesAt )[i];
        const auto& tail = at<const FieldHashTail>( h, l.tailsAt )[i];
        summaries[i] = { from.count, from.firstNl, from.tailStart, from.tailFieldStart, from.tailFieldEnd,
                         hashes.headH, hashes.headXl, hashes.tailH, hashes.tailXl, tail.startHash, tail.endHash, from.headDelims,
                         from.tailDelims, ( from.info & FIELD_HAS_DELIMITER ) != 0 ? 1u : 0u,
                         ( from.info & FIELD_TAIL_NON_EMPTY ) != 0 ? 1u : 0u };
        const uint64_t listed = std::min<uint64_t>( from.headDelims, cap );
        if ( headPositions != nullptr ) std::copy_n( at<const uint64_t>( h, l.headsAt ) + i * cap, listed, headPositions + i * cap );
        if ( headHashes != nullptr ) std::copy_n( at<const uint64_t>( h, l.headHashesAt ) + i * cap, listed, headHashes + i * cap );
    }
    return MI355X_BZ2_OK;
}

static_assert( sizeof( FieldNumberSpan ) == 16 && sizeof( FieldText ) == FIELDNUM_TEXT_BYTES && sizeof( mi355x_bz2_field_text ) == 20,
               "the layout's extents and texts" );
static_assert( FIELDNUM_NOT_A_NUMBER == FIELD_NOT_A_NUMBER && FIELDNUM_MISSING == FIELD_NUMBER_MISSING
               && FIELDNUM_BYTES == FIELD_NUMBER_BYTES && FIELDNUM_TEXT_BYTES == FIELD_TEXT_LONG, "the kernels' constants are the host's" );
static_assert( FIELD_NOT_A_NUMBER == MI355X_BZ2_FIELD_NOT_A_NUMBER && FIELD_NUMBER_MISSING == MI355X_BZ2_FIELD_NUMBER_MISSING,
               "the C ABI's constants" );

/**
 * mi355x_bz2_field_numbers and the reader's launches.  fieldSpans' passes as they are, with its lists; behind k_field_sizes
 * k_field_numbers parses the field of the closed lines [skip, skip + capacity) into dNumbers, device memory of the
 * caller's (dStarts and dSizes may both be null: they then lie in dSearchPositions), and behind k_field_emit
 * k_field_texts writes the texts of every span's head and tail, which come back with the summaries in one D2H.  The
 * first byte of span 0 counts as offset *fileOffset (nullptr: every span's first byte as its offset in the output), which
 * takes n == 1: k_field_numbers finds a field in the output from its start alone.
 */
int
fieldNumbers( mi355x_bz2_ctx* c, const char* what, const mi355x_bz2_byte_span* spans, const uint64_t* fileOffset, uint32_t n,
              uint8_t nl, uint8_t dl, uint32_t field, mi355x_bz2_field_summary* summaries, uint64_t* headPositions,
              mi355x_bz2_field_text* headTexts, mi355x_bz2_field_text* tailTexts, uint64_t skip, uint64_t capacity,
              int64_t* dNumbers, uint64_t* dStarts, int64_t* dSizes )
{
    const std::scoped_lock lock( c->mutex );
    const auto why = fieldArgumentsError( nl, dl, field );
    if ( !why.empty() ) return refuse( c, what, why );
    if ( const int status = refuseQuery( c, what, spans, n ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    if ( fileOffset != nullptr && n != 1 ) return refuse( c, what, "a file offset takes one span" );
    const auto firstTile = firstTiles( spans, n, COUNT_TILE, 1 );
    const uint64_t nTiles = firstTile.back(), slots = nTiles * FIELD_THREADS, cap = (uint64_t)field + 1;
    if ( slots > 0x7FFFFFFFu ) return refuse( c, what, "too many spans" );
    HIP_TRY( c, hipSetDevice( c->device ) );

    const FieldNumberLayout l = layFieldNumbers( QUERY_SIZES, nTiles, n, field );
    if ( const int status = growLineStaging( c, l.tileSummariesAt, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    writeCountTiles( at<CountTile>( h, l.tilesAt ), spans, n, COUNT_TILE, 1 );
    uint64_t bytesInSpans = 0;
    for ( uint32_t s = 0; s < n; ++s ) {
        const uint64_t base = fileOffset != nullptr ? *fileOffset : spans[s].offset;
        at<FieldSpanTiles>( h, l.spansAt )[s] = { firstTile[s], firstTile[s + 1] - firstTile[s], base };
        at<FieldNumberSpan>( h, l.extentsAt )[s] = { spans[s].offset, spans[s].size };
        bytesInSpans += spans[s].size;
    }
    /* a start less this is the field's offset in the output */
    const uint64_t delta = fileOffset != nullptr ? *fileOffset - spans[0].offset : 0;
    const auto* const dTiles = at<const CountTile>( d, l.tilesAt );
    const auto* const dSpans = at<const FieldSpanTiles>( d, l.spansAt );
    auto* const dSummaries = at<FieldSpanSummary>( d, l.resultsAt );
    auto* const dHeads = at<uint64_t>( d, l.headsAt );
    auto* const dTileSummaries = at<FieldTile>( d, l.tileSummariesAt );
    auto* const dPlaces = at<uint64_t>( d, l.placesAt );
    auto* const dPrefixes = at<uint32_t>( d, l.prefixesAt );
    auto* const dCounts = at<uint32_t>( d, l.countsAt );
    /* a span closes at most one line per byte */
    const uint64_t most = std::min( capacity, bytesInSpans );
    if ( most > 0 && ( dStarts == nullptr || dSizes == nullptr ) ) {
        const uint64_t need = most * 2 * sizeof( uint64_t );
        HIP_TRY( c, c->dSearchPositions.grow( c, need, need + need / 4, need ) );
        dStarts = at<uint64_t>( c->dSearchPositions.bytes, 0 );
        dSizes = reinterpret_cast<int64_t*>( dStarts + most );
    }
    HIP_TRY( c, hipMemcpyAsync( d, h, l.resultsAt, hipMemcpyHostToDevice, c->stream ) );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_field_chunks, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, (uint32_t)cap, dPrefixes, dCounts, dTileSummaries );
        HIP_TRY( c, hipGetLastError() );
    }
    hipLaunchKernelGGL( k_field_link, dim3( n ), dim3( FIELD_THREADS ), 0, c->stream, dSpans, dTileSummaries, dSummaries, field );
    HIP_TRY( c, hipGetLastError() );
    if ( nTiles > 0 ) {
        hipLaunchKernelGGL( k_scan_tiles, dim3( 1 ), dim3( SCAN_THREADS ), 0, c->stream, dCounts, (uint32_t)slots, dPlaces );
        HIP_TRY( c, hipGetLastError() );
        hipLaunchKernelGGL( k_field_emit, dim3( (uint32_t)nTiles ), dim3( FIELD_THREADS ), 0, c->stream, dTiles, c->dOut,
                            (uint32_t)nl, (uint32_t)dl, field, dSpans, dPrefixes, dTileSummaries, dPlaces, dSummaries, dHeads, skip,
                            most, dStarts, dSizes );
        HIP_TRY( c, hipGetLastError() );
        if ( most > 0 ) {
            const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( most + FIELD_SIZES_THREADS - 1 ) / FIELD_SIZES_THREADS, FIELD_SIZES_BLOCKS );
            hipLaunchKernelGGL( k_field_sizes, dim3( blocks ), dim3( FIELD_SIZES_THREADS ), 0, c->stream, dPlaces, dCounts, slots,
                                skip, most, dStarts, dSizes );
            HIP_TRY( c, hipGetLastError() );
            hipLaunchKernelGGL( k_field_numbers, dim3( blocks ), dim3( FIELD_SIZES_THREADS ), 0, c->stream, dPlaces, dCounts, slots,
                                skip, most, c->dOut, delta, dStarts, dSizes, reinterpret_cast<long long*>( dNumbers ) );
            HIP_TRY( c, hipGetLastError() );
        }
    }
    hipLaunchKernelGGL( k_field_texts, dim3( n ), dim3( FIELDNUM_TEXT_THREADS ), 0, c->stream, at<const FieldNumberSpan>( d, l.extentsAt ),
                        dSummaries, dHeads, c->dOut, field, d + l.headTextsAt, d + l.tailTextsAt );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipMemcpyAsync( h + l.resultsAt, d + l.resultsAt, l.tileSummariesAt - l.resultsAt, hipMemcpyDeviceToHost, c->stream ) );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    for ( uint32_t i = 0; i < n; ++i ) {
        const auto& from = at<const FieldSpanSummary>( h, l.resultsAt )[i];
        summaries[i] = { from.count, from.firstNl, from.tailStart, from.tailFieldStart, from.tailFieldEnd, from.headDelims,
                         from.tailDelims, ( from.info & FIELD_HAS_DELIMITER ) != 0 ? 1u : 0u,
                         ( from.info & FIELD_TAIL_NON_EMPTY ) != 0 ? 1u : 0u };
        const uint64_t listed = std::min<uint64_t>( from.headDelims, cap );
        if ( headPositions != nullptr ) std::copy_n( at<const uint64_t>( h, l.headsAt ) + i * cap, listed, headPositions + i * cap );
        if ( headTexts != nullptr ) {
            std::memcpy( headTexts + i * cap, h + l.headTextsAt + i * cap * FIELDNUM_TEXT_BYTES,
                         std::min( listed + 1, cap ) * FIELDNUM_TEXT_BYTES );
        }
        if ( tailTexts != nullptr ) std::memcpy( tailTexts + i, h + l.tailTextsAt + (uint64_t)i * FIELDNUM_TEXT_BYTES, FIELDNUM_TEXT_BYTES );
    }
    return MI355X_BZ2_OK;
}

static_assert( FIELDMATCH_VALUES == FIELDMATCH_MAX_VALUES && FIELDMATCH_VALUE_BYTES == FIELDMATCH_MAX_VALUE_BYTES
               && FIELDMATCH_BYTES == FIELDMATCH_MAX_BYTES && FIELDMATCH_IMAGE_WORDS * 4 == FIELDMATCH_IMAGE_MAX
               && FIELDMATCH_MAX_VALUES == SET_MAX_PATTERNS && FIELDMATCH_MAX_BYTES == SET_MAX_BYTES
               && ( 1u << FIELDMATCH_STEPS ) == FIELDMATCH_VALUES, "the kernel's constants are the host's, the caps the search set's" );

/**
 * mi355x_bz2_match_fields and the reader's launches.  The n lines' keys, starts and sizes are in device memory already --
 * the field-hash passes wrote them --, so only the table's image goes up; k_field_match writes dFlags[0, n), one word per
 * line.  A start counts from `base`, modulo 2^64: start - base is the field's offset in the output, and the kernel reads no
 * span that does not lie inside it.
 */
int
matchFields( mi355x_bz2_ctx* c, const char* what, const ValueTable& table, const uint64_t* dKeys, const uint64_t* dStarts,
             const int64_t* dSizes, uint64_t n, uint64_t base, uint64_t* dFlags )
{
    const std::scoped_lock lock( c->mutex );
    std::string why;
    if ( table.count() == 0 || table.count() > FIELDMATCH_MAX_VALUES || table.image.size() > FIELDMATCH_IMAGE_MAX
         || table.image.size() % 4 != 0 || table.image.size() < (uint64_t)table.count() * 12 + 4 ) {
        why = "the value table is not one of buildValueTable's";
    }
    if ( const int status = refuseQuery( c, what, nullptr, 0, why ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    HIP_TRY( c, hipSetDevice( c->device ) );
    const FieldMatchLayout l = layFieldMatch( table.image.size() );
    if ( const int status = growLineStaging( c, l.bytes, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    std::memcpy( h + l.imageAt, table.image.data(), table.image.size() );
    HIP_TRY( c, hipMemcpyAsync( d + l.imageAt, h + l.imageAt, table.image.size(), hipMemcpyHostToDevice, c->stream ) );
    const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( n + FIELDMATCH_THREADS - 1 ) / FIELDMATCH_THREADS, FIELDMATCH_BLOCKS );
    hipLaunchKernelGGL( k_field_match, dim3( blocks ), dim3( FIELDMATCH_THREADS ), 0, c->stream, at<const uint32_t>( d, l.imageAt ),
                        (uint32_t)( table.image.size() / 4 ), table.count(), dKeys, dStarts, dSizes, n, c->dOut, c->outSize, base, dFlags );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    return MI355X_BZ2_OK;
}

/**
 * mi355x_bz2_match_fields_regex and the reader's launches.  The n lines' starts and sizes are in device memory already --
 * the field-span passes wrote them --, so only the table and acceptsAtEnd go up: once per call of this launcher, which for
 * the reader is once per resident stretch, as matchFields sends its image (at most 16 KiB + 64 B, and the dead state is
 * found anew, 64 x 256 comparisons at the most; neither is kept on the context).  k_field_regex writes dFlags[0, n), one
 * word per line.  A start counts from `base`, modulo 2^64, as for matchFields.
 */
static_assert( REGEX_STATES == REGEX_MAX_STATES, "regexDeadState's `none` is a state that k_field_regex never reaches" );

int
matchFieldsRegex( mi355x_bz2_ctx* c, const char* what, const Regex& regex, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n,
                  uint64_t base, uint64_t* dFlags )
{
    const std::scoped_lock lock( c->mutex );
    const bool compiled = regex.n >= 2 && regex.n <= REGEX_MAX_STATES && regex.transitions.size() == (size_t)regex.n * 256
                          && regex.acceptsAtEnd.size() == regex.n;
    if ( const int status = refuseQuery( c, what, nullptr, 0, compiled ? "" : "not a compiled regular expression" ) ) return status;
    if ( n == 0 ) return MI355X_BZ2_OK;
    HIP_TRY( c, hipSetDevice( c->device ) );
    const FieldRegexLayout l = layFieldRegex( regex.n, REGEX_STATES );
    if ( const int status = growLineStaging( c, l.bytes, l.bytes ) ) return status;
    uint8_t* const h = c->hSearch.bytes;
    uint8_t* const d = c->dSearch.bytes;
    std::memset( h, 0, l.bytes );
    std::memcpy( h + l.tableAt, regex.transitions.data(), (size_t)regex.n * 256 );
    std::memcpy( h + l.acceptsAt, regex.acceptsAtEnd.data(), regex.n );
    HIP_TRY( c, hipMemcpyAsync( d, h, l.bytes, hipMemcpyHostToDevice, c->stream ) );
    const uint32_t blocks = (uint32_t)std::min<uint64_t>( ( n + FIELDREGEX_THREADS - 1 ) / FIELDREGEX_THREADS, FIELDREGEX_BLOCKS );
    hipLaunchKernelGGL( k_field_regex, dim3( blocks ), dim3( FIELDREGEX_THREADS ), 0, c->stream, d + l.tableAt, d + l.acceptsAt, regex.n,
                        regexDeadState( regex ), dStarts, dSizes, n, c->dOut, c->outSize, base, dFlags );
    HIP_TRY( c, hipGetLastError() );
    HIP_TRY( c, hipStreamSynchronize( c->stream ) );
    return MI355X_BZ2_OK;
}

/** The set of a C ABI call, checked: false with lastError set if it breaks a limit or `flags` has an unknown bit. */
bool
takeSet( mi355x_bz2_ctx* c, const char* what, const uint8_t* patterns, const uint32_t* sizes, uint32_t n, uint32_t flags,
         PatternSet* set )
{
    const std::scoped_lock lock( c->mutex );
    if ( unknownSearchFlags( c, what, flags ) ) return false;
    const auto why = patternSetError( sizes, n );
    if ( !why.empty() ) {
        refuse( c, what, why );
        return false;
    }
    *set = makePatternSet( patterns, sizes, n, ( flags & SEARCH_IGNORE_CASE ) != 0 );
    return true;
}

/** The field members of a span's C summary -- mi355x_bz2_field_summary, or mi355x_bz2_field_hash_summary, which repeats
 * them -- as the FieldSummary of a stretch of `size` bytes; `heads` has room for field + 1 head positions. */
template<typename CSummary>
void
setFieldSummary( bz2gpu::FieldSummary& f, const CSummary& s, uint64_t size, std::vector<uint64_t> heads )
{
    f.size = size;
    f.hasDelimiter = s.has_delimiter != 0;
    f.tailNonEmpty = s.tail_non_empty != 0;
    f.count = s.count;
    f.firstNl = s.first_nl;
    heads.resize( std::min<size_t>( s.head_delims, heads.size() ) );
    f.headPositions = std::move( heads );
    f.tailStart = s.tail_start;
    f.tailDelims = s.tail_delims;
    f.tailFieldStart = s.tail_field_start;
    f.tailFieldEnd = s.tail_field_end;
}
}  // namespace

int
mi355x::searchOutputSet( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, const bz2gpu::PatternSet& set, uint64_t limit,
                         std::vector<uint64_t>* positions, std::vector<uint32_t>* ids, uint64_t* count, uint64_t* perPattern,
                         uint8_t* seamBytes )
{
    if ( c == nullptr || count == nullptr || seamBytes == nullptr || ( positions == nullptr ) != ( ids == nullptr )
         || !patternSetError( set.sizes.data(), set.count() ).empty() ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return searchBytesSet( c, "search_set", &extent, 1, set, positions != nullptr ? limit : 0, { nullptr, positions, nullptr, ids },
                           count, perPattern, &extent, seamBytes );
}

int
mi355x::searchOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, const uint8_t* pattern, uint32_t m,
                      uint32_t flags, uint64_t limit, std::vector<uint64_t>* positions, uint64_t* count, uint8_t* seamBytes )
{
    if ( c == nullptr || pattern == nullptr || count == nullptr || seamBytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return searchBytes( c, "search", &extent, 1, pattern, m, flags, positions != nullptr ? limit : 0, nullptr, positions, count,
                        &extent, seamBytes );
}

int
mi355x::matchLinesOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, const bz2gpu::Regex& regex, uint8_t nl,
                          uint64_t limit, bz2gpu::StretchSummary* summary )
{
    if ( c == nullptr || summary == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    uint8_t hasDelimiter = 0, exitState = 0;
    summary->witnesses.clear();
    const int status = matchLines( c, "grep_regex", &extent, 1, regex, nl, summary->headMap.data(), &hasDelimiter, &exitState,
                                   limit, nullptr, &summary->witnesses, &summary->count );
    summary->hasDelimiter = hasDelimiter != 0;
    summary->exit = exitState;
    return status;
}

int
mi355x::hashLinesOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, uint8_t nl, uint64_t x, uint64_t skip,
                         uint64_t take, uint64_t* dHashes, bz2gpu::HashSummary* summary )
{
    if ( c == nullptr || summary == nullptr || ( take > 0 && dHashes == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    mi355x_bz2_line_hash_summary s{};
    const int status = hashLines( c, "line_hashes", &extent, 1, nl, x, &s, skip, take, dHashes );
    summary->head = { s.head_hash, s.head_xl };
    summary->tail = { s.tail_hash, s.tail_xl };
    summary->hasDelimiter = s.has_delimiter != 0;
    summary->tailNonEmpty = s.tail_non_empty != 0;
    summary->count = s.count;
    summary->hashes.clear();
    return status;
}

int
mi355x::fieldSpansOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                          uint32_t field, uint64_t skip, uint64_t take, uint64_t* dStarts, int64_t* dSizes,
                          bz2gpu::FieldSummary* summary )
{
    if ( c == nullptr || summary == nullptr || field > FIELD_MAX || ( take > 0 && ( dStarts == nullptr || dSizes == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    mi355x_bz2_field_summary s{};
    std::vector<uint64_t> heads( (size_t)field + 1 );
    const int status = fieldSpans( c, "field_spans", &extent, &fileOffset, 1, nl, dl, field, &s, heads.data(), skip, take, dStarts, dSizes );
    *summary = bz2gpu::emptyFieldSummary( field );
    if ( status != MI355X_BZ2_OK ) return status;
    setFieldSummary( *summary, s, extent.size, std::move( heads ) );
    return status;
}

int
mi355x::fieldSpansQuotedOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                                uint8_t quote, uint32_t field, uint64_t skip, uint64_t take, uint64_t* dStarts, int64_t* dSizes,
                                bz2gpu::QuotedFieldSummary* summary )
{
    if ( c == nullptr || summary == nullptr || field > FIELD_MAX || ( take > 0 && ( dStarts == nullptr || dSizes == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    mi355x_bz2_quoted_field_summary s{};
    const size_t cap = (size_t)field + 1;
    std::vector<uint64_t> heads( 2 * cap );
    const int status = fieldSpansQuoted( c, "field_spans", &extent, &fileOffset, 1, nl, dl, quote, field, &s, heads.data(), skip, take,
                                         dStarts, dSizes );
    *summary = bz2gpu::emptyQuotedFieldSummary( field );
    if ( status != MI355X_BZ2_OK ) return status;
    summary->size = extent.size;
    summary->hasDelimiter = s.has_delimiter != 0;
    summary->tailNonEmpty = s.tail_non_empty != 0;
    summary->count = s.count;
    summary->firstNl = s.first_nl;
    for ( size_t hypothesis = 0; hypothesis < 2; ++hypothesis ) {
        const auto first = heads.begin() + hypothesis * cap;
        summary->headPositions[hypothesis].assign( first, first + std::min<size_t>( s.head_delims[hypothesis], cap ) );
    }
    summary->headQuoteParity = s.head_quote_parity != 0;
    summary->tailStart = s.tail_start;
    summary->tailDelims = s.tail_delims;
    summary->tailFieldStart = s.tail_field_start;
    summary->tailFieldEnd = s.tail_field_end;
    summary->tailInQuote = s.tail_in_quote != 0;
    return status;
}

int
mi355x::fieldHashesOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                           uint32_t field, uint64_t x, uint64_t skip, uint64_t take, uint64_t* dKeys, uint64_t* dStarts,
                           int64_t* dSizes, bz2gpu::FieldHashSummary* summary )
{
    if ( c == nullptr || summary == nullptr || field > FIELD_MAX
         || ( take > 0 && ( dKeys == nullptr || dStarts == nullptr || dSizes == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    mi355x_bz2_field_hash_summary s{};
    std::vector<uint64_t> heads( (size_t)field + 1 ), headHashes( (size_t)field + 1 );
    const int status = fieldHashes( c, "field_hashes", &extent, &fileOffset, 1, nl, dl, field, x, &s, heads.data(), headHashes.data(),
                                    skip, take, dKeys, dStarts, dSizes );
    *summary = bz2gpu::emptyFieldHashSummary( field );
    if ( status != MI355X_BZ2_OK ) return status;
    setFieldSummary( summary->fields, s, extent.size, std::move( heads ) );
    headHashes.resize( summary->fields.headPositions.size() );
    summary->headHashes = std::move( headHashes );
    summary->head = { s.head_hash, s.head_xl };
    summary->tail = { s.tail_hash, s.tail_xl };
    summary->tailStartHash = s.tail_start_hash;
    summary->tailEndHash = s.tail_end_hash;
    return status;
}

int
mi355x::fieldNumbersOutput( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span& extent, uint64_t fileOffset, uint8_t nl, uint8_t dl,
                            uint32_t field, uint64_t skip, uint64_t take, int64_t* dNumbers, uint64_t* dStarts, int64_t* dSizes,
                            bz2gpu::FieldNumberSummary* summary )
{
    if ( c == nullptr || summary == nullptr || field > FIELD_MAX || ( take > 0 && dNumbers == nullptr )
         || ( dStarts == nullptr ) != ( dSizes == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    mi355x_bz2_field_summary s{};
    std::vector<uint64_t> heads( (size_t)field + 1 );
    std::vector<mi355x_bz2_field_text> headTexts( (size_t)field + 1 );
    mi355x_bz2_field_text tailText{};
    const int status = fieldNumbers( c, "field_numbers", &extent, &fileOffset, 1, nl, dl, field, &s, heads.data(), headTexts.data(),
                                     &tailText, skip, take, dNumbers, dStarts, dSizes );
    *summary = bz2gpu::emptyFieldNumberSummary( field );
    if ( status != MI355X_BZ2_OK ) return status;
    setFieldSummary( summary->fields, s, extent.size, std::move( heads ) );
    summary->headTexts.resize( bz2gpu::headTextCount( summary->fields.headDelims(), field ) );
    std::memcpy( summary->headTexts.data(), headTexts.data(), summary->headTexts.size() * sizeof( FieldText ) );
    std::memcpy( &summary->tailText, &tailText, sizeof( FieldText ) );
    return status;
}

int
mi355x::matchFieldsOutput( mi355x_bz2_ctx* c, const bz2gpu::ValueTable& table, const uint64_t* dKeys, const uint64_t* dStarts,
                           const int64_t* dSizes, uint64_t n, uint64_t srcOffset, uint64_t fileOffset, uint64_t* dFlags )
{
    if ( c == nullptr || ( n > 0 && ( dKeys == nullptr || dStarts == nullptr || dSizes == nullptr || dFlags == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    /* modulo 2^64, as gatherFieldsOutput has it */
    return matchFields( c, "field_matches", table, dKeys, dStarts, dSizes, n, fileOffset - srcOffset, dFlags );
}

int
mi355x::matchFieldsRegexOutput( mi355x_bz2_ctx* c, const bz2gpu::Regex& regex, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n,
                                uint64_t srcOffset, uint64_t fileOffset, uint64_t* dFlags )
{
    if ( c == nullptr || ( n > 0 && ( dStarts == nullptr || dSizes == nullptr || dFlags == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    /* modulo 2^64, as gatherFieldsOutput has it */
    return matchFieldsRegex( c, "field_matches_regex", regex, dStarts, dSizes, n, fileOffset - srcOffset, dFlags );
}

int
mi355x::gatherFieldsOutput( mi355x_bz2_ctx* c, const uint64_t* dStarts, const int64_t* dSizes, uint64_t n, uint64_t srcOffset,
                            uint64_t fileOffset, uint64_t* dOffsets, const std::function<uint8_t*( uint64_t )>& allocate,
                            uint64_t* total, uint64_t* firstSize )
{
    if ( c == nullptr || total == nullptr || dOffsets == nullptr || ( n > 0 && ( dStarts == nullptr || dSizes == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    /* modulo 2^64: start - ( fileOffset - srcOffset ) = srcOffset + ( start - fileOffset ) */
    return gatherFields( c, "field_columns", dStarts, dSizes, n, fileOffset - srcOffset, dOffsets, [&] ( uint64_t bytes, uint8_t** dst ) {
        *dst = bytes > 0 ? allocate( bytes ) : nullptr;
        return bytes == 0 || *dst != nullptr;
    }, total, firstSize );
}

int
mi355x::gatherResult( mi355x_bz2_ctx* c, const mi355x_bz2_gather_piece* pieces, uint32_t nPieces, void* dst, int dstIsDevice )
{
    if ( c == nullptr || ( nPieces > 0 && pieces == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    const std::scoped_lock lock( c->mutex );
    return gatherPieces( c, c->result.bytes, c->result.capacity, pieces, nPieces, dst, dstIsDevice );
}

extern "C" {

int
mi355x_bz2_gather_output( mi355x_bz2_ctx* c, const mi355x_bz2_gather_piece* pieces, uint32_t nPieces, void* dst,
                          int dstIsDevice )
{
    if ( c == nullptr || ( nPieces > 0 && pieces == nullptr ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    const std::scoped_lock lock( c->mutex );
    if ( const int status = refuseQuery( c, "gather_output", nullptr, 0 ) ) return status;
    return gatherPieces( c, c->dOut, c->outSize, pieces, nPieces, dst, dstIsDevice );
}

int
mi355x_bz2_count_byte( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t value, uint64_t* counts )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || counts == nullptr ) ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return selectBytes( c, "count_byte", value, n, spans, nullptr, counts );
}

int
mi355x_bz2_find_byte( mi355x_bz2_ctx* c, const mi355x_bz2_byte_query* queries, uint32_t n, uint8_t value,
                      uint64_t* positions )
{
    if ( c == nullptr || ( n > 0 && ( queries == nullptr || positions == nullptr ) ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    std::vector<mi355x_bz2_byte_span> spans( n );
    std::vector<uint64_t> ranks( n );
    for ( uint32_t i = 0; i < n; ++i ) {
        spans[i] = { queries[i].offset, queries[i].size };
        ranks[i] = queries[i].rank;
    }
    return selectBytes( c, "find_byte", value, n, spans.data(), ranks.data(), positions );
}

int
mi355x_bz2_rank_byte( mi355x_bz2_ctx* c, const mi355x_bz2_rank_query* queries, uint32_t n, uint8_t value, uint64_t* ranks )
{
    if ( c == nullptr || ( n > 0 && ( queries == nullptr || ranks == nullptr ) ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return rankBytes( c, queries, n, value, ranks );
}

int
mi355x_bz2_count_bytes_ex( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                           uint32_t patternSize, uint32_t flags, uint64_t* counts )
{
    if ( c == nullptr || pattern == nullptr || ( n > 0 && ( spans == nullptr || counts == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return searchBytes( c, "count_bytes", spans, n, pattern, patternSize, flags, 0, nullptr, nullptr, counts, nullptr, nullptr );
}

int
mi355x_bz2_count_bytes( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                        uint32_t patternSize, uint64_t* counts )
{
    return mi355x_bz2_count_bytes_ex( c, spans, n, pattern, patternSize, 0, counts );
}

int
mi355x_bz2_find_bytes_ex( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                          uint32_t patternSize, uint32_t flags, uint64_t* positions, uint64_t capacity, uint64_t* counts )
{
    if ( c == nullptr || pattern == nullptr || ( n > 0 && ( spans == nullptr || counts == nullptr ) )
         || ( capacity > 0 && positions == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return searchBytes( c, "find_bytes", spans, n, pattern, patternSize, flags, capacity, positions, nullptr, counts, nullptr,
                        nullptr );
}

int
mi355x_bz2_find_bytes( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* pattern,
                       uint32_t patternSize, uint64_t* positions, uint64_t capacity, uint64_t* counts )
{
    return mi355x_bz2_find_bytes_ex( c, spans, n, pattern, patternSize, 0, positions, capacity, counts );
}

int
mi355x_bz2_match_lines( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const mi355x_bz2_regex* re, uint8_t nl,
                        uint8_t* headMaps, uint8_t* hasDelimiter, uint8_t* exitStates, uint64_t* positions, uint64_t capacity,
                        uint64_t* counts )
{
    if ( c == nullptr || re == nullptr
         || ( n > 0 && ( spans == nullptr || headMaps == nullptr || hasDelimiter == nullptr || exitStates == nullptr || counts == nullptr ) )
         || ( capacity > 0 && positions == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return matchLines( c, "match_lines", spans, n, re->dfa, nl, headMaps, hasDelimiter, exitStates, capacity, positions, nullptr,
                       counts );
}

int
mi355x_bz2_hash_lines( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint64_t seed,
                       mi355x_bz2_line_hash_summary* summaries, uint64_t* hashesDevice, uint64_t capacity )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || summaries == nullptr ) ) || ( capacity > 0 && hashesDevice == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return hashLines( c, "hash_lines", spans, n, nl, lineHashBase( seed ), summaries, 0, capacity, hashesDevice );
}

int
mi355x_bz2_field_spans( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl, uint32_t field,
                        mi355x_bz2_field_summary* summaries, uint64_t* headPositions, uint64_t* startsDevice,
                        int64_t* sizesDevice, uint64_t capacity )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || summaries == nullptr ) )
         || ( capacity > 0 && ( startsDevice == nullptr || sizesDevice == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return fieldSpans( c, "field_spans", spans, nullptr, n, nl, dl, field, summaries, headPositions, 0, capacity, startsDevice,
                       sizesDevice );
}

int
mi355x_bz2_field_spans_quoted( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl, uint8_t quote,
                               uint32_t field, mi355x_bz2_quoted_field_summary* summaries, uint64_t* headPositions,
                               uint64_t* startsDevice, int64_t* sizesDevice, uint64_t capacity )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || summaries == nullptr ) )
         || ( capacity > 0 && ( startsDevice == nullptr || sizesDevice == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return fieldSpansQuoted( c, "field_spans_quoted", spans, nullptr, n, nl, dl, quote, field, summaries, headPositions, 0, capacity,
                             startsDevice, sizesDevice );
}

int
mi355x_bz2_gather_fields( mi355x_bz2_ctx* c, const uint64_t* startsDevice, const int64_t* sizesDevice, uint64_t n, uint64_t base,
                          uint64_t* offsetsDevice, void* dstDevice, uint64_t dstCapacity, uint64_t* total )
{
    if ( c == nullptr || total == nullptr || offsetsDevice == nullptr || ( n > 0 && ( startsDevice == nullptr || sizesDevice == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return gatherFields( c, "gather_fields", startsDevice, sizesDevice, n, base, offsetsDevice, [=] ( uint64_t bytes, uint8_t** dst ) {
        *dst = bytes <= dstCapacity ? static_cast<uint8_t*>( dstDevice ) : nullptr;
        return true;
    }, total );
}

int
mi355x_bz2_match_fields( mi355x_bz2_ctx* c, const uint8_t* values, const uint32_t* valueSizes, uint32_t nValues, uint64_t seed,
                         const uint64_t* keysDevice, const uint64_t* startsDevice, const int64_t* sizesDevice, uint64_t n, uint64_t base,
                         uint64_t* flagsDevice )
{
    if ( c == nullptr || ( nValues > 0 && valueSizes == nullptr )
         || ( n > 0 && ( keysDevice == nullptr || startsDevice == nullptr || sizesDevice == nullptr || flagsDevice == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    ValueTable table;
    try {
        const auto why = valueSetError( valueSizes, nValues );
        if ( why.empty() && values == nullptr && std::any_of( valueSizes, valueSizes + nValues, [] ( uint32_t size ) { return size > 0; } ) ) {
            return MI355X_BZ2_ERR_INVALID_ARGUMENT;
        }
        table = valueTableOf( values, valueSizes, nValues, seed );
    } catch ( const std::invalid_argument& refused ) {
        const std::scoped_lock lock( c->mutex );
        return refuse( c, "match_fields", refused.what() );
    } catch ( const std::exception& failed ) {
        const std::scoped_lock lock( c->mutex );
        c->lastError = std::string( "match_fields: " ) + failed.what();
        return MI355X_BZ2_ERR_DEVICE;
    }
    return matchFields( c, "match_fields", table, keysDevice, startsDevice, sizesDevice, n, base, flagsDevice );
}

int
mi355x_bz2_match_fields_regex( mi355x_bz2_ctx* c, const mi355x_bz2_regex* re, const uint64_t* startsDevice, const int64_t* sizesDevice,
                               uint64_t n, uint64_t base, uint64_t* flagsDevice )
{
    if ( c == nullptr || re == nullptr || ( n > 0 && ( startsDevice == nullptr || sizesDevice == nullptr || flagsDevice == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return matchFieldsRegex( c, "match_fields_regex", re->dfa, startsDevice, sizesDevice, n, base, flagsDevice );
}

int
mi355x_bz2_field_hashes( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl, uint32_t field,
                         uint64_t seed, mi355x_bz2_field_hash_summary* summaries, uint64_t* headPositions, uint64_t* headHashes,
                         uint64_t* hashesDevice, uint64_t* startsDevice, int64_t* sizesDevice, uint64_t capacity )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || summaries == nullptr ) ) || ( capacity > 0 && hashesDevice == nullptr )
         || ( startsDevice == nullptr ) != ( sizesDevice == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return fieldHashes( c, "field_hashes", spans, nullptr, n, nl, dl, field, lineHashBase( seed ), summaries, headPositions, headHashes,
                        0, capacity, hashesDevice, startsDevice, sizesDevice );
}

int
mi355x_bz2_field_numbers( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, uint8_t nl, uint8_t dl, uint32_t field,
                          mi355x_bz2_field_summary* summaries, uint64_t* headPositions, mi355x_bz2_field_text* headTexts,
                          mi355x_bz2_field_text* tailTexts, int64_t* numbersDevice, uint64_t* startsDevice, int64_t* sizesDevice,
                          uint64_t capacity )
{
    if ( c == nullptr || ( n > 0 && ( spans == nullptr || summaries == nullptr ) ) || ( capacity > 0 && numbersDevice == nullptr )
         || ( startsDevice == nullptr ) != ( sizesDevice == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    return fieldNumbers( c, "field_numbers", spans, nullptr, n, nl, dl, field, summaries, headPositions, headTexts, tailTexts, 0,
                         capacity, numbersDevice, startsDevice, sizesDevice );
}

int
mi355x_bz2_count_bytes_set_ex( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                               const uint32_t* patternSizes, uint32_t nPatterns, uint32_t flags, uint64_t* counts,
                               uint64_t* perPattern )
{
    if ( c == nullptr || patterns == nullptr || patternSizes == nullptr || ( n > 0 && ( spans == nullptr || counts == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    PatternSet set;
    if ( !takeSet( c, "count_bytes_set", patterns, patternSizes, nPatterns, flags, &set ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return searchBytesSet( c, "count_bytes_set", spans, n, set, 0, {}, counts, perPattern, nullptr, nullptr );
}

int
mi355x_bz2_count_bytes_set( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                            const uint32_t* patternSizes, uint32_t nPatterns, uint64_t* counts, uint64_t* perPattern )
{
    return mi355x_bz2_count_bytes_set_ex( c, spans, n, patterns, patternSizes, nPatterns, 0, counts, perPattern );
}

int
mi355x_bz2_find_bytes_set_ex( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                              const uint32_t* patternSizes, uint32_t nPatterns, uint32_t flags, uint64_t* positions,
                              uint32_t* ids, uint64_t capacity, uint64_t* counts, uint64_t* perPattern )
{
    if ( c == nullptr || patterns == nullptr || patternSizes == nullptr || ( n > 0 && ( spans == nullptr || counts == nullptr ) )
         || ( capacity > 0 && ( positions == nullptr || ids == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    PatternSet set;
    if ( !takeSet( c, "find_bytes_set", patterns, patternSizes, nPatterns, flags, &set ) ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    return searchBytesSet( c, "find_bytes_set", spans, n, set, capacity, { positions, nullptr, ids }, counts, perPattern,
                           nullptr, nullptr );
}

int
mi355x_bz2_find_bytes_set( mi355x_bz2_ctx* c, const mi355x_bz2_byte_span* spans, uint32_t n, const uint8_t* patterns,
                           const uint32_t* patternSizes, uint32_t nPatterns, uint64_t* positions, uint32_t* ids,
                           uint64_t capacity, uint64_t* counts, uint64_t* perPattern )
{
    return mi355x_bz2_find_bytes_set_ex( c, spans, n, patterns, patternSizes, nPatterns, 0, positions, ids, capacity, counts,
                                         perPattern );
}

}  // extern "C"
