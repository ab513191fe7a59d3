/**
 * bz2_fields.hip.h -- where field j of every line lies, for spans of a batch's ragged output: the kernels under
 * mi355x_bz2_field_spans, i.e. under the reader's field_spans and read_fields.  bz2_fields.hpp has the definition (field
 * j starts behind the j-th dl byte of its line and ends at the next dl or at the nl), the summary of a stretch and the
 * rule that composes summaries; these kernels apply that rule between the chunks of a tile and between the tiles of a
 * span.
 *
 * The tiling and the staging are the line-hash kernels' (bz2_linehash.hip.h: lhStage, and why the bytes go through LDS):
 * a span is cut into tiles of COUNT_TILE bytes, a tile into FIELD_THREADS chunks of FIELD_CHUNK bytes, one lane per
 * chunk, one workgroup per tile; chunk k of tile t is slot t * FIELD_THREADS + k of the per-chunk arrays.
 *
 * What is scanned.  All a chunk must know about the bytes in front of it is how many dl bytes the line that is open at
 * its first byte has passed, and no more exactly than "j + 1 or more".  A stretch acts on that count as one 32-bit
 * element: FIELD_RESET says that it holds an nl, the low bits count the dl bytes behind its last nl (all of them
 * without one), saturated at cap = j + 1.  first . second = second if second resets, else first with second's count
 * added and saturated: associative, so it is scanned, on two levels as the line hashes are.
 *
 *   k_field_chunks  per chunk: its element and its number of nl bytes; then the tile's 256 elements are scanned in LDS.
 *                   Written per chunk: its EXCLUSIVE prefix within the tile and its count; per tile: its element, its
 *                   count and whether its last byte is an nl.
 *   k_field_link    one workgroup per span scans the TILE elements, FIELD_THREADS tiles per step with one carry element
 *                   between steps.  Every tile gets the count its first line is entered with (the span itself is entered
 *                   at a line start); the span's count of closed lines, hasDelimiter, tailNonEmpty and tailDelims are
 *                   written, and the members that k_field_emit may not reach are set to their "not reached" values.
 *   k_scan_tiles    (bz2_search.hip.h) the exclusive prefix sums of the chunk counts: the place of every chunk's first
 *                   closed line.
 *   k_field_emit    re-walks each chunk from its entering count.  Where the j-th dl of a line is passed (for j = 0: where
 *                   the line starts) the field's start goes to starts[place]; at the ( j + 1 )-th dl, or at an nl reached
 *                   with exactly j, its END goes to sizes[place]; an nl reached with fewer stores the nl's offset and -1.
 *                   Every closed line so gets one store to each array, from whichever chunks see the two events.  The
 *                   same events in the span's unclosed tail go to the span's summary instead, and the dl bytes in front
 *                   of the span's first nl to its head positions: what the host needs to patch the one line per seam.
 *   k_field_sizes   sizes[i] -= starts[i] wherever sizes[i] holds an end.
 *
 * Every store to starts and sizes goes to the line's place, less `skip`: nothing is written in front of `skip` or at or
 * beyond skip + capacity, and a tile none of whose lines lie there, and which touches neither the head nor the tail of
 * its span, returns at once.  Places, slots and offsets are 64 bit.  Every loop is bounded by the chunk, by the number of
 * tiles or by the number of lines; no workgroup waits on another; vector stores only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_linehash.hip.h"

namespace bz2gpu
{
constexpr uint32_t FIELD_CHUNK = LINEHASH_CHUNK;
constexpr uint32_t FIELD_THREADS = LINEHASH_THREADS;        /* chunks per tile, tiles per step of the link */
constexpr uint32_t FIELD_RESET = 0x80000000u;               /* in an element: the stretch holds an nl */
constexpr uint32_t FIELD_HAS_DELIMITER = 1, FIELD_TAIL_NON_EMPTY = 2;
constexpr uint64_t FIELD_NOT_REACHED = ~uint64_t( 0 );
constexpr uint32_t FIELD_SIZES_THREADS = 256, FIELD_SIZES_BLOCKS = 2048;

/** What k_field_chunks leaves per tile and k_field_link completes. */
struct FieldTile
{
    uint32_t element;     /* of the whole tile */
    uint32_t count;       /* its nl bytes */
    uint32_t info;        /* FIELD_TAIL_NON_EMPTY */
    uint32_t entry;       /* k_field_link: the dl bytes the line open at the tile's first byte has passed, saturated */
};

/** What the kernels are told about a span: its tiles, and the value that stands for its first byte in `starts`. */
struct FieldSpanTiles
{
    uint64_t firstTile, nTiles, base;
};

/** A span's summary as the kernels leave it; positions are relative to the span. */
struct FieldSpanSummary
{
    uint64_t count, firstNl, tailStart, tailFieldStart, tailFieldEnd;
    uint32_t headDelims, tailDelims, info, unused;
};

/** `first` followed by `second`, counts saturated at `cap`. */
__device__ __forceinline__ uint32_t
fdCompose( uint32_t first, uint32_t second, uint32_t cap )
{
    if ( ( second & FIELD_RESET ) != 0 ) return second;
    const uint32_t sum = ( first & ~FIELD_RESET ) + second;
    return ( first & FIELD_RESET ) | ( sum < cap ? sum : cap );
}

/** Inclusive scan of the workgroup's FIELD_THREADS elements in LDS; every lane calls it. */
__device__ __forceinline__ void
fdScan( uint32_t* elements, uint32_t tid, uint32_t cap )
{
    for ( uint32_t d = 1; d < FIELD_THREADS; d <<= 1 ) {
        uint32_t composed = elements[tid];
        if ( tid >= d ) composed = fdCompose( elements[tid - d], composed, cap );
        __syncthreads();
        elements[tid] = composed;
        __syncthreads();
    }
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_field_chunks( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint32_t nl, uint32_t dl, uint32_t cap,
                uint32_t* __restrict__ prefixes, uint32_t* __restrict__ counts, FieldTile* __restrict__ tileSummaries )
{
    __shared__ uint32_t stage[FIELD_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    __shared__ uint32_t elements[FIELD_THREADS];
    __shared__ uint32_t tileCount;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CountTile t = tiles[blockIdx.x];
    if ( tid == 0 ) tileCount = 0;

    const uint64_t slot = (uint64_t)blockIdx.x * FIELD_THREADS + tid;
    const uint32_t begin = tid * FIELD_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < FIELD_CHUNK ? t.size - begin : FIELD_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );

    /* the dl bytes since the chunk's last nl: at most FIELD_CHUNK, saturated behind the walk */
    uint32_t delims = 0, count = 0, last = nl;
    for ( uint32_t pass = 0; pass < LINEHASH_PASSES; ++pass ) {
        lhStage( t, out, stage[wave], wave, lane, pass );
        __syncthreads();
        const uint32_t done = pass * LINEHASH_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < LINEHASH_PIECE ? chunkSize - done : LINEHASH_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            last = row[i];
            if ( last == nl ) {
                ++count;
                delims = 0;
            } else if ( last == dl ) {
                ++delims;
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
    elements[tid] = ( count != 0 ? FIELD_RESET : 0u ) | ( delims < cap ? delims : cap );
    if ( count != 0 ) atomicAdd( &tileCount, count );
    __syncthreads();
    fdScan( elements, tid, cap );

    prefixes[slot] = tid > 0 ? elements[tid - 1] : 0u;
    counts[slot] = count;
    FieldTile* const summary = tileSummaries + blockIdx.x;
    if ( tid == FIELD_THREADS - 1 ) {
        summary->element = elements[tid];
        summary->count = tileCount;
        summary->entry = 0;
    }
    /* the lane that holds the tile's last byte (a tile is never empty) */
    if ( tid == ( t.size - 1 ) / FIELD_CHUNK ) summary->info = last != nl ? FIELD_TAIL_NON_EMPTY : 0u;
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_field_link( const FieldSpanTiles* __restrict__ spans, FieldTile* __restrict__ tileSummaries,
              FieldSpanSummary* __restrict__ spanSummaries, uint32_t field )
{
    __shared__ uint32_t elements[FIELD_THREADS];
    __shared__ uint32_t carry;
    __shared__ unsigned long long total;
    const uint32_t tid = threadIdx.x, cap = field + 1;
    const FieldSpanTiles span = spans[blockIdx.x];
    if ( tid == 0 ) {
        carry = 0;
        total = 0;
    }
    __syncthreads();

    unsigned long long sum = 0;
    uint32_t lastInfo = 0;
    for ( uint64_t t0 = 0; t0 < span.nTiles; t0 += FIELD_THREADS ) {
        const uint32_t n = span.nTiles - t0 < FIELD_THREADS ? (uint32_t)( span.nTiles - t0 ) : FIELD_THREADS;
        FieldTile* const tile = tileSummaries + span.firstTile + t0 + tid;
        uint32_t own = 0;
        if ( tid < n ) {
            own = tile->element;
            sum += tile->count;
            if ( t0 + tid + 1 == span.nTiles ) lastInfo = tile->info;
        }
        elements[tid] = own;
        __syncthreads();
        fdScan( elements, tid, cap );

        if ( tid < n ) {
            const uint32_t before = tid > 0 ? fdCompose( carry, elements[tid - 1], cap ) : carry;
            tile->entry = before & ~FIELD_RESET;
        }
        __syncthreads();
        if ( tid == 0 ) carry = fdCompose( carry, elements[n - 1], cap );
        __syncthreads();
    }

    if ( sum != 0 ) atomicAdd( &total, sum );
    /* the lane that saw the span's last tile; lane 0 of an empty span */
    const bool closes = span.nTiles == 0 ? tid == 0 : tid == ( span.nTiles - 1 ) % FIELD_THREADS;
    __syncthreads();
    if ( closes ) {
        FieldSpanSummary* const summary = spanSummaries + blockIdx.x;
        summary->count = total;
        summary->firstNl = FIELD_NOT_REACHED;
        summary->tailStart = 0;
        /* field 0 starts where its line starts: k_field_emit moves this behind the span's last nl */
        summary->tailFieldStart = field == 0 ? 0 : FIELD_NOT_REACHED;
        summary->tailFieldEnd = FIELD_NOT_REACHED;
        summary->headDelims = carry & ~FIELD_RESET;      /* without an nl; with one, k_field_emit knows */
        summary->tailDelims = carry & ~FIELD_RESET;
        summary->info = ( ( carry & FIELD_RESET ) != 0 ? FIELD_HAS_DELIMITER : 0u ) | ( lastInfo & FIELD_TAIL_NON_EMPTY );
        summary->unused = 0;
    }
}

/** Where k_field_emit's stores go. */
struct FieldSink
{
    uint64_t skip, capacity, base, spanEnd;
    uint64_t* starts;
    int64_t* sizes;
    FieldSpanSummary* summary;
};

/** Field j of line `line` starts at `p` of the span. */
__device__ __forceinline__ void
fdStart( const FieldSink& to, uint64_t line, uint64_t p )
{
    if ( line == to.spanEnd ) {
        to.summary->tailFieldStart = p;
    } else if ( line - to.skip < to.capacity ) {    /* a line in front of `skip` wraps to one beyond every capacity */
        to.starts[line - to.skip] = to.base + p;
    }
}

/** Field j of line `line` ends at `p` of the span. */
__device__ __forceinline__ void
fdEnd( const FieldSink& to, uint64_t line, uint64_t p )
{
    if ( line == to.spanEnd ) {
        to.summary->tailFieldEnd = p;
    } else if ( line - to.skip < to.capacity ) {
        to.sizes[line - to.skip] = (int64_t)( to.base + p );
    }
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_field_emit( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint32_t nl, uint32_t dl, uint32_t field,
              const FieldSpanTiles* __restrict__ spans, const uint32_t* __restrict__ prefixes,
              const FieldTile* __restrict__ tileSummaries, const uint64_t* __restrict__ places, FieldSpanSummary* spanSummaries,
              uint64_t* __restrict__ headPositions, uint64_t skip, uint64_t capacity, uint64_t* __restrict__ starts,
              int64_t* __restrict__ sizes )
{
    __shared__ uint32_t stage[FIELD_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    const CountTile t = tiles[blockIdx.x];
    const FieldSpanTiles span = spans[t.span];
    const FieldTile tile = tileSummaries[blockIdx.x];
    const uint32_t cap = field + 1;
    /* the same in every lane: the places ascend with the slots */
    const uint64_t spanFirst = places[span.firstTile * FIELD_THREADS];
    const uint64_t tileFirst = places[(uint64_t)blockIdx.x * FIELD_THREADS];
    FieldSink to{ skip, capacity, span.base, spanFirst + spanSummaries[t.span].count, starts, sizes, spanSummaries + t.span };
    const bool outside = ( tileFirst >= skip && tileFirst - skip >= capacity ) || tileFirst + tile.count < skip;
    if ( outside && tileFirst != spanFirst && tileFirst + tile.count != to.spanEnd ) return;

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t slot = (uint64_t)blockIdx.x * FIELD_THREADS + tid;
    const uint32_t begin = tid * FIELD_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < FIELD_CHUNK ? t.size - begin : FIELD_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );
    uint64_t* const heads = headPositions + (uint64_t)t.span * cap;

    const uint32_t before = prefixes[slot];
    uint32_t c = before & ~FIELD_RESET;
    if ( ( before & FIELD_RESET ) == 0 ) c = tile.entry + c < cap ? tile.entry + c : cap;
    uint64_t place = places[slot];
    /* of the chunk's first byte in its span */
    const uint64_t chunkAt = ( (uint64_t)blockIdx.x - span.firstTile ) * COUNT_TILE + begin;
    if ( field == 0 && chunkAt == 0 ) fdStart( to, place, 0 );
    for ( uint32_t pass = 0; pass < LINEHASH_PASSES; ++pass ) {
        lhStage( t, out, stage[wave], wave, lane, pass );
        __syncthreads();
        const uint32_t done = pass * LINEHASH_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < LINEHASH_PIECE ? chunkSize - done : LINEHASH_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            const uint32_t b = row[i];
            const uint64_t p = chunkAt + done + i;
            if ( b == nl ) {
                /* an nl closes a line of the span: place < spanEnd */
                if ( c < field ) {
                    if ( place - skip < capacity ) {
                        starts[place - skip] = span.base + p;
                        sizes[place - skip] = -1;
                    }
                } else if ( c == field ) {
                    fdEnd( to, place, p );
                }
                if ( place == spanFirst ) {
                    to.summary->firstNl = p;
                    to.summary->headDelims = c;
                }
                ++place;
                c = 0;
                if ( place == to.spanEnd ) to.summary->tailStart = p + 1;
                if ( field == 0 ) fdStart( to, place, p + 1 );
            } else if ( b == dl && c <= field ) {
                if ( place == spanFirst ) heads[c] = p;
                if ( c == field ) fdEnd( to, place, p );
                ++c;
                if ( c == field ) fdStart( to, place, p + 1 );
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
}

/** Behind k_field_emit: sizes[i] holds field i's end, or -1; its size is the end less its start.  The number of closed
 * lines is read where k_scan_tiles left it. */
__global__ __launch_bounds__( FIELD_SIZES_THREADS ) void
k_field_sizes( const uint64_t* __restrict__ places, const uint32_t* __restrict__ counts, uint64_t slots, uint64_t skip,
               uint64_t capacity, const uint64_t* __restrict__ starts, int64_t* __restrict__ sizes )
{
    const uint64_t total = places[slots - 1] + counts[slots - 1];
    const uint64_t n = total > skip ? ( total - skip < capacity ? total - skip : capacity ) : 0;
    for ( uint64_t i = (uint64_t)blockIdx.x * FIELD_SIZES_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELD_SIZES_THREADS ) {
        const int64_t end = sizes[i];
        if ( end >= 0 ) sizes[i] = end - (int64_t)starts[i];
    }
}
}  // namespace bz2gpu
