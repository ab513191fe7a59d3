/**
 * bz2_fieldquote.hip.h -- where field j of every line lies when fields may be quoted: the kernels under
 * mi355x_bz2_field_spans_quoted, i.e. under the quote= of the reader's field_spans, read_fields and read_columns.
 * bz2_fieldquote.hpp has the definition (every quote byte toggles, a dl inside quotes does not part, the nl always
 * closes), the summary of a stretch and the rule that composes summaries.  These are the quoted twins of
 * bz2_fields.hip.h's kernels, which stay as they are: tiling, staging, slots, FieldTile, FieldSpanTiles, FieldSink and
 * k_field_sizes are shared, and k_scan_tiles places the lines.
 *
 * What is scanned.  Whether a dl counts depends on the quote state, and a chunk does not know the state it is entered
 * with.  So a stretch acts as one 32-bit element that answers for both: FIELD_RESET says that it holds an nl, FQ_PARITY
 * is the parity of the q bytes behind its last nl (of all of them without one), bits 0..10 hold a0, the counted dl bytes
 * behind the last nl when the stretch is entered OUTSIDE quotes, bits 11..21 a1, the same when it is entered INSIDE; both
 * saturated at cap = j + 1 <= 1024, and a1 == a0 with a reset, since a line starts outside quotes.  first . second =
 * second if second resets; else first's reset, the parities xored, and to each of first's counts the count of second
 * under the state first leaves it in: p entered outside, and entered inside !p, or p too if first resets.  Associative
 * (tests/native/fields_quoted_cases.cpp walks random splits), so it is scanned on two levels as the unquoted element is.
 *
 *   k_field_chunks_quoted  per chunk: one walk with two counters and one parity gives the element and the nl bytes; then
 *                          the tile's scan.  Written as k_field_chunks writes.
 *   k_field_link_quoted    as k_field_link; a tile's `entry` is the whole entering element, since the tiles in front of
 *                          a span's first nl need the counts of both hypotheses.  Of the span's summary it writes what
 *                          needs no walk: count, the tail's delimiters and quote state, and the head members of a span
 *                          without an nl.
 *   k_field_emit_quoted    re-walks each chunk from ( c, inq ), the entering element under "the span is entered
 *                          outside", and counts a dl only while inq == 0: events and stores are k_field_emit's.  While
 *                          its line is the span's first it also carries ( c1, !inq ), the state under "entered inside",
 *                          and records the head positions of that hypothesis; nothing else is stored from it.
 *   k_field_sizes          as it is: ends to sizes.
 *   k_field_unquote        one lane per line of [skip, skip + capacity), grid-stride: a field of 2 bytes or more whose
 *                          first and last bytes in the resident output are both q loses them.  Two scattered byte loads
 *                          per such line.  The line's span -- its offset in the output, the value its starts count from
 *                          -- is found by bisecting the spans' first places.
 *
 * Places, slots and offsets are 64 bit.  Every loop is bounded by the chunk, by the number of tiles, of lines or by
 * log2 of the spans; no workgroup waits on another; vector stores only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_fields.hip.h"

namespace bz2gpu
{
constexpr uint32_t FQ_PARITY = 0x40000000u;                 /* in an element: an odd number of q bytes behind the last nl */
constexpr uint32_t FQ_COUNT_BITS = 11, FQ_COUNT_MASK = ( 1u << FQ_COUNT_BITS ) - 1;
constexpr uint32_t FIELD_TAIL_IN_QUOTE = 4;                 /* beside FIELD_HAS_DELIMITER and FIELD_TAIL_NON_EMPTY */
constexpr uint32_t FIELD_UNQUOTE_THREADS = 256, FIELD_UNQUOTE_BLOCKS = 2048;

/** A span's summary as the quoted kernels leave it; positions are relative to the span. */
struct QuotedFieldSpanSummary
{
    uint64_t count, firstNl, tailStart, tailFieldStart, tailFieldEnd;
    uint32_t headDelims[2], tailDelims, info, headQuoteParity, unused;
};

__device__ __forceinline__ uint32_t
fqCount0( uint32_t element )
{
    return element & FQ_COUNT_MASK;
}

__device__ __forceinline__ uint32_t
fqCount1( uint32_t element )
{
    return ( element >> FQ_COUNT_BITS ) & FQ_COUNT_MASK;
}

/** `first` followed by `second`, counts saturated at `cap`. */
__device__ __forceinline__ uint32_t
fqCompose( uint32_t first, uint32_t second, uint32_t cap )
{
    if ( ( second & FIELD_RESET ) != 0 ) return second;
    /* the state `second` is entered with when `first` is entered outside ( e0 ) and inside ( e1 ) */
    const bool e0 = ( first & FQ_PARITY ) != 0, e1 = ( first & FIELD_RESET ) != 0 ? e0 : !e0;
    const uint32_t s0 = fqCount0( second ), s1 = fqCount1( second );
    const uint32_t a0 = fqCount0( first ) + ( e0 ? s1 : s0 ), a1 = fqCount1( first ) + ( e1 ? s1 : s0 );
    return ( first & FIELD_RESET ) | ( ( first ^ second ) & FQ_PARITY ) | ( a0 < cap ? a0 : cap ) | ( ( a1 < cap ? a1 : cap ) << FQ_COUNT_BITS );
}

/** Inclusive scan of the workgroup's FIELD_THREADS elements in LDS; every lane calls it. */
__device__ __forceinline__ void
fqScan( uint32_t* elements, uint32_t tid, uint32_t cap )
{
    for ( uint32_t d = 1; d < FIELD_THREADS; d <<= 1 ) {
        uint32_t composed = elements[tid];
        if ( tid >= d ) composed = fqCompose( elements[tid - d], composed, cap );
        __syncthreads();
        elements[tid] = composed;
        __syncthreads();
    }
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_field_chunks_quoted( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint32_t nl, uint32_t dl, uint32_t quote,
                       uint32_t cap, uint32_t* __restrict__ prefixes, uint32_t* __restrict__ counts,
                       FieldTile* __restrict__ tileSummaries )
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

    /* since the chunk's last nl: the q bytes' parity, and the dl bytes passed with an even ( even ) and an odd ( odd )
     * number of q bytes in front of them -- those that count when the chunk is entered outside and inside quotes */
    uint32_t even = 0, odd = 0, parity = 0, count = 0, last = nl;
    for ( uint32_t pass = 0; pass < LINEHASH_PASSES; ++pass ) {
        lhStage( t, out, stage[wave], wave, lane, pass );
        __syncthreads();
        const uint32_t done = pass * LINEHASH_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < LINEHASH_PIECE ? chunkSize - done : LINEHASH_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            last = row[i];
            if ( last == nl ) {
                ++count;
                even = 0;
                odd = 0;
                parity = 0;
            } else if ( last == quote ) {
                parity ^= 1;
            } else if ( last == dl ) {
                if ( parity != 0 ) ++odd;
                else ++even;
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
    /* behind an nl the line is outside quotes whatever the chunk was entered with */
    const uint32_t a0 = even < cap ? even : cap, a1 = count != 0 ? a0 : ( odd < cap ? odd : cap );
    elements[tid] = ( count != 0 ? FIELD_RESET : 0u ) | ( parity != 0 ? FQ_PARITY : 0u ) | a0 | ( a1 << FQ_COUNT_BITS );
    if ( count != 0 ) atomicAdd( &tileCount, count );
    __syncthreads();
    fqScan( elements, tid, cap );

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
k_field_link_quoted( const FieldSpanTiles* __restrict__ spans, FieldTile* __restrict__ tileSummaries,
                     QuotedFieldSpanSummary* __restrict__ spanSummaries, uint32_t field )
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
        fqScan( elements, tid, cap );

        /* the whole entering element: k_field_emit_quoted reads both hypotheses from it */
        if ( tid < n ) tile->entry = tid > 0 ? fqCompose( carry, elements[tid - 1], cap ) : carry;
        __syncthreads();
        if ( tid == 0 ) carry = fqCompose( carry, elements[n - 1], cap );
        __syncthreads();
    }

    if ( sum != 0 ) atomicAdd( &total, sum );
    /* the lane that saw the span's last tile; lane 0 of an empty span */
    const bool closes = span.nTiles == 0 ? tid == 0 : tid == ( span.nTiles - 1 ) % FIELD_THREADS;
    __syncthreads();
    if ( closes ) {
        QuotedFieldSpanSummary* const summary = spanSummaries + blockIdx.x;
        const bool inQuote = ( carry & FQ_PARITY ) != 0;
        summary->count = total;
        summary->firstNl = FIELD_NOT_REACHED;
        summary->tailStart = 0;
        /* field 0 starts where its line starts: k_field_emit_quoted moves this behind the span's last nl */
        summary->tailFieldStart = field == 0 ? 0 : FIELD_NOT_REACHED;
        summary->tailFieldEnd = FIELD_NOT_REACHED;
        summary->headDelims[0] = fqCount0( carry );     /* the three without an nl; with one, k_field_emit_quoted knows */
        summary->headDelims[1] = fqCount1( carry );
        summary->headQuoteParity = inQuote ? 1u : 0u;
        summary->tailDelims = fqCount0( carry );
        summary->info = ( ( carry & FIELD_RESET ) != 0 ? FIELD_HAS_DELIMITER : 0u ) | ( lastInfo & FIELD_TAIL_NON_EMPTY )
                        | ( inQuote ? FIELD_TAIL_IN_QUOTE : 0u );
        summary->unused = 0;
    }
}

/** Where k_field_emit_quoted's stores go: FieldSink with the quoted summary. */
struct QuotedFieldSink
{
    uint64_t skip, capacity, base, spanEnd;
    uint64_t* starts;
    int64_t* sizes;
    QuotedFieldSpanSummary* summary;
};

/** Field j of line `line` starts at `p` of the span. */
__device__ __forceinline__ void
fqStart( const QuotedFieldSink& to, uint64_t line, uint64_t p )
{
    if ( line == to.spanEnd ) {
        to.summary->tailFieldStart = p;
    } else if ( line - to.skip < to.capacity ) {    /* a line in front of `skip` wraps to one beyond every capacity */
        to.starts[line - to.skip] = to.base + p;
    }
}

/** Field j of line `line` ends at `p` of the span. */
__device__ __forceinline__ void
fqEnd( const QuotedFieldSink& to, uint64_t line, uint64_t p )
{
    if ( line == to.spanEnd ) {
        to.summary->tailFieldEnd = p;
    } else if ( line - to.skip < to.capacity ) {
        to.sizes[line - to.skip] = (int64_t)( to.base + p );
    }
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_field_emit_quoted( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint32_t nl, uint32_t dl, uint32_t quote,
                     uint32_t field, const FieldSpanTiles* __restrict__ spans, const uint32_t* __restrict__ prefixes,
                     const FieldTile* __restrict__ tileSummaries, const uint64_t* __restrict__ places,
                     QuotedFieldSpanSummary* spanSummaries, uint64_t* __restrict__ headPositions, uint64_t skip, uint64_t capacity,
                     uint64_t* __restrict__ starts, int64_t* __restrict__ sizes )
{
    __shared__ uint32_t stage[FIELD_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    const CountTile t = tiles[blockIdx.x];
    const FieldSpanTiles span = spans[t.span];
    const FieldTile tile = tileSummaries[blockIdx.x];
    const uint32_t cap = field + 1;
    /* the same in every lane: the places ascend with the slots */
    const uint64_t spanFirst = places[span.firstTile * FIELD_THREADS];
    const uint64_t tileFirst = places[(uint64_t)blockIdx.x * FIELD_THREADS];
    QuotedFieldSink to{ skip, capacity, span.base, spanFirst + spanSummaries[t.span].count, starts, sizes, spanSummaries + t.span };
    const bool outside = ( tileFirst >= skip && tileFirst - skip >= capacity ) || tileFirst + tile.count < skip;
    if ( outside && tileFirst != spanFirst && tileFirst + tile.count != to.spanEnd ) return;

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t slot = (uint64_t)blockIdx.x * FIELD_THREADS + tid;
    const uint32_t begin = tid * FIELD_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < FIELD_CHUNK ? t.size - begin : FIELD_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );
    /* per span: the positions under "entered outside", then those under "entered inside" */
    uint64_t* const heads = headPositions + (uint64_t)t.span * 2 * cap;

    /* the span is entered outside quotes: ( c, inq ).  Entered inside, the chunk's state is ( c1, !inq ) as long as no
     * nl lies in front of it, i.e. while place == spanFirst, and nobody asks after that */
    const uint32_t entering = fqCompose( tile.entry, prefixes[slot], cap );
    uint32_t c = fqCount0( entering ), c1 = fqCount1( entering );
    uint32_t inq = ( entering & FQ_PARITY ) != 0 ? 1u : 0u;
    uint64_t place = places[slot];
    /* of the chunk's first byte in its span */
    const uint64_t chunkAt = ( (uint64_t)blockIdx.x - span.firstTile ) * COUNT_TILE + begin;
    if ( field == 0 && chunkAt == 0 ) fqStart( to, place, 0 );
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
                    fqEnd( to, place, p );
                }
                if ( place == spanFirst ) {
                    to.summary->firstNl = p;
                    to.summary->headDelims[0] = c;
                    to.summary->headDelims[1] = c1;
                    to.summary->headQuoteParity = inq;
                }
                ++place;
                c = 0;
                inq = 0;
                if ( place == to.spanEnd ) to.summary->tailStart = p + 1;
                if ( field == 0 ) fqStart( to, place, p + 1 );
            } else if ( b == quote ) {
                inq ^= 1;
            } else if ( b == dl ) {
                if ( inq == 0 ) {
                    if ( c <= field ) {
                        if ( place == spanFirst ) heads[c] = p;
                        if ( c == field ) fqEnd( to, place, p );
                        ++c;
                        if ( c == field ) fqStart( to, place, p + 1 );
                    }
                } else if ( place == spanFirst && c1 <= field ) {
                    heads[cap + c1] = p;
                    ++c1;
                }
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
}

/** Behind k_field_sizes: the raw field of line skip + i becomes its content.  The number of closed lines is read where
 * k_scan_tiles left it; span s begins at line places[its first slot], and an empty span, which has no slot, at the line
 * of the span behind it: the last span that begins at or in front of a line is the line's. */
__global__ __launch_bounds__( FIELD_UNQUOTE_THREADS ) void
k_field_unquote( const CountTile* __restrict__ tiles, uint64_t nTiles, const FieldSpanTiles* __restrict__ spans, uint32_t nSpans,
                 const uint64_t* __restrict__ places, const uint32_t* __restrict__ counts, uint64_t slots,
                 const uint8_t* __restrict__ out, uint32_t quote, uint64_t skip, uint64_t capacity, uint64_t* __restrict__ starts,
                 int64_t* __restrict__ sizes )
{
    const uint64_t total = places[slots - 1] + counts[slots - 1];
    const uint64_t n = total > skip ? ( total - skip < capacity ? total - skip : capacity ) : 0;
    for ( uint64_t i = (uint64_t)blockIdx.x * FIELD_UNQUOTE_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELD_UNQUOTE_THREADS ) {
        const int64_t size = sizes[i];
        if ( size < 2 ) continue;
        const uint64_t line = skip + i;
        uint32_t low = 0, high = nSpans - 1;
        for ( uint32_t step = 0; step < 32 && low < high; ++step ) {
            const uint32_t middle = low + ( high - low + 1 ) / 2;
            const uint64_t firstTile = spans[middle].firstTile;
            const uint64_t firstLine = firstTile < nTiles ? places[firstTile * FIELD_THREADS] : total;
            if ( firstLine <= line ) low = middle;
            else high = middle - 1;
        }
        const FieldSpanTiles span = spans[low];
        if ( span.nTiles == 0 ) continue;    /* cannot be: the line's span holds its nl */
        const uint64_t start = starts[i];
        const uint8_t* const field = out + tiles[span.firstTile].src + ( start - span.base );
        if ( field[0] == quote && field[size - 1] == quote ) {
            starts[i] = start + 1;
            sizes[i] = size - 2;
        }
    }
}
}  // namespace bz2gpu
