/**
 * bz2_fieldhash.hip.h -- the 61-bit hash of field j of every line, for spans of a batch's ragged output: the kernels
 * under mi355x_bz2_field_hashes, i.e. under the reader's field_hashes and count_by_field.  bz2_fieldhash.hpp has the
 * definition and the rule: the key of a field over [start, end) of its line is P( end ) - P( start ) * x^( end - start ),
 * P( pos ) being the line hash of the bytes of the line in front of pos.
 *
 * Nothing new is scanned.  What a chunk must know about the bytes in front of it is the delimiter count of the field
 * kernels and the running hash of the line-hash kernels, so the first passes are theirs, unchanged, over the same tiles
 * (bz2_fields.hip.h, bz2_linehash.hip.h: k_field_chunks, k_field_link, k_linehash_chunks, k_linehash_link), and
 * k_scan_tiles gives the places.  Then
 *
 *   k_fieldhash_emit    re-walks each chunk from its entering count and its entering line hash.  It stores the events of
 *                       k_field_emit as that kernel does -- start, end or nl-with-fewer into starts / sizes -- and the
 *                       running hash at the same two events: P( start ) into pStarts[place], P( end ) into keys[place].
 *                       The same events in the span's unclosed tail go to the span's summary and tail hashes, and at
 *                       the dl bytes in front of the span's first nl the position goes to the head positions and the
 *                       hash in front of it to the head hashes (the span is entered with hash 0).
 *   k_fieldhash_finish  grid-stride, one lane per line: the end becomes the size, and keys[i] = P( end ) -
 *                       P( start ) * x^size with x^size by squaring, at most 64 rounds; FIELD_MISSING where size is -1.
 *
 * The skip / capacity rules are k_field_emit's: nothing is written in front of `skip` or at or beyond skip + capacity.
 * Places, slots and offsets are 64 bit.  Every loop is bounded by the chunk, by 64 or by the number of lines; no workgroup
 * waits on another; vector stores only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_fields.hip.h"

namespace bz2gpu
{
constexpr uint64_t FIELDHASH_MISSING = LINEHASH_PRIME;

/** P at the field's start and end in a span's unclosed tail, where k_fieldhash_emit reaches them. */
struct FieldHashTail
{
    uint64_t startHash, endHash;
};

/** Where k_fieldhash_emit's stores go. */
struct FieldHashSink
{
    FieldSink fields;
    uint64_t* pStarts;
    uint64_t* keys;
    FieldHashTail* tail;
};

/** Field j of line `line` starts at `p` of the span, the line's bytes in front of it hashing to `h`. */
__device__ __forceinline__ void
fhStart( const FieldHashSink& to, uint64_t line, uint64_t p, uint64_t h )
{
    if ( line == to.fields.spanEnd ) {
        to.fields.summary->tailFieldStart = p;
        to.tail->startHash = h;
    } else if ( line - to.fields.skip < to.fields.capacity ) {    /* a line in front of `skip` wraps beyond every capacity */
        to.fields.starts[line - to.fields.skip] = to.fields.base + p;
        to.pStarts[line - to.fields.skip] = h;
    }
}

/** Field j of line `line` ends at `p` of the span, the line's bytes in front of it hashing to `h`. */
__device__ __forceinline__ void
fhEnd( const FieldHashSink& to, uint64_t line, uint64_t p, uint64_t h )
{
    if ( line == to.fields.spanEnd ) {
        to.fields.summary->tailFieldEnd = p;
        to.tail->endHash = h;
    } else if ( line - to.fields.skip < to.fields.capacity ) {
        to.fields.sizes[line - to.fields.skip] = (int64_t)( to.fields.base + p );
        to.keys[line - to.fields.skip] = h;
    }
}

__global__ __launch_bounds__( FIELD_THREADS ) void
k_fieldhash_emit( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint64_t x, uint32_t nl, uint32_t dl,
                  uint32_t field, const FieldSpanTiles* __restrict__ spans, const uint32_t* __restrict__ prefixes,
                  const FieldTile* __restrict__ tileSummaries, const ulonglong2* __restrict__ hashPrefixes,
                  const LineHashTile* __restrict__ hashTiles, const uint64_t* __restrict__ places,
                  FieldSpanSummary* spanSummaries, FieldHashTail* tails, uint64_t* __restrict__ headPositions,
                  uint64_t* __restrict__ headHashes, uint64_t skip, uint64_t capacity, uint64_t* __restrict__ starts,
                  int64_t* __restrict__ sizes, uint64_t* __restrict__ pStarts, uint64_t* __restrict__ keys )
{
    __shared__ uint32_t stage[FIELD_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    const CountTile t = tiles[blockIdx.x];
    const FieldSpanTiles span = spans[t.span];
    const FieldTile tile = tileSummaries[blockIdx.x];
    const uint32_t cap = field + 1;
    /* the same in every lane: the places ascend with the slots */
    const uint64_t spanFirst = places[span.firstTile * FIELD_THREADS];
    const uint64_t tileFirst = places[(uint64_t)blockIdx.x * FIELD_THREADS];
    const FieldHashSink to{ { skip, capacity, span.base, spanFirst + spanSummaries[t.span].count, starts, sizes, spanSummaries + t.span },
                            pStarts, keys, tails + t.span };
    const uint64_t spanEnd = to.fields.spanEnd;
    const bool outside = ( tileFirst >= skip && tileFirst - skip >= capacity ) || tileFirst + tile.count < skip;
    if ( outside && tileFirst != spanFirst && tileFirst + tile.count != spanEnd ) return;

    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t slot = (uint64_t)blockIdx.x * FIELD_THREADS + tid;
    const uint32_t begin = tid * FIELD_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < FIELD_CHUNK ? t.size - begin : FIELD_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );
    uint64_t* const heads = headPositions + (uint64_t)t.span * cap;
    uint64_t* const headPrefixes = headHashes + (uint64_t)t.span * cap;

    const uint32_t before = prefixes[slot];
    uint32_t c = before & ~FIELD_RESET;
    if ( ( before & FIELD_RESET ) == 0 ) c = tile.entry + c < cap ? tile.entry + c : cap;
    const ulonglong2 hashBefore = hashPrefixes[slot];
    uint64_t h = lhAdd( lhMul( hashTiles[blockIdx.x].entry, hashBefore.x ), hashBefore.y );
    uint64_t place = places[slot];
    /* of the chunk's first byte in its span */
    const uint64_t chunkAt = ( (uint64_t)blockIdx.x - span.firstTile ) * COUNT_TILE + begin;
    if ( field == 0 && chunkAt == 0 ) fhStart( to, place, 0, 0 );
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
                    fhEnd( to, place, p, h );
                }
                if ( place == spanFirst ) {
                    to.fields.summary->firstNl = p;
                    to.fields.summary->headDelims = c;
                }
                ++place;
                c = 0;
                h = 0;
                if ( place == spanEnd ) to.fields.summary->tailStart = p + 1;
                if ( field == 0 ) fhStart( to, place, p + 1, 0 );
                continue;
            }
            const uint64_t behind = lhAdd( lhMul( h, x ), b + 1 );
            if ( b == dl && c <= field ) {
                if ( place == spanFirst ) {
                    heads[c] = p;
                    headPrefixes[c] = h;
                }
                if ( c == field ) fhEnd( to, place, p, h );
                ++c;
                if ( c == field ) fhStart( to, place, p + 1, behind );
            }
            h = behind;
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
}

/** Behind k_fieldhash_emit: sizes[i] holds field i's end, or -1; keys[i] holds P( end ) and pStarts[i] P( start ) where
 * the field is present.  The number of closed lines is read where k_scan_tiles left it. */
__global__ __launch_bounds__( FIELD_SIZES_THREADS ) void
k_fieldhash_finish( const uint64_t* __restrict__ places, const uint32_t* __restrict__ counts, uint64_t slots, uint64_t skip,
                    uint64_t capacity, uint64_t x, const uint64_t* __restrict__ starts, int64_t* __restrict__ sizes,
                    const uint64_t* __restrict__ pStarts, uint64_t* __restrict__ keys )
{
    const uint64_t total = places[slots - 1] + counts[slots - 1];
    const uint64_t n = total > skip ? ( total - skip < capacity ? total - skip : capacity ) : 0;
    for ( uint64_t i = (uint64_t)blockIdx.x * FIELD_SIZES_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * FIELD_SIZES_THREADS ) {
        const int64_t end = sizes[i];
        if ( end < 0 ) {
            keys[i] = FIELDHASH_MISSING;
            continue;
        }
        const uint64_t size = (uint64_t)end - starts[i];
        sizes[i] = (int64_t)size;
        uint64_t power = 1, square = x;
        for ( uint32_t bit = 0; bit < 64 && ( size >> bit ) != 0; ++bit ) {
            if ( ( ( size >> bit ) & 1u ) != 0 ) power = lhMul( power, square );
            square = lhMul( square, square );
        }
        const uint64_t key = keys[i], product = lhMul( pStarts[i], power );
        keys[i] = key >= product ? key - product : key + LINEHASH_PRIME - product;
    }
}
}  // namespace bz2gpu
