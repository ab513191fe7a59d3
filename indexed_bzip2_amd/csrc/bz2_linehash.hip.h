/**
 * bz2_linehash.hip.h -- one 61-bit polynomial hash per line of spans of a batch's ragged output: the kernels under
 * mi355x_bz2_hash_lines, i.e. under the reader's line_hashes and distinct_lines.  bz2_linehash.hpp has the hash
 * ( h = h * x + b + 1 mod p = 2^61 - 1 over a line's content ), the summary of a stretch and the rule that composes
 * summaries; these kernels apply that rule between the chunks of a tile and between the tiles of a span.
 *
 * The tiling is the regex kernels': a span is cut into tiles of COUNT_TILE bytes (CountTile of bz2_lines.hip.h), a tile
 * into LINEHASH_THREADS chunks of LINEHASH_CHUNK bytes, one lane per chunk, one workgroup per tile; chunk k of tile t is
 * slot t * LINEHASH_THREADS + k of the per-chunk arrays, and the unused slots of a span's last tile count 0.  The bytes
 * are staged through LDS as regexTile stages them and for the same reason (lanes that walk their own chunk with global
 * loads touch 64 cache lines per instruction): per pass, the five aligned 16-byte vectors that cover a chunk's piece of
 * LINEHASH_PIECE bytes are loaded by five of eight adjacent lanes and written to the chunk's row of 21 dwords, an odd
 * stride so that the lanes of a wave, which read the same byte of their rows, hit different banks.  The vectors reach at
 * most 15 bytes in front of a tile (the buffer is 16-byte aligned) and never one that starts at or behind the tile's end.
 *
 * What is scanned.  A stretch acts on the hash c of the unfinished line it is entered with as c -> c * m + a: without
 * a delimiter m = x^len and a = its hash; with one, m = 0 and a = the hash of its tail -- p is prime and x != 0, so
 * m == 0 says "holds a delimiter" and nothing else.  b rides along for the summary's tail.xl: ( m, a, b ) followed by
 * ( m', a', b' ) is ( m m', a m' + a', b m' + b' ), which is the composition of bz2_linehash.hpp with the restart folded
 * into the zero.  It is associative, so it is scanned, on two levels (the one-level scan of k_regex_link is what DESIGN.md
 * measured at 22 to 29 ms per launch):
 *
 *   k_linehash_chunks  per chunk: Horner over the staged bytes gives head, tail and the number of delimiters; x^len comes
 *                      from a table of x^0 .. x^256 in LDS (each lane squares its way to one entry), so a byte costs one
 *                      mulmod.  Then the tile's 256 elements are scanned in LDS, log2( 256 ) rounds.  Written per chunk:
 *                      its EXCLUSIVE prefix ( m, a ) within the tile and its count; per tile: the tile's element, its
 *                      head ( h, xl ), its count, hasDelimiter and whether its last byte is a delimiter.
 *   k_linehash_link    one workgroup per span scans the TILE elements, LINEHASH_THREADS tiles per step with one carry
 *                      element between steps: a span of 430 MB is 26 steps, not 6 600.  Every tile gets the hash its first
 *                      line is entered with (the span itself is entered with 0); the span's summary -- head, tail,
 *                      hasDelimiter, tailNonEmpty -- and its count of closed lines are written.
 *   k_scan_tiles       (bz2_search.hip.h) the exclusive prefix sums of the chunk counts, as they are.
 *   k_linehash_emit    entry = tile entry * m + a of the chunk's prefix, then Horner again; at every delimiter the hash
 *                      goes to the chunk's next place, less `skip`.  Nothing is written in front of `skip` or at or
 *                      beyond skip + capacity, and a tile whose first place is already there returns at once.
 *
 * Places and slots are 64 bit.  Every loop is bounded by the chunk or by the number of tiles; no workgroup waits on
 * another; vector stores only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_lines.hip.h"

namespace bz2gpu
{
constexpr uint32_t LINEHASH_CHUNK = 256;
constexpr uint32_t LINEHASH_THREADS = 256;                  /* chunks per tile, tiles per step of the link */
constexpr uint32_t LINEHASH_PIECE = 64;
constexpr uint32_t LINEHASH_PASSES = LINEHASH_CHUNK / LINEHASH_PIECE;
constexpr uint32_t LINEHASH_ROW_DWORDS = 21;                /* 80 bytes of data, 4 of padding */
constexpr uint64_t LINEHASH_PRIME = ( uint64_t( 1 ) << 61 ) - 1;
constexpr uint64_t LINEHASH_HAS_DELIMITER = 1, LINEHASH_TAIL_NON_EMPTY = 2;
static_assert( LINEHASH_CHUNK * LINEHASH_THREADS == COUNT_TILE, "a tile is one workgroup" );

/** What k_linehash_chunks leaves per tile and k_linehash_link completes. */
struct LineHashTile
{
    uint64_t m, a, b;          /* the tile's element */
    uint64_t headH, headXl;    /* the bytes in front of its first delimiter, all of them without one */
    uint64_t count;            /* delimiters */
    uint64_t info;             /* LINEHASH_HAS_DELIMITER, LINEHASH_TAIL_NON_EMPTY */
    uint64_t entry;            /* k_linehash_link: the hash the tile's first line is entered with */
};

/** What k_linehash_link is told about a span, and what it answers. */
struct LineHashSpan
{
    uint64_t firstTile, nTiles;
};

struct LineHashSpanSummary
{
    uint64_t headH, headXl, tailH, tailXl, count, info;
};

/** a * b mod p for a * b < 2^122: the canonical value. */
__device__ __forceinline__ uint64_t
lhMul( uint64_t a, uint64_t b )
{
    const uint64_t lo = a * b, hi = __umul64hi( a, b );
    uint64_t r = ( lo & LINEHASH_PRIME ) + ( ( lo >> 61 ) | ( hi << 3 ) );
    r = ( r & LINEHASH_PRIME ) + ( r >> 61 );
    return r >= LINEHASH_PRIME ? r - LINEHASH_PRIME : r;
}

/** ( a + b ) mod p for a, b < p (and for a < p, b <= 256 < p). */
__device__ __forceinline__ uint64_t
lhAdd( uint64_t a, uint64_t b )
{
    const uint64_t r = a + b;
    return r >= LINEHASH_PRIME ? r - LINEHASH_PRIME : r;
}

struct LineHashElement
{
    uint64_t m, a, b;
};

/** `first` followed by `second`. */
__device__ __forceinline__ LineHashElement
lhCompose( const LineHashElement& first, const LineHashElement& second )
{
    /* behind a delimiter nothing in front matters: spare the multiplications */
    if ( second.m == 0 ) return second;
    return { lhMul( first.m, second.m ), lhAdd( lhMul( first.a, second.m ), second.a ), lhMul( first.b, second.m ) };
}

/** Inclusive scan of the workgroup's LINEHASH_THREADS elements in LDS; every lane calls it. */
__device__ __forceinline__ void
lhScan( LineHashElement* elements, uint32_t tid )
{
    for ( uint32_t d = 1; d < LINEHASH_THREADS; d <<= 1 ) {
        LineHashElement composed = elements[tid];
        if ( tid >= d ) composed = lhCompose( elements[tid - d], composed );
        __syncthreads();
        elements[tid] = composed;
        __syncthreads();
    }
}

/** The pass's piece of the wave's 64 chunks into its rows: lanes 8 r' .. 8 r' + 4 load the five vectors of row r. */
__device__ __forceinline__ void
lhStage( const CountTile& t, const uint8_t* __restrict__ out, uint32_t* rows, uint32_t wave, uint32_t lane, uint32_t pass )
{
    const uint64_t tileEnd = t.src + t.size;
    const uint32_t j = lane & 7;
#pragma unroll
    for ( uint32_t k = 0; k < 8; ++k ) {
        const uint32_t r = ( lane >> 3 ) + 8 * k;
        const uint64_t pieceBegin = t.src + (uint64_t)( wave * 64 + r ) * LINEHASH_CHUNK + pass * LINEHASH_PIECE;
        const uint64_t pieceEnd = pieceBegin + LINEHASH_PIECE < tileEnd ? pieceBegin + LINEHASH_PIECE : tileEnd;
        const uint64_t vector = ( pieceBegin & ~uint64_t( 15 ) ) + 16ull * j;
        if ( j < 5 && vector < pieceEnd ) {
            const uint4 d = *reinterpret_cast<const uint4*>( out + vector );
            uint32_t* const to = rows + r * LINEHASH_ROW_DWORDS + 4 * j;
            to[0] = d.x;
            to[1] = d.y;
            to[2] = d.z;
            to[3] = d.w;
        }
    }
}

__global__ __launch_bounds__( LINEHASH_THREADS ) void
k_linehash_chunks( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint64_t x, uint32_t nl,
                   ulonglong2* __restrict__ prefixes, uint32_t* __restrict__ counts, LineHashTile* __restrict__ tileSummaries )
{
    __shared__ uint32_t stage[LINEHASH_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    __shared__ uint64_t powers[LINEHASH_CHUNK + 1];
    __shared__ LineHashElement elements[LINEHASH_THREADS];
    __shared__ uint32_t firstDelimiter, tileCount;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CountTile t = tiles[blockIdx.x];

    /* x^tid by squaring: eight rounds whatever the lane; lane 0 adds x^256 */
    {
        uint64_t power = 1, square = x;
#pragma unroll
        for ( uint32_t bit = 0; bit < 8; ++bit ) {
            if ( ( tid >> bit ) & 1u ) power = lhMul( power, square );
            square = lhMul( square, square );
        }
        powers[tid] = power;
        if ( tid == 0 ) {
            powers[LINEHASH_CHUNK] = square;
            firstDelimiter = LINEHASH_THREADS;
            tileCount = 0;
        }
    }

    const uint64_t slot = (uint64_t)blockIdx.x * LINEHASH_THREADS + tid;
    const uint32_t begin = tid * LINEHASH_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < LINEHASH_CHUNK ? t.size - begin : LINEHASH_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );

    /* h and length of the bytes since the chunk's last delimiter, of the head until the first one */
    uint64_t h = 0, headH = 0;
    uint32_t length = 0, headLength = 0, count = 0, last = nl;
    for ( uint32_t pass = 0; pass < LINEHASH_PASSES; ++pass ) {
        lhStage( t, out, stage[wave], wave, lane, pass );
        __syncthreads();
        const uint32_t done = pass * LINEHASH_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < LINEHASH_PIECE ? chunkSize - done : LINEHASH_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            last = row[i];
            if ( last == nl ) {
                if ( count == 0 ) {
                    headH = h;
                    headLength = length;
                }
                ++count;
                h = 0;
                length = 0;
            } else {
                h = lhAdd( lhMul( h, x ), last + 1 );
                ++length;
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
    if ( count == 0 ) {
        headH = h;
        headLength = length;
    }
    const uint64_t headXl = powers[headLength];
    LineHashElement own = count == 0 ? LineHashElement{ headXl, headH, 0 } : LineHashElement{ 0, h, powers[length] };
    elements[tid] = own;
    if ( count != 0 ) {
        atomicMin( &firstDelimiter, tid );
        atomicAdd( &tileCount, count );
    }
    __syncthreads();
    lhScan( elements, tid );

    const LineHashElement before = tid > 0 ? elements[tid - 1] : LineHashElement{ 1, 0, 0 };
    prefixes[slot] = make_ulonglong2( before.m, before.a );
    counts[slot] = count;
    LineHashTile* const summary = tileSummaries + blockIdx.x;
    /* the head ends in the chunk with the first delimiter: no delimiter in front of it, so `before` is all of it */
    if ( tid == firstDelimiter ) {
        summary->headH = lhAdd( lhMul( before.a, headXl ), headH );
        summary->headXl = lhMul( before.m, headXl );
    }
    if ( tid == LINEHASH_THREADS - 1 ) {
        const LineHashElement all = elements[tid];
        summary->m = all.m;
        summary->a = all.a;
        summary->b = all.b;
        if ( firstDelimiter == LINEHASH_THREADS ) {
            summary->headH = all.a;
            summary->headXl = all.m;
        }
        summary->count = tileCount;
        summary->entry = 0;
    }
    /* the lane that holds the tile's last byte (a tile is never empty) */
    if ( tid == ( t.size - 1 ) / LINEHASH_CHUNK ) {
        summary->info = ( firstDelimiter != LINEHASH_THREADS ? LINEHASH_HAS_DELIMITER : 0 ) | ( last != nl ? LINEHASH_TAIL_NON_EMPTY : 0 );
    }
}

__global__ __launch_bounds__( LINEHASH_THREADS ) void
k_linehash_link( const LineHashSpan* __restrict__ spans, LineHashTile* __restrict__ tileSummaries,
                 LineHashSpanSummary* __restrict__ spanSummaries )
{
    __shared__ LineHashElement elements[LINEHASH_THREADS];
    __shared__ LineHashElement carry;
    __shared__ uint32_t firstDelimiter;
    __shared__ uint32_t headFound;
    __shared__ unsigned long long total;
    const uint32_t tid = threadIdx.x;
    const LineHashSpan span = spans[blockIdx.x];
    LineHashSpanSummary* const summary = spanSummaries + blockIdx.x;
    if ( tid == 0 ) {
        carry = { 1, 0, 0 };
        headFound = 0;
        total = 0;
        firstDelimiter = LINEHASH_THREADS;
    }
    __syncthreads();

    unsigned long long sum = 0;
    uint64_t lastInfo = 0;
    for ( uint64_t t0 = 0; t0 < span.nTiles; t0 += LINEHASH_THREADS ) {
        const uint32_t n = span.nTiles - t0 < LINEHASH_THREADS ? (uint32_t)( span.nTiles - t0 ) : LINEHASH_THREADS;
        LineHashTile* const tile = tileSummaries + span.firstTile + t0 + tid;
        LineHashElement own{ 1, 0, 0 };
        uint64_t info = 0;
        if ( tid < n ) {
            own = { tile->m, tile->a, tile->b };
            info = tile->info;
            sum += tile->count;
            if ( ( info & LINEHASH_HAS_DELIMITER ) != 0 ) atomicMin( &firstDelimiter, tid );
            if ( t0 + tid + 1 == span.nTiles ) lastInfo = info;
        }
        elements[tid] = own;
        __syncthreads();
        lhScan( elements, tid );

        if ( tid < n ) {
            const LineHashElement before = tid > 0 ? lhCompose( carry, elements[tid - 1] ) : carry;
            /* the span is entered with hash 0: c * m + a at c = 0 */
            tile->entry = before.a;
            if ( headFound == 0 && tid == firstDelimiter ) {
                summary->headH = lhAdd( lhMul( before.a, tile->headXl ), tile->headH );
                summary->headXl = lhMul( before.m, tile->headXl );
            }
        }
        __syncthreads();
        if ( tid == 0 ) {
            carry = lhCompose( carry, elements[n - 1] );
            if ( firstDelimiter != LINEHASH_THREADS ) headFound = 1;
        }
        __syncthreads();
    }

    if ( sum != 0 ) atomicAdd( &total, sum );
    /* the lane that saw the span's last tile; lane 0 of an empty span */
    const bool closes = span.nTiles == 0 ? tid == 0 : tid == ( span.nTiles - 1 ) % LINEHASH_THREADS;
    __syncthreads();
    if ( closes ) {
        if ( headFound == 0 ) {
            summary->headH = carry.a;
            summary->headXl = carry.m;
        }
        summary->tailH = headFound != 0 ? carry.a : 0;
        summary->tailXl = headFound != 0 ? carry.b : 1;
        summary->count = total;
        summary->info = ( headFound != 0 ? LINEHASH_HAS_DELIMITER : 0 ) | ( lastInfo & LINEHASH_TAIL_NON_EMPTY );
    }
}

__global__ __launch_bounds__( LINEHASH_THREADS ) void
k_linehash_emit( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint64_t x, uint32_t nl,
                 const ulonglong2* __restrict__ prefixes, const LineHashTile* __restrict__ tileSummaries,
                 const uint64_t* __restrict__ places, uint64_t skip, uint64_t capacity, uint64_t* __restrict__ hashes )
{
    __shared__ uint32_t stage[LINEHASH_THREADS / 64][64 * LINEHASH_ROW_DWORDS];
    /* the same in every lane: the places ascend with the slots */
    const uint64_t firstPlace = places[(uint64_t)blockIdx.x * LINEHASH_THREADS];
    if ( firstPlace >= skip && firstPlace - skip >= capacity ) return;
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const CountTile t = tiles[blockIdx.x];
    const uint64_t slot = (uint64_t)blockIdx.x * LINEHASH_THREADS + tid;
    const uint32_t begin = tid * LINEHASH_CHUNK;
    const uint32_t chunkSize = begin < t.size ? ( t.size - begin < LINEHASH_CHUNK ? t.size - begin : LINEHASH_CHUNK ) : 0u;
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * LINEHASH_ROW_DWORDS ) + (uint32_t)( t.src & 15 );

    const ulonglong2 prefix = prefixes[slot];
    uint64_t h = lhAdd( lhMul( tileSummaries[blockIdx.x].entry, prefix.x ), prefix.y );
    uint64_t place = places[slot];
    for ( uint32_t pass = 0; pass < LINEHASH_PASSES; ++pass ) {
        lhStage( t, out, stage[wave], wave, lane, pass );
        __syncthreads();
        const uint32_t done = pass * LINEHASH_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < LINEHASH_PIECE ? chunkSize - done : LINEHASH_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            const uint32_t b = row[i];
            if ( b == nl ) {
                /* a place in front of `skip` wraps to one beyond every capacity */
                if ( place - skip < capacity ) hashes[place - skip] = h;
                ++place;
                h = 0;
            } else {
                h = lhAdd( lhMul( h, x ), b + 1 );
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }
}
}  // namespace bz2gpu
