/**
 * bz2_lines.hip.h -- counting and selecting one byte value in spans of a batch's ragged output: the kernels under
 * mi355x_bz2_count_byte / mi355x_bz2_find_byte, i.e. under the newline index and the line ranges of the reader.
 *
 * The host cuts every span into tiles of at most COUNT_TILE bytes (as it cuts gather pieces for k_gather), so that a
 * block that decodes to tens of MB neither serialises on one workgroup when it is counted nor is walked serially when the
 * k-th occurrence in it is looked for.
 *
 *   k_count_byte  one workgroup per tile: 16-byte loads of the aligned vectors that cover the tile, a compare of all four
 *                 bytes of a dword at once (no branch per byte), popcounts, a wave reduction, one count per tile -- and,
 *                 for callers that want sums, one 64-bit atomic add per tile to its span's counter.  Spans start and end
 *                 at any alignment (blocks lie back to back at prefix-sum offsets): the first and the last vector of a
 *                 tile are masked, so that nothing outside [src, src + size) is counted.  The aligned loads reach at most
 *                 15 bytes in front of a tile (never in front of the buffer, which is 16-byte aligned) and 15 behind it
 *                 (the output buffer has 256 bytes of slack behind the batch's last byte).
 *   k_find_byte   one wave per query {tiles of a span, rank}: (1) the tile -- the wave scans the prefix sums of the span's
 *                 tile counts, 64 tiles per step; (2) the lane -- every lane counts a contiguous 64th of the tile's
 *                 vectors, a wave prefix picks the one that holds the occurrence; (3) the vector -- the lanes take that
 *                 lane's vectors one each, a wave prefix picks the vector and the lane that has it picks the bit.
 *                 "Fewer than rank occurrences" (also: counts that do not add up) gives UINT64_MAX.
 *   k_rank_byte   the inverse: how many occurrences lie in front of a position.  One wave per TILE that holds queries,
 *                 however many: the host sorts a span's positions and groups them by tile, so that a tile is read at most
 *                 once per call (the matches of a frequent string fall into one tile by the thousand).  The wave (1) sums
 *                 the counts of the span's tiles in front of its own, 64 per step; (2) walks its tile 64 vectors (1 KiB)
 *                 per step: a wave-inclusive scan of the lanes' popcounts gives the count in front of every vector of the
 *                 step; (3) answers the step's queries 64 at a time -- the lane of a query fetches the exclusive prefix
 *                 and the hit mask of the query's vector with __shfl and adds the hits below the position --; and stops
 *                 behind the tile's last query.  No atomics, no LDS, and every loop is bounded by the tile and the
 *                 query count.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bz2gpu
{
constexpr uint32_t COUNT_THREADS = 256;
constexpr uint32_t COUNT_TILE = 65536;
constexpr uint32_t FIND_THREADS = 64;
constexpr uint64_t FIND_NONE = ~uint64_t( 0 );

struct CountTile
{
    uint64_t src;      /* in the batch's output */
    uint32_t size;     /* <= COUNT_TILE */
    uint32_t span;     /* whose counter the tile adds to */
};

struct FindQuery
{
    uint64_t rank;     /* 1-based */
    uint32_t firstTile, nTiles;
};

/** The queries of one tile for k_rank_byte: ends[firstQuery .. firstQuery + nQueries) ascending, each the number of the
 * tile's bytes in front of the position, 1 .. the tile's size (a position at a tile's first byte belongs to the tile in
 * front, as its end; the host answers a position at the span's first byte itself). */
struct RankTile
{
    uint32_t tile;         /* in the tile list */
    uint32_t firstTile;    /* of the tile's span */
    uint32_t firstQuery, nQueries;
};

/** Bit 7 of every byte of x that is zero (exact: the sums stay inside their bytes). */
__device__ __forceinline__ uint32_t
zeroBytes( uint32_t x )
{
    return ~( ( ( x & 0x7F7F7F7Fu ) + 0x7F7F7F7Fu ) | x | 0x7F7F7F7Fu );
}

/** Bit i: byte i of the 16 bytes equals the value whose four copies are `pattern`. */
__device__ __forceinline__ uint32_t
matches16( uint4 d, uint32_t pattern )
{
    /* bits 7, 15, 23, 31 -> bits 0..3: the four products land on 21..24 and no two partial products meet */
    const auto nibble = [] ( uint32_t m ) { return ( ( ( m >> 7 ) * 0x00204081u ) >> 21 ) & 0xFu; };
    return nibble( zeroBytes( d.x ^ pattern ) ) | ( nibble( zeroBytes( d.y ^ pattern ) ) << 4 )
           | ( nibble( zeroBytes( d.z ^ pattern ) ) << 8 ) | ( nibble( zeroBytes( d.w ^ pattern ) ) << 12 );
}

/** Bit i: byte a + i lies in [begin, end). */
__device__ __forceinline__ uint32_t
validBytes16( uint64_t a, uint64_t begin, uint64_t end )
{
    const uint32_t lo = a < begin ? ( begin - a < 16 ? (uint32_t)( begin - a ) : 16u ) : 0u;
    const uint32_t hi = a + 16 > end ? ( a < end ? (uint32_t)( end - a ) : 0u ) : 16u;
    return hi > lo ? ( ( 0xFFFFu >> ( 16u - hi ) ) & ( 0xFFFFu << lo ) ) : 0u;
}

__device__ __forceinline__ uint32_t
waveInclusiveScan( uint32_t x, uint32_t lane )
{
#pragma unroll
    for ( uint32_t d = 1; d < 64; d <<= 1 ) {
        const uint32_t below = __shfl_up( x, d );
        if ( lane >= d ) x += below;
    }
    return x;
}

__global__ __launch_bounds__( COUNT_THREADS ) void
k_count_byte( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, uint32_t pattern,
              uint32_t* __restrict__ tileCounts, unsigned long long* __restrict__ spanCounts )
{
    __shared__ uint32_t waveCounts[COUNT_THREADS / 64];
    const CountTile t = tiles[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t begin = t.src, end = t.src + t.size;
    const uint64_t base = begin & ~uint64_t( 15 );
    const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
    const uint4* const v = reinterpret_cast<const uint4*>( out + base );

    uint32_t count = 0;
    /* the two vectors that may reach outside the tile */
    if ( tid < 2 && tid < vectors ) {
        const uint32_t k = tid == 0 ? 0 : vectors - 1;
        if ( tid == 0 || vectors > 1 ) {
            count = __popc( matches16( v[k], pattern ) & validBytes16( base + 16ull * k, begin, end ) );
        }
    }
    /* those between lie inside it */
#pragma unroll 4
    for ( uint32_t k = 1 + tid; k + 1 < vectors; k += COUNT_THREADS ) {
        const uint4 d = v[k];
        count += __popc( zeroBytes( d.x ^ pattern ) ) + __popc( zeroBytes( d.y ^ pattern ) )
                 + __popc( zeroBytes( d.z ^ pattern ) ) + __popc( zeroBytes( d.w ^ pattern ) );
    }
#pragma unroll
    for ( uint32_t d = 32; d > 0; d >>= 1 ) count += __shfl_down( count, d );
    if ( ( tid & 63 ) == 0 ) waveCounts[tid >> 6] = count;
    __syncthreads();
    if ( tid == 0 ) {
        uint32_t total = 0;
#pragma unroll
        for ( uint32_t w = 0; w < COUNT_THREADS / 64; ++w ) total += waveCounts[w];
        tileCounts[blockIdx.x] = total;
        if ( spanCounts != nullptr && total != 0 ) atomicAdd( spanCounts + t.span, (unsigned long long)total );
    }
}

__global__ __launch_bounds__( FIND_THREADS ) void
k_find_byte( const FindQuery* __restrict__ queries, const CountTile* __restrict__ tiles,
             const uint32_t* __restrict__ tileCounts, const uint8_t* __restrict__ out, uint32_t pattern,
             uint64_t* __restrict__ positions )
{
    const FindQuery q = queries[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    uint64_t rank = q.rank;    /* of the occurrence within what has not been skipped yet; the same in every lane */

    /* (1) the tile */
    uint32_t tile = ~0u;
    for ( uint32_t t0 = 0; t0 < q.nTiles; t0 += 64 ) {
        const uint32_t c = t0 + lane < q.nTiles ? tileCounts[q.firstTile + t0 + lane] : 0u;
        const uint32_t upTo = waveInclusiveScan( c, lane );
        const uint64_t reached = __ballot( (uint64_t)upTo >= rank );
        if ( reached != 0 ) {
            const int l = __ffsll( (unsigned long long)reached ) - 1;
            tile = t0 + (uint32_t)l;
            rank -= __shfl( upTo, l ) - __shfl( c, l );
            break;
        }
        rank -= __shfl( upTo, 63 );
    }
    if ( tile == ~0u || rank == 0 ) {
        if ( lane == 0 ) positions[blockIdx.x] = FIND_NONE;
        return;
    }

    /* (2) the lane whose 64th of the tile's vectors holds it */
    const CountTile t = tiles[q.firstTile + tile];
    const uint64_t begin = t.src, end = t.src + t.size;
    const uint64_t base = begin & ~uint64_t( 15 );
    const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
    const uint32_t perLane = ( vectors + 63 ) >> 6;
    const uint4* const v = reinterpret_cast<const uint4*>( out + base );
    uint32_t mine = 0;
    for ( uint32_t j = 0; j < perLane; ++j ) {
        const uint32_t k = lane * perLane + j;
        if ( k < vectors ) mine += __popc( matches16( v[k], pattern ) & validBytes16( base + 16ull * k, begin, end ) );
    }
    uint32_t upTo = waveInclusiveScan( mine, lane );
    uint64_t reached = __ballot( (uint64_t)upTo >= rank );
    if ( reached == 0 ) {
        if ( lane == 0 ) positions[blockIdx.x] = FIND_NONE;
        return;
    }
    int l = __ffsll( (unsigned long long)reached ) - 1;
    rank -= __shfl( upTo, l ) - __shfl( mine, l );

    /* (3) the vector among that lane's, one per lane, and the bit in it */
    const uint32_t first = (uint32_t)l * perLane;
    for ( uint32_t j0 = 0; j0 < perLane; j0 += 64 ) {
        const uint32_t k = first + j0 + lane;
        uint32_t hits = 0;
        if ( j0 + lane < perLane && k < vectors ) {
            hits = matches16( v[k], pattern ) & validBytes16( base + 16ull * k, begin, end );
        }
        const uint32_t c = __popc( hits );
        upTo = waveInclusiveScan( c, lane );
        reached = __ballot( (uint64_t)upTo >= rank );
        if ( reached != 0 ) {
            l = __ffsll( (unsigned long long)reached ) - 1;
            if ( (int)lane == l ) {
                uint32_t skip = (uint32_t)rank - ( upTo - c ) - 1;
                while ( skip-- > 0 ) hits &= hits - 1;
                positions[blockIdx.x] = base + 16ull * k + (uint32_t)( __ffs( hits ) - 1 );
            }
            return;
        }
        rank -= __shfl( upTo, 63 );
    }
    if ( lane == 0 ) positions[blockIdx.x] = FIND_NONE;
}
__global__ __launch_bounds__( FIND_THREADS ) void
k_rank_byte( const RankTile* __restrict__ work, const CountTile* __restrict__ tiles, const uint32_t* __restrict__ tileCounts,
             const uint32_t* __restrict__ ends, const uint8_t* __restrict__ out, uint32_t pattern,
             uint64_t* __restrict__ ranks )
{
    const RankTile w = work[blockIdx.x];
    const uint32_t lane = threadIdx.x;

    /* (1) the occurrences in the span's tiles in front of this one; the same in every lane */
    uint64_t running = 0;
    for ( uint32_t t0 = w.firstTile; t0 < w.tile; t0 += 64 ) {
        const uint32_t c = t0 + lane < w.tile ? tileCounts[t0 + lane] : 0u;
        running += __shfl( waveInclusiveScan( c, lane ), 63 );
    }

    /* (2) the tile, 64 vectors per step, as far as its last query */
    const CountTile t = tiles[w.tile];
    const uint64_t begin = t.src, end = t.src + t.size;
    const uint64_t base = begin & ~uint64_t( 15 );
    const uint32_t lead = (uint32_t)( begin - base );
    const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
    const uint4* const v = reinterpret_cast<const uint4*>( out + base );
    const uint32_t* const e = ends + w.firstQuery;
    uint64_t* const r = ranks + w.firstQuery;
    uint32_t q = 0;   /* queries answered; the same in every lane */
    for ( uint32_t k0 = 0; k0 < vectors && q < w.nQueries; k0 += 64 ) {
        const uint32_t k = k0 + lane;
        /* the mask matters on the tile's first vector only (bytes in front of the tile): what lies behind a position is
         * masked per query below, and no query lies behind the tile's end */
        const uint32_t hits = k < vectors ? matches16( v[k], pattern ) & validBytes16( base + 16ull * k, begin, end ) : 0u;
        const uint32_t c = __popc( hits );
        const uint32_t upTo = waveInclusiveScan( c, lane );
        const uint32_t before = upTo - c;

        /* (3) the queries whose last byte in front of the position lies in this step, 64 at a time */
        while ( q < w.nQueries ) {
            const bool have = q + lane < w.nQueries;
            const uint32_t last = have ? lead + e[q + lane] - 1 : 0u;   /* that byte, from `base` */
            const bool mine = have && ( last >> 4 ) < k0 + 64;
            const uint32_t from = mine ? ( last >> 4 ) - k0 : 0u;
            const uint32_t prefix = __shfl( before, (int)from );
            const uint32_t mask = __shfl( hits, (int)from );
            if ( mine ) r[q + lane] = running + prefix + __popc( mask & ( 0xFFFFu >> ( 15u - ( last & 15u ) ) ) );
            const uint32_t answered = (uint32_t)__popcll( __ballot( mine ) );
            q += answered;
            if ( answered < 64 ) break;
        }
        running += __shfl( upTo, 63 );
    }
}
}  // namespace bz2gpu
