/**
 * bz2_search.hip.h -- counting and listing the occurrences of a byte string P (1 <= m = len(P) <= SEARCH_MAX_PATTERN) in
 * spans of a batch's ragged output: the kernels under mi355x_bz2_count_bytes / mi355x_bz2_find_bytes, i.e. under the
 * reader's search.
 *
 * The host cuts the START POSITIONS a span allows -- [offset, offset + size - m + 1), nothing if size < m -- into tiles
 * of at most SEARCH_TILE bytes (the CountTile of bz2_lines.hip.h).  Every byte of a tile is therefore a position p with
 * p + m <= the span's end: a match starts in its tile, may end in the next tile of the same span, and no byte outside
 * the span decides anything.  A tile is one wave: nothing is exchanged through LDS but the pattern, and the order of the
 * positions inside a tile is the order of the lanes.
 *
 *   k_count_bytes  one workgroup (one wave) per tile: 16-byte loads of the aligned vectors that cover the tile's start
 *                  positions, masked at both ends exactly as k_count_byte masks them (validBytes16), matches16 on P[0]
 *                  gives the candidates, and every candidate p is verified byte by byte against P[1..m) in LDS.  The
 *                  verify stops at the first difference, so its first step is the filter on the second byte.  The
 *                  vector loads reach at most 15 bytes behind the last start position, the verify at most to the span's
 *                  last byte.  One count per tile, and one 64-bit atomic add per tile to its span's counter.
 *   k_scan_tiles   one workgroup: the exclusive prefix sums of the tile counts (64 bit), 256 tiles per step.
 *   k_emit_bytes   the same walk as k_count_bytes, 64 vectors per step in ascending order: a wave prefix sum over the
 *                  lanes' hits gives every lane the place of its first hit behind the tile's prefix sum, the lane writes
 *                  its hits in ascending order.  Places >= capacity are not written, and a tile whose prefix sum is
 *                  already >= capacity returns at once: with a limit, only the tiles up to the one that reaches it emit.
 *                  The matches are recomputed, not kept as a bit mask by the counting pass (DESIGN.md says why).
 *   k_seam_bytes   copies the first and the last `n` bytes of one extent behind the counts, so that they come back in
 *                  the same D2H (bz2_search.hpp: what the reader needs for matches that straddle two launches).
 *
 * k_count_bytes and k_emit_bytes are templates over FOLD.  FOLD = false is the exact search.  FOLD = true ignores the
 * case of ASCII letters (foldAscii of bz2_search.hpp: 'A' .. 'Z' | 0x20, every other byte unchanged): the pattern comes
 * folded from the host, every 16-byte vector is folded once (fold16, four 32-bit SWAR steps) before matches16, and the
 * verify folds the data byte it compares.  Folding changes no address: both instantiations read the same bytes.
 *
 * Every loop is bounded by the tile's size (and m); no workgroup waits on another.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_lines.hip.h"

namespace bz2gpu
{
constexpr uint32_t SEARCH_THREADS = 64;
constexpr uint32_t SEARCH_TILE = 16384;
constexpr uint32_t SEARCH_MAX_PATTERN = 256;
constexpr uint32_t SCAN_THREADS = 256;

/** P into LDS, four bytes per lane (the device copy of P is padded to SEARCH_MAX_PATTERN bytes). */
__device__ __forceinline__ void
loadPattern( uint8_t* lds, const uint8_t* __restrict__ pattern, uint32_t lane )
{
    reinterpret_cast<uint32_t*>( lds )[lane] = reinterpret_cast<const uint32_t*>( pattern )[lane];
    __syncthreads();
}

/** foldAscii on the four bytes of w: a byte gets 0x20 iff its top bit is clear and its low seven bits lie in 'A' .. 'Z'
 * (0x41 + 0x3F and 0x5B + 0x25 carry into bit 7; no sum passes 0xBE, so nothing carries into the next byte). */
__device__ __forceinline__ uint32_t
fold4( uint32_t w )
{
    const uint32_t low = w & 0x7F7F7F7Fu;
    const uint32_t up = ( low + 0x3F3F3F3Fu ) & ~( low + 0x25252525u ) & ~w & 0x80808080u;
    return w | ( up >> 2 );
}

template<bool FOLD>
__device__ __forceinline__ uint4
fold16( uint4 d )
{
    if constexpr ( FOLD ) return uint4{ fold4( d.x ), fold4( d.y ), fold4( d.z ), fold4( d.w ) };
    return d;
}

template<bool FOLD>
__device__ __forceinline__ uint32_t
foldByte( uint32_t b )
{
    if constexpr ( FOLD ) return b - 'A' < 26u ? b | 0x20u : b;
    return b;
}

/** Bit i: a match starts at byte a + i, given the candidates (P[0] found there, inside the tile).  FOLD: the pattern in
 * LDS is folded, and so is every data byte that is compared with it. */
template<bool FOLD>
__device__ __forceinline__ uint32_t
verified16( const uint8_t* __restrict__ out, uint64_t a, uint32_t candidates, const uint8_t* lds, uint32_t m )
{
    uint32_t hits = 0;
    while ( candidates != 0 ) {
        const uint32_t bit = (uint32_t)__ffs( candidates ) - 1;
        candidates &= candidates - 1;
        const uint8_t* const at = out + a + bit;
        uint32_t j = 1;
        while ( j < m && foldByte<FOLD>( at[j] ) == lds[j] ) ++j;
        hits |= ( j == m ? 1u : 0u ) << bit;
    }
    return hits;
}

template<bool FOLD>
__global__ __launch_bounds__( SEARCH_THREADS ) void
k_count_bytes( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, const uint8_t* __restrict__ pattern,
               uint32_t m, uint32_t* __restrict__ tileCounts, unsigned long long* __restrict__ spanCounts )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[SEARCH_MAX_PATTERN];
    const uint32_t lane = threadIdx.x;
    loadPattern( lds, pattern, lane );
    const CountTile t = tiles[blockIdx.x];
    const uint64_t begin = t.src, end = t.src + t.size;
    const uint64_t base = begin & ~uint64_t( 15 );
    const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
    const uint4* const v = reinterpret_cast<const uint4*>( out + base );
    const uint32_t first = 0x01010101u * lds[0];

    uint32_t count = 0;
    for ( uint32_t k = lane; k < vectors; k += SEARCH_THREADS ) {
        const uint64_t a = base + 16ull * k;
        const uint32_t candidates = matches16( fold16<FOLD>( v[k] ), first ) & validBytes16( a, begin, end );
        count += __popc( verified16<FOLD>( out, a, candidates, lds, m ) );
    }
#pragma unroll
    for ( uint32_t d = 32; d > 0; d >>= 1 ) count += __shfl_down( count, d );
    if ( lane == 0 ) {
        tileCounts[blockIdx.x] = count;
        if ( count != 0 ) atomicAdd( spanCounts + t.span, (unsigned long long)count );
    }
}

__global__ __launch_bounds__( SCAN_THREADS ) void
k_scan_tiles( const uint32_t* __restrict__ tileCounts, uint32_t nTiles, uint64_t* __restrict__ tileOffsets )
{
    __shared__ uint32_t waveSums[SCAN_THREADS / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    uint64_t before = 0;    /* the same in every thread */
    for ( uint32_t t0 = 0; t0 < nTiles; t0 += SCAN_THREADS ) {
        const uint32_t c = t0 + tid < nTiles ? tileCounts[t0 + tid] : 0u;
        const uint32_t upTo = waveInclusiveScan( c, lane );
        if ( lane == 63 ) waveSums[wave] = upTo;
        __syncthreads();
        uint32_t below = 0, all = 0;
#pragma unroll
        for ( uint32_t w = 0; w < SCAN_THREADS / 64; ++w ) {
            below += w < wave ? waveSums[w] : 0u;
            all += waveSums[w];
        }
        if ( t0 + tid < nTiles ) tileOffsets[t0 + tid] = before + below + ( upTo - c );
        before += all;
        __syncthreads();
    }
}

template<bool FOLD>
__global__ __launch_bounds__( SEARCH_THREADS ) void
k_emit_bytes( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, const uint8_t* __restrict__ pattern,
              uint32_t m, const uint64_t* __restrict__ tileOffsets, uint64_t capacity, uint64_t* __restrict__ positions )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[SEARCH_MAX_PATTERN];
    const uint32_t lane = threadIdx.x;
    uint64_t place = tileOffsets[blockIdx.x];    /* of the tile's next hit; the same in every lane */
    if ( place >= capacity ) return;
    loadPattern( lds, pattern, lane );
    const CountTile t = tiles[blockIdx.x];
    const uint64_t begin = t.src, end = t.src + t.size;
    const uint64_t base = begin & ~uint64_t( 15 );
    const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
    const uint4* const v = reinterpret_cast<const uint4*>( out + base );
    const uint32_t first = 0x01010101u * lds[0];

    for ( uint32_t k0 = 0; k0 < vectors; k0 += SEARCH_THREADS ) {
        const uint32_t k = k0 + lane;
        const uint64_t a = base + 16ull * k;
        uint32_t hits = 0;
        if ( k < vectors ) {
            hits = verified16<FOLD>( out, a, matches16( fold16<FOLD>( v[k] ), first ) & validBytes16( a, begin, end ), lds, m );
        }
        const uint32_t c = __popc( hits );
        const uint32_t upTo = waveInclusiveScan( c, lane );
        uint64_t mine = place + ( upTo - c );
        while ( hits != 0 && mine < capacity ) {
            positions[mine++] = a + (uint32_t)( __ffs( hits ) - 1 );
            hits &= hits - 1;
        }
        place += __shfl( upTo, 63 );
    }
}

/** dst[0, n) = out[src, src + n) and dst[SEARCH_MAX_PATTERN, SEARCH_MAX_PATTERN + n) = out[src + size - n, src + size).
 * The caller keeps n <= size and n < SEARCH_MAX_PATTERN. */
__global__ __launch_bounds__( 2 * SEARCH_MAX_PATTERN ) void
k_seam_bytes( const uint8_t* __restrict__ out, uint64_t src, uint64_t size, uint32_t n, uint8_t* __restrict__ dst )
{
    const uint32_t tid = threadIdx.x, i = tid & ( SEARCH_MAX_PATTERN - 1 );
    if ( i >= n ) return;
    dst[tid] = tid < SEARCH_MAX_PATTERN ? out[src + i] : out[src + size - n + i];
}
}  // namespace bz2gpu
