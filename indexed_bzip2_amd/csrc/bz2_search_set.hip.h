/**
 * bz2_search_set.hip.h -- counting and listing the occurrences of a SET of byte strings S = (P_0 .. P_{k-1}) in spans of a
 * batch's ragged output, in one pass over the bytes: the kernels under mi355x_bz2_count_bytes_set /
 * mi355x_bz2_find_bytes_set, i.e. under the reader's search_set.  1 <= k <= SET_MAX_PATTERNS, 1 <= m_i <=
 * SEARCH_MAX_PATTERN, sum of the m_i <= SET_MAX_BYTES (bz2_search.hpp checks them and lays the set out).
 *
 * A match is a pair (p, i) with out[p : p + m_i] == P_i that lies inside its span; the order of a result is ascending p,
 * then ascending i.  The host cuts the start positions a span allows for its SHORTEST pattern -- [offset, offset + size -
 * m_min + 1) -- into tiles of at most SEARCH_TILE bytes.  Unlike bz2_search.hip.h's tiles these carry the span's end: a
 * candidate (p, i) with p + m_i > end is no match, and the verify never reads a byte at or behind the end.  The 16-byte
 * loads reach at most 15 bytes behind the last start position, as there.
 *
 * The set lives in LDS, loaded ONCE per workgroup (bz2_search.hpp, SET_TABLE_AT, describes the image): the pattern bytes,
 * one 32-bit entry per pattern ordered by (first byte, id), and a 256-entry table first byte -> bucket of entries.  A
 * workgroup is SET_WAVES waves; a tile is searched by ONE wave, and every wave takes tiles in a strided loop bounded by
 * the tile count, so that a 16-KiB set is not read again from L2 for every 16 KiB of data.  Nothing is exchanged between
 * waves but the set and the histogram; no wave waits on another inside the loop.
 *
 *   k_count_set   per position: the bucket of its byte, and every pattern of the bucket, in id order, verified byte by
 *                 byte against LDS until the first difference.  One count of pairs per tile (< 2^32: 16 384 x 1 024), one
 *                 64-bit atomic add per tile to its span's counter, and the per-pattern counts in an LDS histogram that
 *                 the workgroup adds to the global counters once, at its end, for the entries that are not zero.
 *   k_emit_set    the same walk, 64 vectors per step: a wave prefix sum over the lanes' pair counts places every lane's
 *                 pairs behind the tile's prefix sum (k_scan_tiles, unchanged), and the lane walks its vector a second
 *                 time and writes positions[place] and ids[place] in (position, id) order.  Places >= capacity are not
 *                 written; a wave stops at the first tile whose prefix sum has reached the capacity (the prefix sums
 *                 ascend with the tiles).  No atomics, no sort: the same call gives the same arrays.
 *
 * k_count_set and k_emit_set are templates over FOLD, as k_count_bytes is.  FOLD = true ignores the case of ASCII letters:
 * writeSetImage( set, image, true ) stores the patterns folded and builds the buckets by folded first byte, every vector is
 * folded once (fold16) where it is loaded, so that the table is indexed by the folded byte, and the verify folds the data
 * byte it compares.  The addresses read are those of FOLD = false.
 *
 * The pairs are recomputed by the emitting pass, not kept as a mask, as k_emit_bytes does and for the same reasons
 * (DESIGN.md).  k_seam_bytes of bz2_search.hip.h serves heads and tails of min( m_max - 1, size ) bytes.  Every loop is
 * bounded by the tile count, the tile's size, the bucket's length and m_i.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_search.hip.h"
#include "bz2_search.hpp"

namespace bz2gpu
{
constexpr uint32_t SET_WAVES = 4;
constexpr uint32_t SET_THREADS = 64 * SET_WAVES;
constexpr uint32_t SET_MAX_GROUPS = 2048;

struct SetTile
{
    uint64_t src;      /* in the batch's output */
    uint64_t end;      /* of the tile's span */
    uint32_t size;     /* start positions, <= SEARCH_TILE */
    uint32_t span;     /* whose counter the tile adds to */
};

/** The image of the set into LDS: the pattern bytes in use, the k entries, the 256 first bytes (16 bytes per step; the
 * image on the device is SET_IMAGE_BYTES whatever the set). */
__device__ __forceinline__ void
loadSet( uint8_t* lds, const uint8_t* __restrict__ image, uint32_t nBytes, uint32_t k, uint32_t tid )
{
    const uint4* const src = reinterpret_cast<const uint4*>( image );
    uint4* const dst = reinterpret_cast<uint4*>( lds );
    for ( uint32_t i = tid; i < ( nBytes + 15 ) / 16; i += SET_THREADS ) dst[i] = src[i];
    for ( uint32_t i = tid; i < ( k + 3 ) / 4; i += SET_THREADS ) dst[SET_TABLE_AT / 16 + i] = src[SET_TABLE_AT / 16 + i];
    for ( uint32_t i = tid; i < 64; i += SET_THREADS ) dst[SET_FIRST_AT / 16 + i] = src[SET_FIRST_AT / 16 + i];
    __syncthreads();
}

enum class SetWalk { COUNT_EACH, COUNT, WRITE };

/**
 * The pairs that start in the 16 bytes d = out[a, a + 16), at the positions of `valid`, in (position, id) order; returns
 * their number.  COUNT_EACH adds every pair to histogram[id] (LDS), WRITE stores pair number n at place + n while that is
 * below the capacity.  FOLD: d and the set in LDS are folded, and the verify folds the bytes it reads.
 */
template<SetWalk WALK, bool FOLD>
__device__ __forceinline__ uint32_t
pairs16( const uint8_t* __restrict__ out, uint64_t a, uint4 d, uint32_t valid, uint64_t spanEnd, const uint8_t* lds,
         uint32_t* histogram, uint64_t place, uint64_t capacity, uint64_t* __restrict__ positions, uint32_t* __restrict__ ids )
{
    const uint32_t* const table = reinterpret_cast<const uint32_t*>( lds + SET_TABLE_AT );
    const uint32_t* const first = reinterpret_cast<const uint32_t*>( lds + SET_FIRST_AT );
    uint32_t n = 0;
    while ( valid != 0 ) {
        const uint32_t bit = (uint32_t)__ffs( valid ) - 1;
        valid &= valid - 1;
        const uint32_t word = bit < 8 ? ( bit < 4 ? d.x : d.y ) : ( bit < 12 ? d.z : d.w );
        const uint32_t bucket = first[( word >> ( 8 * ( bit & 3 ) ) ) & 0xFFu];
        if ( bucket == 0 ) continue;
        const uint64_t p = a + bit;
        const uint8_t* const at = out + p;
        const uint64_t room = spanEnd - p;    /* >= m_min: p is a start position of the span */
        const uint32_t begin = bucket & 0xFFFFu, length = bucket >> 16;
        for ( uint32_t e = begin; e < begin + length; ++e ) {
            const uint32_t entry = table[e];
            const uint32_t m = ( ( entry >> SET_ENTRY_SIZE_SHIFT ) & 0xFFu ) + 1;
            if ( m > room ) continue;
            const uint8_t* const pattern = lds + ( entry & ( SET_MAX_BYTES - 1 ) );
            uint32_t j = 1;
            while ( j < m && foldByte<FOLD>( at[j] ) == pattern[j] ) ++j;
            if ( j != m ) continue;
            const uint32_t id = entry >> SET_ENTRY_ID_SHIFT;
            if constexpr ( WALK == SetWalk::COUNT_EACH ) atomicAdd( histogram + id, 1u );
            if constexpr ( WALK == SetWalk::WRITE ) {
                if ( place + n >= capacity ) return n;
                positions[place + n] = p;
                ids[place + n] = id;
            }
            ++n;
        }
    }
    return n;
}

template<bool FOLD>
__global__ __launch_bounds__( SET_THREADS ) void
k_count_set( const SetTile* __restrict__ tiles, uint32_t nTiles, const uint8_t* __restrict__ out,
             const uint8_t* __restrict__ image, uint32_t nBytes, uint32_t k, uint32_t* __restrict__ tileCounts,
             unsigned long long* __restrict__ spanCounts, unsigned long long* __restrict__ perPattern )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[SET_IMAGE_BYTES];
    __shared__ uint32_t histogram[SET_MAX_PATTERNS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for ( uint32_t i = tid; i < k; i += SET_THREADS ) histogram[i] = 0;
    loadSet( lds, image, nBytes, k, tid );

    for ( uint32_t tile = blockIdx.x * SET_WAVES + wave; tile < nTiles; tile += gridDim.x * SET_WAVES ) {
        const SetTile t = tiles[tile];
        const uint64_t begin = t.src, end = t.src + t.size;
        const uint64_t base = begin & ~uint64_t( 15 );
        const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
        const uint4* const v = reinterpret_cast<const uint4*>( out + base );
        uint32_t count = 0;
        for ( uint32_t i = lane; i < vectors; i += 64 ) {
            const uint64_t a = base + 16ull * i;
            count += pairs16<SetWalk::COUNT_EACH, FOLD>( out, a, fold16<FOLD>( v[i] ), validBytes16( a, begin, end ), t.end, lds,
                                                         histogram, 0, 0, nullptr, nullptr );
        }
#pragma unroll
        for ( uint32_t d = 32; d > 0; d >>= 1 ) count += __shfl_down( count, d );
        if ( lane == 0 ) {
            tileCounts[tile] = count;
            if ( count != 0 ) atomicAdd( spanCounts + t.span, (unsigned long long)count );
        }
    }
    __syncthreads();
    for ( uint32_t i = tid; i < k; i += SET_THREADS ) {
        if ( histogram[i] != 0 ) atomicAdd( perPattern + i, (unsigned long long)histogram[i] );
    }
}

template<bool FOLD>
__global__ __launch_bounds__( SET_THREADS ) void
k_emit_set( const SetTile* __restrict__ tiles, uint32_t nTiles, const uint8_t* __restrict__ out,
            const uint8_t* __restrict__ image, uint32_t nBytes, uint32_t k, const uint64_t* __restrict__ tileOffsets,
            uint64_t capacity, uint64_t* __restrict__ positions, uint32_t* __restrict__ ids )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[SET_IMAGE_BYTES];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    loadSet( lds, image, nBytes, k, tid );

    for ( uint32_t tile = blockIdx.x * SET_WAVES + wave; tile < nTiles; tile += gridDim.x * SET_WAVES ) {
        uint64_t place = tileOffsets[tile];    /* of the tile's next pair; the same in every lane */
        if ( place >= capacity ) break;        /* and so has every tile behind this one */
        const SetTile t = tiles[tile];
        const uint64_t begin = t.src, end = t.src + t.size;
        const uint64_t base = begin & ~uint64_t( 15 );
        const uint32_t vectors = (uint32_t)( ( end - base + 15 ) >> 4 );
        const uint4* const v = reinterpret_cast<const uint4*>( out + base );
        for ( uint32_t i0 = 0; i0 < vectors; i0 += 64 ) {
            const uint32_t i = i0 + lane;
            const uint64_t a = base + 16ull * i;
            uint4 d{ 0, 0, 0, 0 };
            uint32_t valid = 0, c = 0;
            if ( i < vectors ) {
                d = fold16<FOLD>( v[i] );
                valid = validBytes16( a, begin, end );
                c = pairs16<SetWalk::COUNT, FOLD>( out, a, d, valid, t.end, lds, nullptr, 0, 0, nullptr, nullptr );
            }
            const uint32_t upTo = waveInclusiveScan( c, lane );
            const uint64_t mine = place + ( upTo - c );
            if ( c != 0 && mine < capacity ) {
                pairs16<SetWalk::WRITE, FOLD>( out, a, d, valid, t.end, lds, nullptr, mine, capacity, positions, ids );
            }
            place += __shfl( upTo, 63 );
        }
    }
}
}  // namespace bz2gpu
