/**
 * bz2_fieldcols.hip.h -- a column of fields as packed bytes: the kernels of mi355x_bz2_gather_fields.  Given n spans
 * ( start, size ) in device memory, as k_field_emit / k_field_sizes write them, the bytes of every span with size > 0 go
 * back to back, in span order, to a destination, and offsets[0 .. n] receives where each begins: the exclusive prefix
 * sums of max( size, 0 ), offsets[n] the total.
 *
 *   k_fieldcol_sums     one workgroup per FIELDCOL_SCAN_TILE spans: the tile's sum of max( size, 0 ); and the check of
 *                       every span with size > 0 against the output -- ( start - base, size ) inside [0, outSize) --, the
 *                       offenders counted and the least index among them kept (two atomics per offender, none otherwise).
 *   k_fieldcol_top      one workgroup: the exclusive prefix sums of the tile sums, 256 per step, and the total.  For n
 *                       spans it scans n / FIELDCOL_SCAN_TILE values: 14 648 for 30 million lines, 58 steps.
 *   k_fieldcol_offsets  one workgroup per tile again: offsets[i] for the tile's spans, from the tile's prefix.
 *   k_field_gather      the copy, divided by OUTPUT bytes: one workgroup per FIELDCOL_TILE bytes of the destination, one
 *                       lane per 16-byte aligned destination vector and step.  The lane finds the span that owns its
 *                       first byte by a binary search in offsets (upper bound - 1: the spans that own nothing share their
 *                       offset with the next one and are never found), narrowed to the spans the tile touches, which
 *                       the workgroup's first lane finds the same way.  A vector that lies inside one span is read as
 *                       k_gather reads: four aligned dwords, or five shifted with v_alignbyte_b32, which reach up to 3
 *                       bytes behind the span -- the output buffer's 256 bytes of slack cover that.  Otherwise the lane
 *                       assembles its 16 bytes from byte loads, moving to the next owner at every span end: the next
 *                       span if that owns the byte, else a search again -- a million empty or missing fields between two
 *                       one-byte fields cost a search, not a walk.  Whole vectors are stored as 16 bytes, the partial ones
 *                       at the two ends of the destination byte by byte.  An 8 MB field spreads over 512 workgroups.
 *
 * The kernels run only when k_fieldcol_sums found no offender (the host waits for its counts), so k_field_gather reads
 * no byte outside the output and its slack.  64-bit offsets and places throughout; plain vector loads and stores; no
 * workgroup waits on another; every loop is bounded by the tile, by 16 bytes or by log2( n ).
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace bz2gpu
{
constexpr uint32_t FIELDCOL_THREADS = 256;
constexpr uint32_t FIELDCOL_PER_THREAD = 8;
constexpr uint32_t FIELDCOL_SCAN_TILE = FIELDCOL_THREADS * FIELDCOL_PER_THREAD;   /* spans per workgroup of the scan */
constexpr uint32_t FIELDCOL_TILE = 16384;                                         /* destination bytes per workgroup */
constexpr uint64_t FIELDCOL_NONE = ~uint64_t( 0 );

/** What k_fieldcol_sums and k_fieldcol_top leave for the host. */
struct FieldColumnCheck
{
    unsigned long long offenders, first, total;   /* first: FIELDCOL_NONE without an offender */
};

__device__ __forceinline__ uint64_t
fieldcolWaveInclusiveScan( uint64_t x, uint32_t lane )
{
#pragma unroll
    for ( uint32_t d = 1; d < 64; d <<= 1 ) {
        const uint64_t below = __shfl_up( (unsigned long long)x, d );
        if ( lane >= d ) x += below;
    }
    return x;
}

/** The exclusive prefix of `mine` over the workgroup's threads, and in *all their sum.  All threads call it. */
__device__ __forceinline__ uint64_t
fieldcolBlockExclusiveScan( uint64_t mine, uint64_t* waveSums, uint64_t* all )
{
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const uint64_t upTo = fieldcolWaveInclusiveScan( mine, lane );
    if ( lane == 63 ) waveSums[wave] = upTo;
    __syncthreads();
    uint64_t below = 0, sum = 0;
#pragma unroll
    for ( uint32_t w = 0; w < FIELDCOL_THREADS / 64; ++w ) {
        below += w < wave ? waveSums[w] : 0;
        sum += waveSums[w];
    }
    __syncthreads();
    *all = sum;
    return below + ( upTo - mine );
}

__global__ __launch_bounds__( FIELDCOL_THREADS ) void
k_fieldcol_sums( const uint64_t* __restrict__ starts, const int64_t* __restrict__ sizes, uint64_t n, uint64_t base,
                 uint64_t outSize, uint64_t* __restrict__ tileSums, FieldColumnCheck* __restrict__ check )
{
    __shared__ uint64_t waveSums[FIELDCOL_THREADS / 64];
    const uint64_t first = (uint64_t)blockIdx.x * FIELDCOL_SCAN_TILE + (uint64_t)threadIdx.x * FIELDCOL_PER_THREAD;
    uint64_t mine = 0;
#pragma unroll
    for ( uint32_t j = 0; j < FIELDCOL_PER_THREAD; ++j ) {
        const uint64_t i = first + j;
        if ( i >= n ) break;
        const int64_t size = sizes[i];
        if ( size <= 0 ) continue;
        const uint64_t start = starts[i];
        /* modulo 2^64, as the launcher's `base` may be: a start in front of it gives an offset beyond every output */
        const uint64_t offset = start - base;
        const bool inside = offset <= outSize && (uint64_t)size <= outSize - offset;
        if ( !inside ) {
            atomicAdd( &check->offenders, 1ull );
            atomicMin( &check->first, (unsigned long long)i );
            continue;
        }
        mine += (uint64_t)size;
    }
    uint64_t all;
    fieldcolBlockExclusiveScan( mine, waveSums, &all );
    if ( threadIdx.x == 0 ) tileSums[blockIdx.x] = all;
}

__global__ __launch_bounds__( FIELDCOL_THREADS ) void
k_fieldcol_top( const uint64_t* __restrict__ tileSums, uint64_t nTiles, uint64_t* __restrict__ tilePrefixes,
                FieldColumnCheck* __restrict__ check )
{
    __shared__ uint64_t waveSums[FIELDCOL_THREADS / 64];
    uint64_t before = 0;    /* the same in every thread */
    for ( uint64_t t0 = 0; t0 < nTiles; t0 += FIELDCOL_THREADS ) {
        const uint64_t t = t0 + threadIdx.x;
        uint64_t all;
        const uint64_t below = fieldcolBlockExclusiveScan( t < nTiles ? tileSums[t] : 0, waveSums, &all );
        if ( t < nTiles ) tilePrefixes[t] = before + below;
        before += all;
    }
    if ( threadIdx.x == 0 ) check->total = before;
}

__global__ __launch_bounds__( FIELDCOL_THREADS ) void
k_fieldcol_offsets( const int64_t* __restrict__ sizes, uint64_t n, const uint64_t* __restrict__ tilePrefixes,
                    const FieldColumnCheck* __restrict__ check, uint64_t* __restrict__ offsets )
{
    __shared__ uint64_t waveSums[FIELDCOL_THREADS / 64];
    const uint64_t first = (uint64_t)blockIdx.x * FIELDCOL_SCAN_TILE + (uint64_t)threadIdx.x * FIELDCOL_PER_THREAD;
    uint64_t size[FIELDCOL_PER_THREAD];
    uint64_t mine = 0;
#pragma unroll
    for ( uint32_t j = 0; j < FIELDCOL_PER_THREAD; ++j ) {
        const int64_t s = first + j < n ? sizes[first + j] : 0;
        size[j] = s > 0 ? (uint64_t)s : 0;
        mine += size[j];
    }
    uint64_t all;
    uint64_t at = tilePrefixes[blockIdx.x] + fieldcolBlockExclusiveScan( mine, waveSums, &all );
#pragma unroll
    for ( uint32_t j = 0; j < FIELDCOL_PER_THREAD; ++j ) {
        if ( first + j < n ) offsets[first + j] = at;
        at += size[j];
    }
    if ( blockIdx.x == 0 && threadIdx.x == 0 ) offsets[n] = check->total;
}

/** The span that owns byte p of the packed column: the largest i in [lo, hi] with offsets[i] <= p, given that
 * offsets[lo] <= p < offsets[hi + 1].  At most log2( hi - lo + 1 ) + 1 steps. */
__device__ __forceinline__ uint64_t
fieldcolOwner( const uint64_t* __restrict__ offsets, uint64_t lo, uint64_t hi, uint64_t p )
{
    while ( lo < hi ) {
        const uint64_t mid = lo + ( hi - lo + 1 ) / 2;
        if ( offsets[mid] <= p ) {
            lo = mid;
        } else {
            hi = mid - 1;
        }
    }
    return lo;
}

__global__ __launch_bounds__( FIELDCOL_THREADS ) void
k_field_gather( const uint64_t* __restrict__ starts, const uint64_t* __restrict__ offsets, uint64_t n, uint64_t base,
                uint64_t total, const uint8_t* __restrict__ out, uint8_t* __restrict__ dst )
{
    __shared__ uint64_t tileSpans[2];
    /* q = p + lead counts the destination's bytes from the 16-byte boundary in front of it: a vector is 16 | q */
    const uint64_t lead = reinterpret_cast<uintptr_t>( dst ) & 15u;
    const uint64_t q0 = (uint64_t)blockIdx.x * FIELDCOL_TILE, qEnd = lead + total;
    const uint64_t q1 = q0 + FIELDCOL_TILE < qEnd ? q0 + FIELDCOL_TILE : qEnd;
    if ( threadIdx.x == 0 ) {
        const uint64_t pFirst = q0 > lead ? q0 - lead : 0;
        tileSpans[0] = fieldcolOwner( offsets, 0, n - 1, pFirst );
        tileSpans[1] = fieldcolOwner( offsets, tileSpans[0], n - 1, q1 - lead - 1 );
    }
    __syncthreads();
    const uint64_t firstSpan = tileSpans[0], lastSpan = tileSpans[1];

    for ( uint64_t q = q0 + 16ull * threadIdx.x; q < q1; q += 16ull * FIELDCOL_THREADS ) {
        const uint64_t pLow = q > lead ? q - lead : 0, pHigh = ( q + 16 < qEnd ? q + 16 : qEnd ) - lead;
        uint64_t i = fieldcolOwner( offsets, firstSpan, lastSpan, pLow );
        uint64_t begin = offsets[i], end = offsets[i + 1];
        if ( pHigh - pLow == 16 && end >= pHigh ) {
            /* inside one span: k_gather's loads */
            const uint8_t* const s = out + ( starts[i] - base ) + ( pLow - begin );
            const uint32_t shift = (uint32_t)( reinterpret_cast<uintptr_t>( s ) & 3u );
            const uint32_t* const w = reinterpret_cast<const uint32_t*>( s - shift );
            uint4 v;
            if ( shift == 0 ) {
                v = make_uint4( w[0], w[1], w[2], w[3] );
            } else {
                const uint32_t w0 = w[0], w1 = w[1], w2 = w[2], w3 = w[3], w4 = w[4];
                v = make_uint4( __builtin_amdgcn_alignbyte( w1, w0, shift ), __builtin_amdgcn_alignbyte( w2, w1, shift ),
                                __builtin_amdgcn_alignbyte( w3, w2, shift ), __builtin_amdgcn_alignbyte( w4, w3, shift ) );
            }
            *reinterpret_cast<uint4*>( dst + pLow ) = v;
            continue;
        }
        /* byte k of the vector is packed byte q - lead + k; every round of the outer loop takes at least one byte */
        uint64_t low = 0, high = 0;
        uint64_t p = pLow;
        while ( p < pHigh ) {
            const uint64_t upTo = end < pHigh ? end : pHigh;
            const uint8_t* const s = out + ( starts[i] - base ) + ( p - begin );
            for ( uint64_t k = 0; k < upTo - p; ++k ) {
                const uint32_t at = (uint32_t)( p + k + lead - q );
                const uint64_t byte = s[k];
                if ( at < 8 ) {
                    low |= byte << ( 8 * at );
                } else {
                    high |= byte << ( 8 * ( at - 8 ) );
                }
            }
            p = upTo;
            if ( p < pHigh ) {
                /* p = end < total: some span behind i owns it, at most lastSpan */
                ++i;
                begin = end;
                end = offsets[i + 1];
                if ( end <= p ) {
                    i = fieldcolOwner( offsets, i, lastSpan, p );
                    begin = offsets[i];
                    end = offsets[i + 1];
                }
            }
        }
        if ( pHigh - pLow == 16 ) {
            *reinterpret_cast<uint4*>( dst + pLow ) = make_uint4( (uint32_t)low, (uint32_t)( low >> 32 ), (uint32_t)high,
                                                                  (uint32_t)( high >> 32 ) );
        } else {
            for ( uint64_t b = pLow; b < pHigh; ++b ) {
                const uint32_t at = (uint32_t)( b + lead - q );
                dst[b] = (uint8_t)( at < 8 ? low >> ( 8 * at ) : high >> ( 8 * ( at - 8 ) ) );
            }
        }
    }
}
}  // namespace bz2gpu
