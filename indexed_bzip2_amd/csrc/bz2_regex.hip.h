/**
 * bz2_regex.hip.h -- one offset inside every line that matches a regular expression, in spans of a batch's ragged
 * output: the kernels under mi355x_bz2_match_lines, i.e. under the reader's grep_regex.  bz2_regex.hpp has the automaton
 * (state 0 = start of a line, state 1 = A = "this line has matched"), the summary of a stretch and the rule that
 * composes summaries; these kernels apply that rule between the chunks of a span.
 *
 * A span is cut into chunks of REGEX_CHUNK bytes, one lane per chunk, REGEX_THREADS chunks -- one tile of COUNT_TILE
 * bytes, the CountTile of bz2_lines.hip.h -- per workgroup.  Chunk k of a span is slot (span's first tile) *
 * REGEX_THREADS + k of the per-chunk arrays: only the last tile of a span is partial, and its unused slots count 0.
 *
 * The chunk size.  A lane pays up to n table steps per byte of its chunk's head (the bytes in front of the chunk's first
 * nl: it does not know the state it is entered in, so it runs all n) and one per byte behind it.  A head is as long as
 * the rest of a line, whatever the chunk size, so a larger chunk dilutes it: with lines of about 100 bytes the head is a
 * fifth of a 256-byte chunk and a twentieth of a 1-KiB one.  Against that stand (a) parallelism -- a launch of one
 * 100-kB block is 400 chunks of 256 bytes, six waves, but one and a half waves of 1-KiB chunks, and every wave runs as
 * long as its longest head --, (b) the data without delimiters, where every chunk is all head and only the number of
 * lanes hides the n-fold cost, and (c) the per-chunk summary, n bytes rounded up to 16 plus 8, which at 256 bytes is
 * 9 to 28 % of the data and shrinks in proportion.  256 bytes keeps small launches parallel and lets one tile of the
 * existing 64-KiB tiling be one workgroup; tools/regex_probe.py measures what it costs on large ones.
 *
 * How a lane reads its chunk.  Lanes that each walked their own chunk with global loads would touch 64 cache lines per
 * load instruction.  Instead a wave stages its 64 chunks through LDS in REGEX_PASSES passes of REGEX_PIECE = 64 bytes
 * per chunk: the five aligned 16-byte vectors that cover a chunk's piece (a span starts at any alignment; all pieces of a
 * tile share the shift src & 15) are loaded by five of eight adjacent lanes, eight chunks per load instruction, whole
 * 64-byte sectors each, and written to the chunk's row.  A row is 21 dwords: 20 of data and one of padding, so that the
 * 32 lanes of an LDS lane group, which read the same byte of their rows, hit 32 different banks (21 is odd).  The
 * vectors reach at most 15 bytes in front of a tile (the buffer is 16-byte aligned) and never a vector that starts at or
 * behind the tile's end.
 *
 * The table (n * 256 bytes, at most 16 KiB) and acceptsAtEnd live in LDS, transitions[state][byte] as the host has it: the
 * lanes of a wave are in few states and read different bytes, which spreads them over the 64 dwords of a state's row.
 * With the staging rows (4 waves * 64 * 84 bytes) a workgroup holds 38 KiB: four workgroups, 16 waves, per CU.
 *
 *   k_regex_chunks  per chunk: headMap[q] for all n entry states (packed four to a register, so that no lane indexes an
 *                   array), hasDelimiter, exit, and the number of body witnesses (the body runs once, from state 0).
 *   k_regex_link    one workgroup per span scans the chunk summaries by composition, REGEX_THREADS chunks per step.  An
 *                   element is a function entry state -> state behind the chunk: a constant (the chunk holds nl: its
 *                   exit) or the chunk's headMap.  compose( a, b ) = b if b is constant, the constant b[a] if a is,
 *                   else the map q -> b[a[q]].  Inside a step the elements are scanned in LDS in log2( REGEX_THREADS )
 *                   rounds; between steps one carry element is composed in front.  Every chunk behind the span's first
 *                   delimiter so gets its entry state and adds its head hit (0 or 1) to its count; the chunk with the
 *                   span's first delimiter composes the span's headMap; the last carry is the span's exit.  No chain of
 *                   dependent global loads: a step loads its 256 summaries at once.
 *   k_scan_tiles    (bz2_search.hip.h) the exclusive prefix sums of the chunk counts, as they are.
 *   k_regex_emit    recomputes each chunk's body and writes its witnesses, the head hit (the chunk's first byte) first,
 *                   at its prefix sum; nothing is written at or beyond `capacity`, and a tile whose first place is
 *                   already there returns at once.
 *
 * Every loop is bounded by the chunk, by n or by the number of chunks; no workgroup waits on another; vector stores only.
 */
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "bz2_lines.hip.h"

namespace bz2gpu
{
constexpr uint32_t REGEX_CHUNK = 256;
constexpr uint32_t REGEX_THREADS = 256;                     /* chunks per tile and per step of the link */
constexpr uint32_t REGEX_PIECE = 64;
constexpr uint32_t REGEX_PASSES = REGEX_CHUNK / REGEX_PIECE;
constexpr uint32_t REGEX_ROW_DWORDS = 21;                   /* 80 bytes of data, 4 of padding */
constexpr uint32_t REGEX_STATES = 64;                       /* REGEX_MAX_STATES of bz2_regex.hpp */
constexpr uint32_t REGEX_LINK_ROW_DWORDS = 17;              /* 64 bytes of map, 4 of padding */
constexpr uint32_t REGEX_HAS_DELIMITER = 1u, REGEX_EXIT_SHIFT = 8, REGEX_HEAD_HIT = 1u << 16;
static_assert( REGEX_CHUNK * REGEX_THREADS == COUNT_TILE, "a tile is one workgroup" );

/** What k_regex_link is told about a span. */
struct RegexSpan
{
    uint32_t firstSlot;    /* of its chunks in the per-chunk arrays */
    uint32_t nChunks;
};

/** Bytes of one chunk's headMap in global memory: n rounded up to whole 16-byte vectors. */
__host__ __device__ constexpr uint32_t
regexMapStride( uint32_t n )
{
    return ( n + 15u ) & ~15u;
}

__device__ __forceinline__ void
loadRegexTable( uint8_t* lds, uint8_t* ldsAccepts, const uint8_t* __restrict__ table, const uint8_t* __restrict__ accepts,
                uint32_t n, uint32_t tid )
{
    for ( uint32_t k = tid; k < n * 64; k += REGEX_THREADS ) {
        reinterpret_cast<uint32_t*>( lds )[k] = reinterpret_cast<const uint32_t*>( table )[k];
    }
    if ( tid < REGEX_STATES ) ldsAccepts[tid] = tid < n ? accepts[tid] : uint8_t( 0 );
    __syncthreads();
}

/** One workgroup walks one tile, one lane per chunk.  EMIT false: the chunk's summary and count.  EMIT true: its
 * witnesses. */
template<bool EMIT>
__device__ __forceinline__ void
regexTile( const CountTile t, const uint8_t* __restrict__ out, const uint8_t* __restrict__ table,
           const uint8_t* __restrict__ accepts, uint32_t n, uint32_t nl, uint8_t* headMaps, uint32_t* info, uint32_t* counts,
           const uint64_t* places, uint64_t capacity, uint64_t* positions )
{
    __shared__ __attribute__( ( aligned( 16 ) ) ) uint8_t lds[REGEX_STATES * 256];
    __shared__ uint8_t ldsAccepts[REGEX_STATES];
    __shared__ uint32_t stage[REGEX_THREADS / 64][64 * REGEX_ROW_DWORDS];
    const uint32_t tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    loadRegexTable( lds, ldsAccepts, table, accepts, n, tid );

    const uint64_t slot = (uint64_t)blockIdx.x * REGEX_THREADS + tid;
    const uint64_t tileEnd = t.src + t.size;
    const uint64_t chunkBegin = t.src + (uint64_t)tid * REGEX_CHUNK;
    const uint32_t chunkSize = chunkBegin < tileEnd ? (uint32_t)( tileEnd - chunkBegin < REGEX_CHUNK ? tileEnd - chunkBegin : REGEX_CHUNK ) : 0u;
    const uint32_t shift = (uint32_t)( t.src & 15 );
    const uint8_t* const row = reinterpret_cast<const uint8_t*>( stage[wave] + lane * REGEX_ROW_DWORDS ) + shift;

    /* the head: state q of group g is byte q & 3 of hm[q >> 2]; states >= n ride along as state 0 */
    uint32_t hm[REGEX_STATES / 4];
    if constexpr ( !EMIT ) {
#pragma unroll
        for ( uint32_t g = 0; g < REGEX_STATES / 4; ++g ) {
            hm[g] = 0;
#pragma unroll
            for ( uint32_t k = 0; k < 4; ++k ) hm[g] |= ( 4 * g + k < n ? 4 * g + k : 0u ) << ( 8 * k );
        }
    }
    bool inHead = true;
    uint32_t state = 0, count = 0;
    uint64_t place = 0;
    if constexpr ( EMIT ) {
        if ( chunkSize > 0 ) {
            place = places[slot];
            if ( ( info[slot] & REGEX_HEAD_HIT ) != 0 && place < capacity ) positions[place] = chunkBegin;
            place += ( info[slot] & REGEX_HEAD_HIT ) != 0 ? 1 : 0;
        }
    }

    for ( uint32_t pass = 0; pass < REGEX_PASSES; ++pass ) {
        /* stage the pass's piece of the wave's 64 chunks: lanes 8 r' .. 8 r' + 4 load the five vectors of row r */
        const uint32_t j = lane & 7;
#pragma unroll
        for ( uint32_t k = 0; k < 8; ++k ) {
            const uint32_t r = ( lane >> 3 ) + 8 * k;
            const uint64_t pieceBegin = t.src + (uint64_t)( wave * 64 + r ) * REGEX_CHUNK + pass * REGEX_PIECE;
            const uint64_t pieceEnd = pieceBegin + REGEX_PIECE < tileEnd ? pieceBegin + REGEX_PIECE : tileEnd;
            const uint64_t vector = ( pieceBegin & ~uint64_t( 15 ) ) + 16ull * j;
            if ( j < 5 && vector < pieceEnd ) {
                const uint4 d = *reinterpret_cast<const uint4*>( out + vector );
                uint32_t* const to = stage[wave] + r * REGEX_ROW_DWORDS + 4 * j;
                to[0] = d.x;
                to[1] = d.y;
                to[2] = d.z;
                to[3] = d.w;
            }
        }
        __syncthreads();
        const uint32_t done = pass * REGEX_PIECE;
        const uint32_t valid = chunkSize > done ? ( chunkSize - done < REGEX_PIECE ? chunkSize - done : REGEX_PIECE ) : 0u;
        for ( uint32_t i = 0; i < valid; ++i ) {
            const uint32_t b = row[i];
            if ( inHead ) {
                if ( b == nl ) {
                    inHead = false;
                    state = 0;
                    continue;
                }
                if constexpr ( !EMIT ) {
#pragma unroll
                    for ( uint32_t g = 0; g < REGEX_STATES / 4; ++g ) {
                        if ( 4 * g < n ) {
                            const uint32_t w = hm[g];
                            hm[g] = (uint32_t)lds[( w & 0xFFu ) * 256 + b] | ( (uint32_t)lds[( ( w >> 8 ) & 0xFFu ) * 256 + b] << 8 )
                                    | ( (uint32_t)lds[( ( w >> 16 ) & 0xFFu ) * 256 + b] << 16 ) | ( (uint32_t)lds[( w >> 24 ) * 256 + b] << 24 );
                        }
                    }
                }
                continue;
            }
            bool witness;
            if ( b == nl ) {
                witness = state != 1 && ldsAccepts[state] != 0;
                state = 0;
            } else {
                const uint32_t next = lds[state * 256 + b];
                witness = next == 1 && state != 1;
                state = next;
            }
            if ( witness ) {
                if constexpr ( EMIT ) {
                    if ( place < capacity ) positions[place] = chunkBegin + done + i;
                    ++place;
                } else {
                    ++count;
                }
            }
        }
        __syncthreads();    /* the next pass overwrites the rows */
    }

    if constexpr ( !EMIT ) {
        /* states >= n read 0, as the host's summary has them */
#pragma unroll
        for ( uint32_t g = 0; g < REGEX_STATES / 4; ++g ) {
            uint32_t mask = 0;
#pragma unroll
            for ( uint32_t k = 0; k < 4; ++k ) mask |= ( 4 * g + k < n ? 0xFFu : 0u ) << ( 8 * k );
            hm[g] &= mask;
        }
        uint4* const to = reinterpret_cast<uint4*>( headMaps + slot * regexMapStride( n ) );
#pragma unroll
        for ( uint32_t v = 0; v < REGEX_STATES / 16; ++v ) {
            if ( 16 * v < n ) to[v] = uint4{ hm[4 * v], hm[4 * v + 1], hm[4 * v + 2], hm[4 * v + 3] };
        }
        info[slot] = inHead ? 0u : ( REGEX_HAS_DELIMITER | ( state << REGEX_EXIT_SHIFT ) );
        counts[slot] = count;
    }
}

__global__ __launch_bounds__( REGEX_THREADS ) void
k_regex_chunks( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, const uint8_t* __restrict__ table,
                const uint8_t* __restrict__ accepts, uint32_t n, uint32_t nl, uint8_t* __restrict__ headMaps,
                uint32_t* __restrict__ info, uint32_t* __restrict__ counts )
{
    regexTile<false>( tiles[blockIdx.x], out, table, accepts, n, nl, headMaps, info, counts, nullptr, 0, nullptr );
}

__global__ __launch_bounds__( REGEX_THREADS ) void
k_regex_emit( const CountTile* __restrict__ tiles, const uint8_t* __restrict__ out, const uint8_t* __restrict__ table,
              const uint8_t* __restrict__ accepts, uint32_t n, uint32_t nl, uint32_t* __restrict__ info,
              const uint64_t* __restrict__ places, uint64_t capacity, uint64_t* __restrict__ positions )
{
    /* the same in every lane: the places ascend with the slots */
    if ( places[(uint64_t)blockIdx.x * REGEX_THREADS] >= capacity ) return;
    regexTile<true>( tiles[blockIdx.x], out, table, accepts, n, nl, nullptr, info, nullptr, places, capacity, positions );
}

__global__ __launch_bounds__( REGEX_THREADS ) void
k_regex_link( const RegexSpan* __restrict__ spans, const uint8_t* __restrict__ accepts, uint32_t n,
              const uint8_t* __restrict__ headMaps, uint32_t* info, uint32_t* counts, uint8_t* __restrict__ spanHeadMaps,
              uint32_t* __restrict__ spanInfo, unsigned long long* __restrict__ spanCounts )
{
    __shared__ uint32_t maps[REGEX_THREADS * REGEX_LINK_ROW_DWORDS];
    __shared__ uint8_t kind[REGEX_THREADS], value[REGEX_THREADS];    /* kind 1: the constant `value`; 0: the map of the row */
    __shared__ uint8_t carryMap[REGEX_STATES], ldsAccepts[REGEX_STATES];
    __shared__ uint32_t carryKind, carryValue;
    __shared__ unsigned long long total;
    const uint32_t tid = threadIdx.x;
    const RegexSpan span = spans[blockIdx.x];
    const uint32_t stride = regexMapStride( n ), vectorsPerRow = stride / 16;
    const auto rowByte = [&] ( uint32_t r, uint32_t q ) -> uint32_t {
        return reinterpret_cast<const uint8_t*>( maps + r * REGEX_LINK_ROW_DWORDS )[q];
    };
    if ( tid < REGEX_STATES ) {
        carryMap[tid] = (uint8_t)tid;
        ldsAccepts[tid] = tid < n ? accepts[tid] : uint8_t( 0 );
    }
    if ( tid == 0 ) {
        carryKind = 0;
        carryValue = 0;
        total = 0;
    }
    __syncthreads();

    unsigned long long sum = 0;
    for ( uint32_t c0 = 0; c0 < span.nChunks; c0 += REGEX_THREADS ) {
        const uint32_t m = span.nChunks - c0 < REGEX_THREADS ? span.nChunks - c0 : REGEX_THREADS;
        const uint64_t slot = (uint64_t)span.firstSlot + c0 + tid;
        const uint4* const from = reinterpret_cast<const uint4*>( headMaps + ( (uint64_t)span.firstSlot + c0 ) * stride );
        for ( uint32_t v = tid; v < m * vectorsPerRow; v += REGEX_THREADS ) {
            const uint4 d = from[v];
            uint32_t* const to = maps + ( v / vectorsPerRow ) * REGEX_LINK_ROW_DWORDS + 4 * ( v % vectorsPerRow );
            to[0] = d.x;
            to[1] = d.y;
            to[2] = d.z;
            to[3] = d.w;
        }
        const uint32_t mine = tid < m ? info[slot] : 0u;
        const bool hasDelimiter = ( mine & REGEX_HAS_DELIMITER ) != 0;
        kind[tid] = hasDelimiter ? 1 : 0;
        value[tid] = (uint8_t)( mine >> REGEX_EXIT_SHIFT );
        __syncthreads();

        /* inclusive scan by composition: after the round with distance d, row i is the composition of chunks
         * ( i - 2d, i ] of the step */
        for ( uint32_t d = 1; d < REGEX_THREADS; d <<= 1 ) {
            const bool active = tid >= d && tid < m && kind[tid] == 0;
            bool toConstant = false;
            uint32_t newValue = 0;
            uint32_t newMap[REGEX_STATES / 4];
            if ( active ) {
                if ( kind[tid - d] != 0 ) {
                    toConstant = true;
                    newValue = rowByte( tid, value[tid - d] );
                } else {
#pragma unroll
                    for ( uint32_t g = 0; g < REGEX_STATES / 4; ++g ) {
                        if ( 4 * g < n ) {
                            const uint32_t a = maps[( tid - d ) * REGEX_LINK_ROW_DWORDS + g];
                            newMap[g] = rowByte( tid, a & 0xFFu ) | ( rowByte( tid, ( a >> 8 ) & 0xFFu ) << 8 )
                                        | ( rowByte( tid, ( a >> 16 ) & 0xFFu ) << 16 ) | ( rowByte( tid, a >> 24 ) << 24 );
                        }
                    }
                }
            }
            __syncthreads();
            if ( active ) {
                if ( toConstant ) {
                    kind[tid] = 1;
                    value[tid] = (uint8_t)newValue;
                } else {
#pragma unroll
                    for ( uint32_t g = 0; g < REGEX_STATES / 4; ++g ) {
                        if ( 4 * g < n ) maps[tid * REGEX_LINK_ROW_DWORDS + g] = newMap[g];
                    }
                }
            }
            __syncthreads();
        }

        if ( tid < m ) {
            /* the state the chunk is entered in: the carry, then the chunks of the step in front of it */
            constexpr uint32_t UNKNOWN = 0xFFu;    /* no delimiter in front of the chunk: the span's head line */
            uint32_t entry = UNKNOWN;
            if ( tid > 0 && kind[tid - 1] != 0 ) {
                entry = value[tid - 1];
            } else if ( carryKind != 0 ) {
                entry = tid > 0 ? rowByte( tid - 1, carryValue ) : carryValue;
            }
            const uint8_t* const own = headMaps + slot * stride;
            uint32_t hit = 0;
            if ( entry != UNKNOWN && entry != 1 ) {
                const uint32_t behind = own[entry];
                hit = behind == 1 || ( hasDelimiter && ldsAccepts[behind] != 0 ) ? 1 : 0;
            }
            const uint32_t count = counts[slot] + hit;
            if ( hit != 0 ) {
                counts[slot] = count;
                info[slot] = mine | REGEX_HEAD_HIT;
            }
            sum += count;
            if ( entry == UNKNOWN && hasDelimiter ) {
                /* the span's first delimiter: its head ends in this chunk */
                for ( uint32_t q = 0; q < REGEX_STATES; ++q ) {
                    uint32_t s = 0;
                    if ( q < n ) {
                        s = carryMap[q];
                        if ( tid > 0 ) s = rowByte( tid - 1, s );
                        s = own[s];
                    }
                    spanHeadMaps[(uint64_t)blockIdx.x * REGEX_STATES + q] = (uint8_t)s;
                }
            }
        }
        __syncthreads();
        /* the carry behind this step */
        const uint32_t last = m - 1;
        if ( kind[last] != 0 ) {
            if ( tid == 0 ) {
                carryKind = 1;
                carryValue = value[last];
            }
        } else if ( carryKind != 0 ) {
            if ( tid == 0 ) carryValue = rowByte( last, carryValue );
        } else if ( tid < n ) {
            carryMap[tid] = (uint8_t)rowByte( last, carryMap[tid] );
        }
        __syncthreads();
    }

    if ( carryKind == 0 && tid < REGEX_STATES ) {
        spanHeadMaps[(uint64_t)blockIdx.x * REGEX_STATES + tid] = tid < n ? carryMap[tid] : uint8_t( 0 );
    }
    if ( sum != 0 ) atomicAdd( &total, sum );
    __syncthreads();
    if ( tid == 0 ) {
        spanInfo[blockIdx.x] = carryKind != 0 ? ( REGEX_HAS_DELIMITER | ( carryValue << REGEX_EXIT_SHIFT ) ) : 0u;
        spanCounts[blockIdx.x] = total;
    }
}
}  // namespace bz2gpu
