/**
 * bz2_compress.hip -- mi355x_bz2_compress_buffers: bzip2 compression of many buffers in shared GPU launches.
 *
 * The host cuts every buffer into libbz2's blocks and the blocks of all buffers into launches (bz2_compress.hpp).  Per
 * launch, on the context's stream:
 *   CRC        k_crc over the launch's input (mi355x_bz2_crc32_device): every block's CRC over its original bytes
 *   k_enc_rle1     one workgroup per block: RLE1 into the block's positions, the byte values in use
 *   BWT        prefix doubling over cyclic rotations: rotations sorted by (block, first 4 bytes) with rocPRIM's radix
 *              sort, then rounds h = 4, 8, ... that re-sort only the slots of groups still tied by (rank, rank at +h);
 *              a rank is the slot of its group's first member, a position in the launch, so it fits in 32 bits.  A block
 *              drops out once h reaches its length: rotations still tied are then equal, in any order.
 *   k_bwt_finish   L column and origPtr
 *   k_enc_mtf      one wave per block: MTF over the used-symbol alphabet with RUNA/RUNB zero runs and EOB
 *   k_enc_tables   one workgroup per block: bzip2's 2..6 tables (equal-frequency start, four rounds of selection and
 *                  Huffman lengths capped at 17), selector MTF, canonical codes, the block's exact bit length
 *   k_enc_emit     one workgroup per block, at the block's absolute bit offset (from the host's scan of the lengths):
 *                  the header by one thread, one thread per 50-symbol group after it
 * and, once all launches have run, k_enc_frame writes every stream's "BZh<level>" and end-of-stream trailer.  Output
 * words are big-endian; the output is zeroed first, words a writer owns whole are stored, boundary words OR-ed.
 */
#include <hip/hip_runtime.h>

#include <rocprim/device/device_radix_sort.hpp>
#include <rocprim/device/device_scan.hpp>
#include <rocprim/device/device_select.hpp>

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "../../include/mi355x_bz2.h"
#include "bz2_compress.hpp"
#include "bz2_ctx.hpp"

namespace
{
using namespace mi355x::compress;

constexpr int MAX_TABLES = 6;
constexpr int MAX_ALPHA = 258;
constexpr int MAX_CODE_LENGTH = 17;
constexpr uint32_t PLAN_THREADS = 16;                   /* host threads of the block planner */
constexpr uint64_t PLAN_THREAD_BYTES = 16u << 20;       /* below this much input one thread plans */

struct EncBlock
{
    uint64_t inOff;    /* of its bytes in the launch's input */
    uint32_t inSize;
    uint32_t pos;      /* first RLE1 position in the launch */
    uint32_t n;        /* RLE1 bytes */
    uint32_t sym;      /* first symbol slot */
    uint32_t sel;      /* first selector slot */
    uint32_t crc;
};

struct EncMeta
{
    uint32_t inUse[8];
    uint32_t rleCount;     /* RLE1 bytes written (== n) */
    uint32_t origPtr;
    uint32_t nInUse;
    uint32_t nMTF;
    uint32_t nGroups;
    uint32_t nSel;
    uint32_t headerBits;
    uint32_t dataBits;
    uint32_t emitted;      /* header bits the emit kernel wrote (== headerBits) */
    uint32_t reserved;
};

struct EncTables
{
    uint8_t len[MAX_TABLES][MAX_ALPHA];
    uint32_t code[MAX_TABLES][MAX_ALPHA];
};

struct FrameJob
{
    uint64_t bit;
    uint32_t kind;     /* 0: "BZh<value>", 1: end-of-stream magic and CRC <value> */
    uint32_t value;
};

/* ------------------------------------------------------------------------------------------------ device helpers */

/** MSB-first bits into a zeroed buffer of big-endian 32-bit words: words the writer owns whole are stored, its first
 * word (if it starts inside one) and its last partial word are OR-ed, since a neighbour writes the rest of them. */
struct BitWriter
{
    uint32_t* words;
    uint64_t wi;
    uint64_t acc{ 0 };
    uint32_t fill;
    bool shared;
    uint64_t written{ 0 };

    __device__ BitWriter( uint32_t* w, uint64_t bit ) : words( w ), wi( bit >> 5 ), fill( bit & 31 ), shared( ( bit & 31 ) != 0 ) {}

    /** the low `n` bits of v, 1 <= n <= 32 */
    __device__ void
    put( uint32_t v, uint32_t n )
    {
        acc |= (uint64_t)v << ( 64 - fill - n );
        fill += n;
        written += n;
        if ( fill >= 32 ) {
            word( (uint32_t)( acc >> 32 ), shared );
            shared = false;
            acc <<= 32;
            fill -= 32;
            ++wi;
        }
    }

    __device__ void
    finish()
    {
        if ( fill > 0 ) word( (uint32_t)( acc >> 32 ), true );
    }

    __device__ void
    word( uint32_t x, bool atomic )
    {
        x = __builtin_bswap32( x );
        if ( atomic ) {
            if ( x != 0 ) atomicOr( words + wi, x );
        } else {
            words[wi] = x;
        }
    }
};

/** The block of launch position `p` (blocks ascending by pos). */
__device__ inline uint32_t
blockOf( const EncBlock* blocks, uint32_t nBlocks, uint32_t p )
{
    uint32_t lo = 0, hi = nBlocks - 1;
    while ( lo < hi ) {
        const uint32_t mid = ( lo + hi + 1 ) / 2;
        if ( blocks[mid].pos <= p ) lo = mid; else hi = mid - 1;
    }
    return lo;
}

/* ------------------------------------------------------------------------------------------------ RLE1 */

constexpr int RLE_THREADS = 256;
constexpr int RLE_BYTES = 16;   /* per thread and tile */

/** Inclusive scan over the workgroup of (full, value): a later element that is `full` continues the run of the one
 * before it (value += earlier value), one that is not starts afresh. */
__device__ inline void
scanRuns( uint32_t* sFull, uint32_t* sVal, uint32_t tid )
{
    for ( uint32_t d = 1; d < RLE_THREADS; d <<= 1 ) {
        uint32_t full = sFull[tid], val = sVal[tid];
        if ( tid >= d && full ) {
            full = sFull[tid - d];
            val += sVal[tid - d];
        }
        __syncthreads();
        sFull[tid] = full;
        sVal[tid] = val;
        __syncthreads();
    }
}

__device__ inline void
scanSum( uint32_t* s, uint32_t tid )
{
    for ( uint32_t d = 1; d < RLE_THREADS; d <<= 1 ) {
        const uint32_t v = s[tid] + ( tid >= d ? s[tid - d] : 0 );
        __syncthreads();
        s[tid] = v;
        __syncthreads();
    }
}

__global__ __launch_bounds__( RLE_THREADS ) void
k_enc_rle1( const EncBlock* __restrict__ blocks, const uint8_t* __restrict__ in, uint8_t* __restrict__ rle,
            EncMeta* __restrict__ meta )
{
    const EncBlock b = blocks[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    __shared__ uint32_t sFull[RLE_THREADS], sVal[RLE_THREADS], sSum[RLE_THREADS];
    __shared__ uint32_t sLast[RLE_THREADS];
    __shared__ uint8_t used[256];
    __shared__ uint32_t carryByte, carryOff, outAt;
    used[tid] = 0;
    if ( tid == 0 ) {
        carryByte = 256;   /* none */
        carryOff = 0;
        outAt = 0;
    }
    __syncthreads();
    const uint8_t* src = in + b.inOff;
    uint8_t* dst = rle + b.pos;
    for ( uint64_t base = 0; base < b.inSize; base += RLE_THREADS * RLE_BYTES ) {
        const uint64_t lo = base + (uint64_t)tid * RLE_BYTES;
        const uint32_t cnt = lo < b.inSize ? (uint32_t)std::min<uint64_t>( RLE_BYTES, b.inSize - lo ) : 0;
        uint8_t v[RLE_BYTES];
#pragma unroll
        for ( int k = 0; k < RLE_BYTES; ++k ) v[k] = k < (int)cnt ? src[lo + k] : 0;
        sLast[tid] = cnt > 0 ? v[cnt - 1] : 256;
        __syncthreads();
        const uint32_t prevByte = tid == 0 ? carryByte : sLast[tid - 1];
        /* leading bytes that continue the run of prevByte; offset of the last byte in a run that starts here */
        uint32_t head = 0;
        while ( head < cnt && v[head] == prevByte ) ++head;
        uint32_t tail = 0;
        while ( tail < cnt && v[cnt - 1 - tail] == v[cnt - 1] ) ++tail;
        const bool full = cnt == 0 || head == cnt;
        sFull[tid] = full ? 1 : 0;
        sVal[tid] = full ? cnt : tail - 1;
        if ( tid == 0 && full ) {
            sFull[0] = 0;
            sVal[0] = carryOff + cnt;
        }
        __syncthreads();
        scanRuns( sFull, sVal, tid );
        /* run offset of the byte in front of this thread's first */
        uint32_t off = tid == 0 ? carryOff : sVal[tid - 1];
        uint32_t prev = prevByte;
        uint32_t emit = 0;
        uint32_t offs[RLE_BYTES];
#pragma unroll
        for ( int k = 0; k < RLE_BYTES; ++k ) {
            if ( k < (int)cnt ) {
                off = v[k] == prev ? off + 1 : 0;
                prev = v[k];
                offs[k] = off % 255;
                emit += offs[k] < 3 ? 1 : ( offs[k] == 3 ? 2 : 0 );
            }
        }
        sSum[tid] = emit;
        __syncthreads();
        scanSum( sSum, tid );
        uint32_t at = outAt + sSum[tid] - emit;
#pragma unroll
        for ( int k = 0; k < RLE_BYTES; ++k ) {
            if ( k < (int)cnt && offs[k] <= 3 && at + ( offs[k] == 3 ? 1 : 0 ) < b.n ) {   /* (the plan's size bounds it) */
                dst[at++] = v[k];
                used[v[k]] = 1;
                if ( offs[k] == 3 ) {
                    /* the piece began 3 bytes back; it runs on while the byte repeats, 255 bytes at most */
                    const uint64_t pieceStart = lo + k - 3;
                    const uint64_t stop = std::min<uint64_t>( b.inSize, pieceStart + 255 );
                    uint64_t j = lo + k + 1;
                    while ( j < stop && src[j] == v[k] ) ++j;
                    const uint8_t count = (uint8_t)( j - pieceStart - 4 );
                    dst[at++] = count;
                    used[count] = 1;
                }
            }
        }
        __syncthreads();
        if ( tid == RLE_THREADS - 1 ) {
            outAt += sSum[RLE_THREADS - 1];
            /* the last thread with bytes holds the tile's last byte */
            const uint64_t lastIndex = std::min<uint64_t>( b.inSize, base + RLE_THREADS * RLE_BYTES ) - 1;
            carryByte = src[lastIndex];
            const uint32_t lastThread = (uint32_t)( ( lastIndex - base ) / RLE_BYTES );
            carryOff = sVal[lastThread];
        }
        __syncthreads();
    }
    const uint64_t ballot = __ballot( used[tid] != 0 );
    if ( tid % 32 == 0 ) meta[blockIdx.x].inUse[tid / 32] = (uint32_t)( ballot >> ( tid & 32 ) );
    if ( tid == 0 ) meta[blockIdx.x].rleCount = outAt;
}

/* ------------------------------------------------------------------------------------------------ BWT */

/** Initial sort keys: (block, first 4 bytes of the rotation). */
__global__ void
k_bwt_init( const EncBlock* __restrict__ blocks, uint32_t nBlocks, const uint8_t* __restrict__ rle, uint32_t N,
            uint64_t* __restrict__ keys, uint32_t* __restrict__ values )
{
    const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
    if ( p >= N ) return;
    const uint32_t bi = blockOf( blocks, nBlocks, p );
    const uint32_t pos = blocks[bi].pos, n = blocks[bi].n;
    uint32_t r = p - pos, k = 0;
    for ( int j = 0; j < 4; ++j ) {
        k = ( k << 8 ) | rle[pos + r];
        r = r + 1 == n ? 0 : r + 1;
    }
    keys[p] = ( (uint64_t)bi << 32 ) | k;
    values[p] = p;
}

/** After a sort of m items (slots `active[i]`, or i itself when active is null): the sorted positions go to their
 * slots, group heads are marked for the rank scan, and items still tied whose block is longer than the next h stay
 * active. */
__global__ void
k_bwt_heads( const EncBlock* __restrict__ blocks, uint32_t nBlocks, const uint32_t* __restrict__ active, uint32_t m,
             const uint64_t* __restrict__ keys, const uint32_t* __restrict__ sorted, uint32_t* __restrict__ sa,
             uint32_t* __restrict__ heads, uint8_t* __restrict__ flags, uint64_t nextH )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= m ) return;
    const uint32_t slot = active != nullptr ? active[i] : i;
    if ( active != nullptr ) sa[slot] = sorted[i];
    const uint64_t key = keys[i];
    const bool head = i == 0 || keys[i - 1] != key;
    const bool tied = !head || ( i + 1 < m && keys[i + 1] == key );
    heads[i] = head ? slot : 0;
    flags[i] = tied && nextH < blocks[blockOf( blocks, nBlocks, slot )].n ? 1 : 0;
}

__global__ void
k_bwt_rank( const uint32_t* __restrict__ sorted, const uint32_t* __restrict__ groupStart, uint32_t m,
            uint32_t* __restrict__ rank )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i < m ) rank[sorted[i]] = groupStart[i];
}

/** Keys of a doubling round: (rank, rank of the rotation h further on). */
__global__ void
k_bwt_keys( const EncBlock* __restrict__ blocks, uint32_t nBlocks, const uint32_t* __restrict__ active, uint32_t m,
            const uint32_t* __restrict__ sa, const uint32_t* __restrict__ rank, uint64_t h, uint32_t bits,
            uint64_t* __restrict__ keys, uint32_t* __restrict__ values )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= m ) return;
    const uint32_t p = sa[active[i]];
    const EncBlock& b = blocks[blockOf( blocks, nBlocks, p )];
    uint64_t r = p - b.pos + h;   /* h < n */
    if ( r >= b.n ) r -= b.n;
    keys[i] = ( (uint64_t)rank[p] << bits ) | rank[b.pos + r];
    values[i] = p;
}

__global__ void
k_iota( uint32_t* __restrict__ out, uint32_t m )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i < m ) out[i] = i;
}

__global__ void
k_bwt_finish( const EncBlock* __restrict__ blocks, uint32_t nBlocks, const uint8_t* __restrict__ rle,
              const uint32_t* __restrict__ sa, uint32_t N, uint8_t* __restrict__ L, EncMeta* __restrict__ meta )
{
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    if ( s >= N ) return;
    const uint32_t bi = blockOf( blocks, nBlocks, s );
    const uint32_t pos = blocks[bi].pos, n = blocks[bi].n;
    const uint32_t r = sa[s] - pos;
    L[s] = rle[pos + ( r == 0 ? n - 1 : r - 1 )];
    if ( r == 0 ) meta[bi].origPtr = s - pos;
}

/* ------------------------------------------------------------------------------------------------ MTF */

__global__ __launch_bounds__( 64 ) void
k_enc_mtf( const EncBlock* __restrict__ blocks, const uint8_t* __restrict__ L, EncMeta* __restrict__ meta,
           uint16_t* __restrict__ syms, uint32_t* __restrict__ freqs )
{
    const EncBlock b = blocks[blockIdx.x];
    const uint32_t lane = threadIdx.x;
    __shared__ uint8_t toSeq[256];
    __shared__ uint32_t freq[MAX_ALPHA];
    __shared__ uint32_t sInUse;
    for ( uint32_t i = lane; i < MAX_ALPHA; i += 64 ) freq[i] = 0;
    if ( lane == 0 ) {
        uint32_t k = 0;
        for ( uint32_t v = 0; v < 256; ++v ) {
            toSeq[v] = (uint8_t)k;
            if ( ( meta[blockIdx.x].inUse[v / 32] >> ( v % 32 ) ) & 1u ) ++k;
        }
        sInUse = k;
    }
    __syncthreads();
    const uint32_t nInUse = sInUse;
    /* list position 4 * lane + j is byte j of w */
    uint32_t w = 0;
    for ( uint32_t j = 0; j < 4; ++j ) {
        const uint32_t p = 4 * lane + j;
        w |= ( p < nInUse ? p : 0xFFu ) << ( 8 * j );
    }
    uint16_t* out = syms + b.sym;
    uint32_t wr = 0, zPend = 0;
    const auto emit = [&] ( uint32_t v ) {
        if ( lane == 0 && wr <= b.n ) {   /* symbolSlots: n + 1 */
            out[wr] = (uint16_t)v;
            freq[v] += 1;
        }
        ++wr;
    };
    const auto flushZeros = [&] () {
        if ( zPend == 0 ) return;
        zPend -= 1;
        for ( ;; ) {
            emit( zPend & 1 );   /* RUNB = 1, RUNA = 0 */
            if ( zPend < 2 ) break;
            zPend = ( zPend - 2 ) / 2;
        }
        zPend = 0;
    };
    for ( uint32_t base = 0; base < b.n; base += 64 ) {
        const uint32_t mine = base + lane < b.n ? toSeq[L[b.pos + base + lane]] : 0;
        const uint32_t cnt = std::min<uint32_t>( 64, b.n - base );
        for ( uint32_t t = 0; t < cnt; ++t ) {
            const uint32_t s = __shfl( mine, t );
            const uint32_t x = w ^ ( s * 0x01010101u );
            const uint32_t zero = ( x - 0x01010101u ) & ~x & 0x80808080u;
            const uint64_t ballot = __ballot( zero != 0 );
            const uint32_t owner = (uint32_t)__builtin_ctzll( ballot );
            const uint32_t byteIdx = __shfl( zero != 0 ? (uint32_t)__builtin_ctz( zero ) / 8 : 0u, owner );
            const uint32_t idx = 4 * owner + byteIdx;
            if ( idx == 0 ) {
                ++zPend;
                continue;
            }
            flushZeros();
            emit( idx + 1 );
            uint32_t top = __shfl_up( w, 1 ) >> 24;
            if ( lane == 0 ) top = s;
            const uint32_t shifted = ( w << 8 ) | top;
            uint32_t mask;
            if ( 4 * lane + 3 <= idx ) mask = 0xFFFFFFFFu;
            else if ( 4 * lane > idx ) mask = 0;
            else mask = ( 1u << ( 8 * ( idx - 4 * lane + 1 ) ) ) - 1;
            w = ( w & ~mask ) | ( shifted & mask );
        }
    }
    flushZeros();
    emit( nInUse + 1 );
    __syncthreads();
    uint32_t* f = freqs + (uint64_t)blockIdx.x * MAX_ALPHA;
    for ( uint32_t i = lane; i < MAX_ALPHA; i += 64 ) f[i] = freq[i];
    if ( lane == 0 ) {
        meta[blockIdx.x].nMTF = std::min( wr, b.n + 1 );
        meta[blockIdx.x].nInUse = nInUse;
    }
}

/* ------------------------------------------------------------------------------------------------ tables */

constexpr int TAB_THREADS = 256;

/** Huffman code lengths of `alpha` symbols (frequency 0 counts as 1), at most MAX_CODE_LENGTH: while a length exceeds
 * it, every weight w becomes 1 + w / 2 and the code is built again.  Ties go to the lower symbol. */
__device__ void
buildLengths( const uint32_t* freq, uint32_t alpha, uint8_t* len )
{
    uint32_t w[MAX_ALPHA];
    uint16_t order[MAX_ALPHA];
    uint32_t inner[MAX_ALPHA];
    uint16_t parent[2 * MAX_ALPHA];
    uint8_t depth[MAX_ALPHA];
    for ( uint32_t i = 0; i < alpha; ++i ) w[i] = freq[i] == 0 ? 1 : freq[i];
    for ( ;; ) {
        for ( uint32_t i = 0; i < alpha; ++i ) {   /* insertion sort by (weight, symbol) */
            uint32_t j = i;
            while ( j > 0 && w[order[j - 1]] > w[i] ) {
                order[j] = order[j - 1];
                --j;
            }
            order[j] = (uint16_t)i;
        }
        uint32_t li = 0, ii = 0, ni = 0;
        const auto pick = [&] () -> uint32_t {
            if ( li < alpha && ( ii >= ni || w[order[li]] <= inner[ii] ) ) return li++;
            return alpha + ii++;
        };
        const auto weight = [&] ( uint32_t node ) { return node < alpha ? w[order[node]] : inner[node - alpha]; };
        for ( uint32_t k = 0; k + 1 < alpha; ++k ) {
            const uint32_t a = pick(), c = pick();
            inner[ni] = weight( a ) + weight( c );
            parent[a] = parent[c] = (uint16_t)( alpha + ni );
            ++ni;
        }
        depth[ni - 1] = 0;
        for ( int j = (int)ni - 2; j >= 0; --j ) depth[j] = depth[parent[alpha + j] - alpha] + 1;
        uint32_t longest = 0;
        for ( uint32_t k = 0; k < alpha; ++k ) {
            const uint32_t l = depth[parent[k] - alpha] + 1u;
            len[order[k]] = (uint8_t)std::min<uint32_t>( l, 255 );
            longest = std::max( longest, l );
        }
        if ( longest <= MAX_CODE_LENGTH ) return;
        for ( uint32_t i = 0; i < alpha; ++i ) w[i] = 1 + w[i] / 2;
    }
}

__global__ __launch_bounds__( TAB_THREADS ) void
k_enc_tables( const EncBlock* __restrict__ blocks, EncMeta* __restrict__ meta, const uint16_t* __restrict__ syms,
              const uint32_t* __restrict__ freqs, uint8_t* __restrict__ selectors, uint8_t* __restrict__ selectorMtf,
              uint32_t* __restrict__ groupOffsets, EncTables* __restrict__ tables )
{
    const EncBlock b = blocks[blockIdx.x];
    EncMeta& me = meta[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    __shared__ uint8_t len[MAX_TABLES][MAX_ALPHA];
    __shared__ uint32_t rfreq[MAX_TABLES][MAX_ALPHA];
    __shared__ uint32_t sSum[TAB_THREADS];
    __shared__ uint32_t sHeader;
    const uint32_t nMTF = me.nMTF;
    const uint32_t alpha = me.nInUse + 2;
    const uint32_t nGroups = nMTF < 200 ? 2 : nMTF < 600 ? 3 : nMTF < 1200 ? 4 : nMTF < 2400 ? 5 : 6;
    const uint32_t nSel = ( nMTF + GROUP_SIZE - 1 ) / GROUP_SIZE;
    const uint16_t* s = syms + b.sym;
    const uint32_t* freq = freqs + (uint64_t)blockIdx.x * MAX_ALPHA;
    uint8_t* sel = selectors + b.sel;
    uint32_t* goff = groupOffsets + b.sel;

    if ( tid == 0 ) {
        /* initial tables: ranges of the alphabet of about equal frequency */
        uint32_t nPart = nGroups, remF = nMTF, gs = 0;
        while ( nPart > 0 ) {
            const uint32_t tFreq = remF / nPart;
            int ge = (int)gs - 1;
            uint32_t aFreq = 0;
            while ( aFreq < tFreq && ge < (int)alpha - 1 ) {
                ++ge;
                aFreq += freq[ge];
            }
            if ( ge > (int)gs && nPart != nGroups && nPart != 1 && ( ( nGroups - nPart ) % 2 == 1 ) ) {
                aFreq -= freq[ge];
                --ge;
            }
            for ( uint32_t v = 0; v < alpha; ++v ) len[nPart - 1][v] = ( (int)v >= (int)gs && (int)v <= ge ) ? 0 : 15;
            --nPart;
            gs = (uint32_t)( ge + 1 );
            remF -= aFreq;
        }
    }
    __syncthreads();
    for ( int iter = 0; iter <= 4; ++iter ) {
        const bool last = iter == 4;   /* selection against the final tables; no rebuild */
        for ( uint32_t i = tid; i < MAX_TABLES * MAX_ALPHA; i += TAB_THREADS ) ( &rfreq[0][0] )[i] = 0;
        __syncthreads();
        for ( uint32_t g = tid; g < nSel; g += TAB_THREADS ) {
            const uint32_t end = std::min( nMTF, ( g + 1 ) * GROUP_SIZE );
            uint32_t cost[MAX_TABLES] = { 0, 0, 0, 0, 0, 0 };
            for ( uint32_t i = g * GROUP_SIZE; i < end; ++i ) {
                const uint32_t v = s[i];
#pragma unroll
                for ( int t = 0; t < MAX_TABLES; ++t ) cost[t] += len[t][v];
            }
            uint32_t best = 0;
            for ( uint32_t t = 1; t < nGroups; ++t ) {
                if ( cost[t] < cost[best] ) best = t;
            }
            sel[g] = (uint8_t)best;
            if ( last ) {
                goff[g] = cost[best];
            } else {
                for ( uint32_t i = g * GROUP_SIZE; i < end; ++i ) atomicAdd( &rfreq[best][s[i]], 1u );
            }
        }
        __syncthreads();
        if ( last ) break;
        if ( tid < nGroups ) buildLengths( rfreq[tid], alpha, len[tid] );
        __syncthreads();
    }
    /* group bit offsets: exclusive scan of the group costs, each thread a contiguous range */
    const uint32_t per = ( nSel + TAB_THREADS - 1 ) / TAB_THREADS;
    const uint32_t g0 = std::min( nSel, tid * per ), g1 = std::min( nSel, g0 + per );
    uint32_t sum = 0;
    for ( uint32_t g = g0; g < g1; ++g ) sum += goff[g];
    sSum[tid] = sum;
    __syncthreads();
    for ( uint32_t d = 1; d < TAB_THREADS; d <<= 1 ) {
        const uint32_t v = sSum[tid] + ( tid >= d ? sSum[tid - d] : 0 );
        __syncthreads();
        sSum[tid] = v;
        __syncthreads();
    }
    uint32_t at = sSum[tid] - sum;
    for ( uint32_t g = g0; g < g1; ++g ) {
        const uint32_t c = goff[g];
        goff[g] = at;
        at += c;
    }
    if ( tid < nGroups ) {
        /* canonical codes: by length, then by symbol */
        EncTables& tab = tables[blockIdx.x];
        uint32_t code = 0;
        for ( uint32_t l = 1; l <= MAX_CODE_LENGTH; ++l ) {
            for ( uint32_t v = 0; v < alpha; ++v ) {
                if ( len[tid][v] == l ) tab.code[tid][v] = code++;
            }
            code <<= 1;
        }
        for ( uint32_t v = 0; v < alpha; ++v ) tab.len[tid][v] = len[tid][v];
    }
    if ( tid == 0 ) {
        uint32_t bits = 48 + 32 + 1 + 24 + 16 + 3 + 15;
        for ( uint32_t i = 0; i < 16; ++i ) {
            if ( ( me.inUse[i / 2] >> ( 16 * ( i % 2 ) ) ) & 0xFFFFu ) bits += 16;
        }
        uint8_t list[MAX_TABLES] = { 0, 1, 2, 3, 4, 5 };
        uint8_t* mtf = selectorMtf + b.sel;
        for ( uint32_t g = 0; g < nSel; ++g ) {
            const uint8_t v = sel[g];
            uint32_t j = 0;
            while ( list[j] != v ) ++j;
            for ( uint32_t k = j; k > 0; --k ) list[k] = list[k - 1];
            list[0] = v;
            mtf[g] = (uint8_t)j;
            bits += j + 1;
        }
        for ( uint32_t t = 0; t < nGroups; ++t ) {
            int curr = len[t][0];
            bits += 5;
            for ( uint32_t v = 0; v < alpha; ++v ) {
                const int d = (int)len[t][v] - curr;
                bits += 2 * (uint32_t)( d < 0 ? -d : d ) + 1;
                curr = len[t][v];
            }
        }
        sHeader = bits;
        me.nGroups = nGroups;
        me.nSel = nSel;
        me.headerBits = bits;
    }
    __syncthreads();
    if ( tid == TAB_THREADS - 1 ) me.dataBits = sSum[TAB_THREADS - 1];
    (void)sHeader;
}

/* ------------------------------------------------------------------------------------------------ emit */

__global__ __launch_bounds__( TAB_THREADS ) void
k_enc_emit( const EncBlock* __restrict__ blocks, EncMeta* __restrict__ meta, const uint64_t* __restrict__ bitPos,
            const uint16_t* __restrict__ syms, const uint8_t* __restrict__ selectors,
            const uint8_t* __restrict__ selectorMtf, const uint32_t* __restrict__ groupOffsets,
            const EncTables* __restrict__ tables, uint32_t* __restrict__ out )
{
    const EncBlock b = blocks[blockIdx.x];
    EncMeta& me = meta[blockIdx.x];
    const EncTables& tab = tables[blockIdx.x];
    const uint32_t tid = threadIdx.x;
    const uint64_t start = bitPos[blockIdx.x];
    const uint32_t nMTF = me.nMTF, nSel = me.nSel, nGroups = me.nGroups, alpha = me.nInUse + 2;
    const uint64_t dataStart = start + me.headerBits;
    if ( tid == 0 ) {
        BitWriter bw( out, start );
        bw.put( 0x314159, 24 );
        bw.put( 0x265359, 24 );
        bw.put( b.crc, 32 );
        bw.put( 0, 1 );
        bw.put( me.origPtr, 24 );
        uint32_t ranges = 0;
        for ( uint32_t i = 0; i < 16; ++i ) {
            if ( ( me.inUse[i / 2] >> ( 16 * ( i % 2 ) ) ) & 0xFFFFu ) ranges |= 1u << ( 15 - i );
        }
        bw.put( ranges, 16 );
        for ( uint32_t i = 0; i < 16; ++i ) {
            const uint32_t bitsLow = ( me.inUse[i / 2] >> ( 16 * ( i % 2 ) ) ) & 0xFFFFu;   /* bit j = value 16 i + j */
            if ( bitsLow == 0 ) continue;
            uint32_t v = 0;
            for ( uint32_t j = 0; j < 16; ++j ) v |= ( ( bitsLow >> j ) & 1u ) << ( 15 - j );
            bw.put( v, 16 );
        }
        bw.put( nGroups, 3 );
        bw.put( nSel, 15 );
        const uint8_t* mtf = selectorMtf + b.sel;
        for ( uint32_t g = 0; g < nSel; ++g ) {
            const uint32_t j = mtf[g];
            bw.put( ( ( 1u << j ) - 1 ) << 1, j + 1 );
        }
        for ( uint32_t t = 0; t < nGroups; ++t ) {
            uint32_t curr = tab.len[t][0];
            bw.put( curr, 5 );
            for ( uint32_t v = 0; v < alpha; ++v ) {
                const uint32_t l = tab.len[t][v];
                while ( curr < l ) { bw.put( 2, 2 ); ++curr; }
                while ( curr > l ) { bw.put( 3, 2 ); --curr; }
                bw.put( 0, 1 );
            }
        }
        bw.finish();
        me.emitted = (uint32_t)bw.written;
    }
    const uint16_t* s = syms + b.sym;
    const uint8_t* sel = selectors + b.sel;
    const uint32_t* goff = groupOffsets + b.sel;
    for ( uint32_t g = tid; g < nSel; g += TAB_THREADS ) {
        BitWriter bw( out, dataStart + goff[g] );
        const uint32_t t = sel[g];
        const uint32_t end = std::min( nMTF, ( g + 1 ) * GROUP_SIZE );
        for ( uint32_t i = g * GROUP_SIZE; i < end; ++i ) bw.put( tab.code[t][s[i]], tab.len[t][s[i]] );
        bw.finish();
    }
}

__global__ void
k_enc_frame( const FrameJob* __restrict__ jobs, uint32_t n, uint32_t* __restrict__ out )
{
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if ( i >= n ) return;
    const FrameJob j = jobs[i];
    BitWriter bw( out, j.bit );
    if ( j.kind == 0 ) {
        bw.put( 0x425A68, 24 );   /* "BZh" */
        bw.put( '0' + j.value, 8 );
    } else {
        bw.put( 0x177245, 24 );
        bw.put( 0x385090, 24 );
        bw.put( j.value, 32 );
    }
    bw.finish();
}

/* ------------------------------------------------------------------------------------------------ host */

struct DeviceBuffer
{
    void* p{ nullptr };
    uint64_t cap{ 0 };
};

enum EncBuffer   /* the encoder's device buffers, each grown on its own (ensure) */
{
    B_IN, B_RLE, B_L, B_SA, B_RANK, B_KA, B_KB, B_VA, B_VB, B_ACT0, B_ACT1, B_HEADS, B_FLAGS, B_SYMS, B_SEL, B_SELMTF, B_GOFF,
    B_BLOCKS, B_META, B_FREQS, B_TABLES, B_BITPOS, B_JOBS, B_COUNT, B_TEMP, ENC_BUFFERS
};

struct Encoder
{
    int device{ 0 };
    DeviceBuffer buffer[ENC_BUFFERS];
    std::vector<uint64_t> mapBits, mapBytes, mapFirst, mapCount;
    std::vector<uint8_t> staging;

    uint64_t
    bytes() const
    {
        uint64_t total = 0;
        for ( const DeviceBuffer& b : buffer ) total += b.cap;
        return total;
    }

    ~Encoder()
    {
        (void)hipSetDevice( device );
        for ( DeviceBuffer& b : buffer ) (void)hipFree( b.p );
    }
};

void
releaseEncoder( void* e )
{
    delete static_cast<Encoder*>( e );
}

struct Failure
{
    int status;
    std::string message;
};

#define ENC_TRY( expr )                                                                                  \
    do {                                                                                                 \
        const hipError_t err_ = ( expr );                                                                \
        if ( err_ != hipSuccess ) throw Failure{ MI355X_BZ2_ERR_DEVICE, std::string( #expr ) + ": " + hipGetErrorString( err_ ) }; \
    } while ( 0 )

template<typename T>
T*
ensure( DeviceBuffer& b, uint64_t count )
{
    const uint64_t need = std::max<uint64_t>( count * sizeof( T ), 256 );
    if ( need > b.cap ) {
        /* nothing of the previous launch reads it: the caller has synchronised the stream */
        const uint64_t cap = std::max( need, b.cap + b.cap / 2 );
        (void)hipFree( b.p );
        b.p = nullptr;
        b.cap = 0;
        ENC_TRY( hipMalloc( &b.p, cap ) );
        b.cap = cap;
    }
    return static_cast<T*>( b.p );
}

uint32_t
bitsFor( uint64_t n )
{
    uint32_t bits = 1;
    while ( ( uint64_t( 1 ) << bits ) < n ) ++bits;
    return bits;
}

dim3
gridFor( uint64_t n, uint32_t threads )
{
    return dim3( (uint32_t)std::max<uint64_t>( 1, ( n + threads - 1 ) / threads ) );
}

/** Where a buffer's stream stands while its blocks are placed. */
struct StreamState
{
    uint64_t outOffset{ 0 };   /* bytes */
    uint64_t bits{ 32 };       /* behind "BZh<level>" */
    uint64_t decoded{ 0 };
    uint32_t crc{ 0 };
    uint32_t blocksPlaced{ 0 };
};

void
runCall( mi355x_bz2_ctx* ctx, Encoder& e, const uint8_t* const* buffers, const uint64_t* sizes, uint32_t n, int level,
         uint32_t maxLaunchBlocks, mi355x_bz2_compress_result* results, uint64_t* totalCompressed )
{
    const hipStream_t stream = static_cast<hipStream_t>( mi355x_bz2_stream( ctx ) );
    /* block cuts: one linear pass per buffer, buffers spread over up to PLAN_THREADS threads */
    std::vector<std::vector<Block>> perBuffer( n );
    {
        uint64_t totalBytes = 0;
        for ( uint32_t i = 0; i < n; ++i ) totalBytes += sizes[i];
        const uint32_t threads = totalBytes < PLAN_THREAD_BYTES
                                     ? 1u
                                     : std::min<uint32_t>( { PLAN_THREADS, n, std::max( 1u, std::thread::hardware_concurrency() ) } );
        std::atomic<uint32_t> next{ 0 };
        const auto work = [&] () {
            for ( uint32_t i = next++; i < n; i = next++ ) planBlocks( buffers[i], sizes[i], level, perBuffer[i] );
        };
        std::vector<std::thread> pool;
        for ( uint32_t t = 1; t < threads; ++t ) pool.emplace_back( work );
        work();
        for ( auto& t : pool ) t.join();
    }
    std::vector<Block> blocks;
    std::vector<uint32_t> blockBuffer, firstBlock( n + 1, 0 );
    for ( uint32_t i = 0; i < n; ++i ) {
        firstBlock[i] = (uint32_t)blocks.size();
        blocks.insert( blocks.end(), perBuffer[i].begin(), perBuffer[i].end() );
        blockBuffer.resize( blocks.size(), i );
    }
    firstBlock[n] = (uint32_t)blocks.size();
    const auto launches = planLaunches( blocks, maxLaunchBlocks, 0 );

    e.mapFirst.assign( n, 0 );
    e.mapCount.assign( n, 0 );
    uint64_t entries = 0;
    for ( uint32_t i = 0; i < n; ++i ) {
        e.mapFirst[i] = entries;
        e.mapCount[i] = mapEntries( firstBlock[i + 1] - firstBlock[i] );
        entries += e.mapCount[i];
    }
    e.mapBits.assign( entries, 0 );
    e.mapBytes.assign( entries, 0 );

    std::vector<StreamState> streams( n );
    std::vector<FrameJob> frames;
    uint32_t nextBuffer = 0;      /* buffers before it have their output offset */
    uint64_t outEnd = 0;          /* bytes: end of the last finished buffer's stream */
    uint64_t zeroedUpTo = 0;      /* bytes of the result buffer that are zero or written */
    uint8_t* dResult = nullptr;

    const auto finishStream = [&] ( uint32_t i ) {
        StreamState& st = streams[i];
        const uint32_t nb = firstBlock[i + 1] - firstBlock[i];
        const uint64_t eos = 8 * st.outOffset + st.bits;
        frames.push_back( { 8 * st.outOffset, 0u, (uint32_t)level } );
        frames.push_back( { eos, 1u, st.crc } );
        const uint64_t size = streamBytes( st.bits + 80 );
        const uint64_t m = e.mapFirst[i];
        if ( nb == 0 ) {
            e.mapBits[m] = 0;
            e.mapBytes[m] = 0;
        } else {
            e.mapBits[m + nb] = eos - 8 * st.outOffset;
            e.mapBytes[m + nb] = st.decoded;
            e.mapBits[m + nb + 1] = 8 * size;
            e.mapBytes[m + nb + 1] = st.decoded;
        }
        results[i].output_offset = st.outOffset;
        results[i].compressed_size = size;
        results[i].n_blocks = nb;
        results[i].map_first = e.mapFirst[i];
        results[i].map_entries = (uint32_t)e.mapCount[i];
        results[i].status = MI355X_BZ2_OK;
        outEnd = st.outOffset + size;
    };
    /* buffers up to `upTo` (exclusive) that have no blocks left to place are finished in order */
    const auto advance = [&] ( uint32_t upTo ) {
        while ( nextBuffer < upTo ) {
            streams[nextBuffer].outOffset = outEnd;
            const uint32_t nb = firstBlock[nextBuffer + 1] - firstBlock[nextBuffer];
            if ( nb != 0 ) break;
            finishStream( nextBuffer );
            ++nextBuffer;
        }
    };
    const auto zeroTo = [&] ( uint64_t end ) {
        end = ( end + 3 ) / 4 * 4 + 8;
        if ( end <= zeroedUpTo && dResult != nullptr ) return;
        const int rc = mi355x::resultBuffer( ctx, end, zeroedUpTo, &dResult );
        if ( rc != MI355X_BZ2_OK ) throw Failure{ rc, "the result buffer could not grow" };
        if ( end > zeroedUpTo ) ENC_TRY( hipMemsetAsync( dResult + zeroedUpTo, 0, end - zeroedUpTo, stream ) );
        zeroedUpTo = std::max( zeroedUpTo, end );
    };

    std::vector<EncBlock> hb;
    std::vector<uint64_t> pieceSizes;
    std::vector<uint32_t> crcs;
    std::vector<EncMeta> hm;
    std::vector<uint64_t> hBitPos;
    for ( const Launch& launch : launches ) {
        /* input: the launch's blocks back to back */
        e.staging.resize( launch.inputBytes );
        hb.resize( launch.count );
        pieceSizes.resize( launch.count );
        uint64_t at = 0, sym = 0, selector = 0;
        uint32_t pos = 0;
        for ( uint32_t k = 0; k < launch.count; ++k ) {
            const Block& b = blocks[launch.first + k];
            std::memcpy( e.staging.data() + at, buffers[blockBuffer[launch.first + k]] + b.start, b.size );
            hb[k] = { at, (uint32_t)b.size, pos, b.rle, (uint32_t)sym, (uint32_t)selector, 0 };
            pieceSizes[k] = b.size;
            at += b.size;
            pos += b.rle;
            sym += symbolSlots( b.rle );
            selector += selectorSlots( b.rle );
        }
        const uint32_t N = pos, nb = launch.count;
        uint8_t* dIn = ensure<uint8_t>( e.buffer[B_IN], launch.inputBytes + 64 );
        ENC_TRY( hipMemcpyAsync( dIn, e.staging.data(), launch.inputBytes, hipMemcpyHostToDevice, stream ) );
        ENC_TRY( hipStreamSynchronize( stream ) );
        crcs.resize( nb );
        int rc = mi355x_bz2_crc32_device( ctx, dIn, pieceSizes.data(), nb, crcs.data() );
        if ( rc != MI355X_BZ2_OK ) throw Failure{ rc, "block CRCs failed" };
        for ( uint32_t k = 0; k < nb; ++k ) hb[k].crc = crcs[k];

        EncBlock* dBlocks = ensure<EncBlock>( e.buffer[B_BLOCKS], nb );
        EncMeta* dMeta = ensure<EncMeta>( e.buffer[B_META], nb );
        uint8_t* dRle = ensure<uint8_t>( e.buffer[B_RLE], N );
        uint8_t* dL = ensure<uint8_t>( e.buffer[B_L], N );
        uint32_t* dSa = ensure<uint32_t>( e.buffer[B_SA], N );
        uint32_t* dRank = ensure<uint32_t>( e.buffer[B_RANK], N );
        uint64_t* dKA = ensure<uint64_t>( e.buffer[B_KA], N );
        uint64_t* dKB = ensure<uint64_t>( e.buffer[B_KB], N );
        uint32_t* dVA = ensure<uint32_t>( e.buffer[B_VA], N );
        uint32_t* dVB = ensure<uint32_t>( e.buffer[B_VB], N );
        uint32_t* dAct[2] = { ensure<uint32_t>( e.buffer[B_ACT0], N ), ensure<uint32_t>( e.buffer[B_ACT1], N ) };
        uint32_t* dHeads = ensure<uint32_t>( e.buffer[B_HEADS], N );
        uint8_t* dFlags = ensure<uint8_t>( e.buffer[B_FLAGS], N );
        uint16_t* dSyms = ensure<uint16_t>( e.buffer[B_SYMS], sym );
        uint8_t* dSel = ensure<uint8_t>( e.buffer[B_SEL], selector );
        uint8_t* dSelMtf = ensure<uint8_t>( e.buffer[B_SELMTF], selector );
        uint32_t* dGoff = ensure<uint32_t>( e.buffer[B_GOFF], selector );
        uint32_t* dFreqs = ensure<uint32_t>( e.buffer[B_FREQS], (uint64_t)nb * MAX_ALPHA );
        EncTables* dTables = ensure<EncTables>( e.buffer[B_TABLES], nb );
        uint64_t* dBitPos = ensure<uint64_t>( e.buffer[B_BITPOS], nb );
        uint32_t* dCount = ensure<uint32_t>( e.buffer[B_COUNT], 1 );
        size_t sortBytes = 0, scanBytes = 0, selectBytes = 0;
        ENC_TRY( rocprim::radix_sort_pairs( nullptr, sortBytes, dKA, dKB, dVA, dVB, N, 0, 64, stream ) );
        ENC_TRY( rocprim::inclusive_scan( nullptr, scanBytes, dHeads, dHeads, N, rocprim::maximum<uint32_t>(), stream ) );
        ENC_TRY( rocprim::select( nullptr, selectBytes, dAct[0], dFlags, dAct[1], dCount, N, stream ) );
        size_t tempBytes = std::max( { sortBytes, scanBytes, selectBytes } );
        void* dTemp = ensure<uint8_t>( e.buffer[B_TEMP], tempBytes );
        tempBytes = e.buffer[B_TEMP].cap;

        ENC_TRY( hipMemcpyAsync( dBlocks, hb.data(), nb * sizeof( EncBlock ), hipMemcpyHostToDevice, stream ) );
        ENC_TRY( hipMemsetAsync( dMeta, 0, nb * sizeof( EncMeta ), stream ) );
        hipLaunchKernelGGL( k_enc_rle1, dim3( nb ), dim3( RLE_THREADS ), 0, stream, dBlocks, dIn, dRle, dMeta );
        ENC_TRY( hipGetLastError() );

        /* BWT: initial sort by (block, 4 bytes), then doubling rounds over the slots still tied */
        hipLaunchKernelGGL( k_bwt_init, gridFor( N, 256 ), dim3( 256 ), 0, stream, dBlocks, nb, dRle, N, dKA, dVA );
        ENC_TRY( hipGetLastError() );
        ENC_TRY( rocprim::radix_sort_pairs( dTemp, tempBytes, dKA, dKB, dVA, dSa, N, 0, 32 + bitsFor( nb ), stream ) );
        hipLaunchKernelGGL( k_bwt_heads, gridFor( N, 256 ), dim3( 256 ), 0, stream, dBlocks, nb,
                            static_cast<const uint32_t*>( nullptr ), N, dKB, static_cast<const uint32_t*>( nullptr ), dSa,
                            dHeads, dFlags, uint64_t( 4 ) );
        ENC_TRY( hipGetLastError() );
        ENC_TRY( rocprim::inclusive_scan( dTemp, tempBytes, dHeads, dVB, N, rocprim::maximum<uint32_t>(), stream ) );
        hipLaunchKernelGGL( k_bwt_rank, gridFor( N, 256 ), dim3( 256 ), 0, stream, dSa, dVB, N, dRank );
        ENC_TRY( hipGetLastError() );
        hipLaunchKernelGGL( k_iota, gridFor( N, 256 ), dim3( 256 ), 0, stream, dAct[1], N );
        ENC_TRY( rocprim::select( dTemp, tempBytes, dAct[1], dFlags, dAct[0], dCount, N, stream ) );
        const uint32_t bits = bitsFor( N );
        int cur = 0;
        for ( uint64_t h = 4;; h *= 2 ) {
            uint32_t m = 0;
            ENC_TRY( hipMemcpyAsync( &m, dCount, sizeof( m ), hipMemcpyDeviceToHost, stream ) );
            ENC_TRY( hipStreamSynchronize( stream ) );
            if ( m == 0 ) break;
            const uint32_t* act = dAct[cur];
            hipLaunchKernelGGL( k_bwt_keys, gridFor( m, 256 ), dim3( 256 ), 0, stream, dBlocks, nb, act, m, dSa, dRank, h,
                                bits, dKA, dVA );
            ENC_TRY( hipGetLastError() );
            ENC_TRY( rocprim::radix_sort_pairs( dTemp, tempBytes, dKA, dKB, dVA, dVB, m, 0, 2 * bits, stream ) );
            hipLaunchKernelGGL( k_bwt_heads, gridFor( m, 256 ), dim3( 256 ), 0, stream, dBlocks, nb, act, m, dKB, dVB,
                                dSa, dHeads, dFlags, 2 * h );
            ENC_TRY( hipGetLastError() );
            /* (the scan's output may not overlap its input: dKA is free now) */
            uint32_t* groupStart = reinterpret_cast<uint32_t*>( dKA );
            ENC_TRY( rocprim::inclusive_scan( dTemp, tempBytes, dHeads, groupStart, m, rocprim::maximum<uint32_t>(), stream ) );
            hipLaunchKernelGGL( k_bwt_rank, gridFor( m, 256 ), dim3( 256 ), 0, stream, dVB, groupStart, m, dRank );
            ENC_TRY( hipGetLastError() );
            ENC_TRY( rocprim::select( dTemp, tempBytes, act, dFlags, dAct[1 - cur], dCount, m, stream ) );
            cur = 1 - cur;
        }
        hipLaunchKernelGGL( k_bwt_finish, gridFor( N, 256 ), dim3( 256 ), 0, stream, dBlocks, nb, dRle, dSa, N, dL, dMeta );
        ENC_TRY( hipGetLastError() );
        hipLaunchKernelGGL( k_enc_mtf, dim3( nb ), dim3( 64 ), 0, stream, dBlocks, dL, dMeta, dSyms, dFreqs );
        ENC_TRY( hipGetLastError() );
        hipLaunchKernelGGL( k_enc_tables, dim3( nb ), dim3( TAB_THREADS ), 0, stream, dBlocks, dMeta, dSyms, dFreqs, dSel,
                            dSelMtf, dGoff, dTables );
        ENC_TRY( hipGetLastError() );
        hm.resize( nb );
        ENC_TRY( hipMemcpyAsync( hm.data(), dMeta, nb * sizeof( EncMeta ), hipMemcpyDeviceToHost, stream ) );
        ENC_TRY( hipStreamSynchronize( stream ) );

        /* every block's place in its stream */
        hBitPos.resize( nb );
        uint64_t lastEnd = 0;
        for ( uint32_t k = 0; k < nb; ++k ) {
            const uint32_t gb = launch.first + k;
            const uint32_t i = blockBuffer[gb];
            if ( hm[k].rleCount != hb[k].n ) {
                throw Failure{ MI355X_BZ2_ERR_LOGIC, "block " + std::to_string( gb ) + ": RLE1 wrote "
                                                         + std::to_string( hm[k].rleCount ) + " bytes, the plan says "
                                                         + std::to_string( hb[k].n ) };
            }
            advance( i + 1 );
            StreamState& st = streams[i];
            const uint64_t m = e.mapFirst[i] + st.blocksPlaced;
            e.mapBits[m] = st.bits;
            e.mapBytes[m] = st.decoded;
            hBitPos[k] = 8 * st.outOffset + st.bits;
            st.bits += (uint64_t)hm[k].headerBits + hm[k].dataBits;
            st.decoded += blocks[gb].size;
            st.crc = combineCrc( st.crc, hb[k].crc );
            st.blocksPlaced += 1;
            lastEnd = 8 * st.outOffset + st.bits;
            if ( gb + 1 == firstBlock[i + 1] ) {
                finishStream( i );
                nextBuffer = i + 1;
            }
        }
        zeroTo( ( lastEnd + 7 ) / 8 );
        ENC_TRY( hipMemcpyAsync( dBitPos, hBitPos.data(), nb * sizeof( uint64_t ), hipMemcpyHostToDevice, stream ) );
        hipLaunchKernelGGL( k_enc_emit, dim3( nb ), dim3( TAB_THREADS ), 0, stream, dBlocks, dMeta, dBitPos, dSyms, dSel,
                            dSelMtf, dGoff, dTables, reinterpret_cast<uint32_t*>( dResult ) );
        ENC_TRY( hipGetLastError() );
        ENC_TRY( hipMemcpyAsync( hm.data(), dMeta, nb * sizeof( EncMeta ), hipMemcpyDeviceToHost, stream ) );
        ENC_TRY( hipStreamSynchronize( stream ) );
        for ( uint32_t k = 0; k < nb; ++k ) {
            if ( hm[k].emitted != hm[k].headerBits ) {
                throw Failure{ MI355X_BZ2_ERR_LOGIC, "block " + std::to_string( launch.first + k ) + ": header of "
                                                         + std::to_string( hm[k].emitted ) + " bits, planned "
                                                         + std::to_string( hm[k].headerBits ) };
            }
        }
    }
    advance( n );
    zeroTo( outEnd );
    if ( !frames.empty() ) {
        FrameJob* dJobs = ensure<FrameJob>( e.buffer[B_JOBS], frames.size() );
        ENC_TRY( hipMemcpyAsync( dJobs, frames.data(), frames.size() * sizeof( FrameJob ), hipMemcpyHostToDevice, stream ) );
        hipLaunchKernelGGL( k_enc_frame, gridFor( frames.size(), 64 ), dim3( 64 ), 0, stream, dJobs,
                            (uint32_t)frames.size(), reinterpret_cast<uint32_t*>( dResult ) );
        ENC_TRY( hipGetLastError() );
    }
    ENC_TRY( hipStreamSynchronize( stream ) );
    const int rc = mi355x::publishResult( ctx, outEnd );
    if ( rc != MI355X_BZ2_OK ) throw Failure{ rc, "publishing the result failed" };
    if ( totalCompressed != nullptr ) *totalCompressed = outEnd;
}
}  // namespace

extern "C" {

int
mi355x_bz2_plan_compress_blocks( const uint8_t* data, uint64_t size, int level, uint64_t* blockSizes, uint64_t capacity,
                                 uint64_t* count )
{
    if ( ( size > 0 && data == nullptr ) || level < 1 || level > 9 || count == nullptr
         || ( capacity > 0 && blockSizes == nullptr ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    std::vector<Block> blocks;
    planBlocks( data, size, level, blocks );
    *count = blocks.size();
    for ( uint64_t i = 0; i < blocks.size() && i < capacity; ++i ) blockSizes[i] = blocks[i].size;
    return MI355X_BZ2_OK;
}

int
mi355x_bz2_compress_buffers( mi355x_bz2_ctx* ctx, const uint8_t* const* buffers, const uint64_t* sizes, uint32_t n,
                             int level, uint32_t maxLaunchBlocks, mi355x_bz2_compress_result* results,
                             uint64_t* totalCompressed )
{
    if ( ctx == nullptr || ( n > 0 && ( buffers == nullptr || sizes == nullptr || results == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    if ( level < 1 || level > 9 ) {
        mi355x::setLastError( ctx, "compress_buffers: the level must be 1 to 9" );
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    for ( uint32_t i = 0; i < n; ++i ) {
        if ( buffers[i] == nullptr && sizes[i] > 0 ) {
            mi355x::setLastError( ctx, "compress_buffers: buffer " + std::to_string( i ) + " is NULL" );
            return MI355X_BZ2_ERR_INVALID_ARGUMENT;
        }
    }
    if ( totalCompressed != nullptr ) *totalCompressed = 0;
    void*& slot = mi355x::encoderOf( ctx, releaseEncoder );
    try {
        if ( hipSetDevice( mi355x::deviceOf( ctx ) ) != hipSuccess ) {
            throw Failure{ MI355X_BZ2_ERR_DEVICE, "hipSetDevice failed" };
        }
        if ( slot == nullptr ) {
            auto* e = new Encoder();
            e->device = mi355x::deviceOf( ctx );
            slot = e;
        }
        for ( uint32_t i = 0; i < n; ++i ) results[i] = mi355x_bz2_compress_result{};
        runCall( ctx, *static_cast<Encoder*>( slot ), buffers, sizes, n, level, maxLaunchBlocks, results, totalCompressed );
    } catch ( const Failure& f ) {
        mi355x::setLastError( ctx, "compress_buffers: " + f.message );
        return f.status;
    } catch ( const std::bad_alloc& ) {
        mi355x::setLastError( ctx, "compress_buffers: out of host memory" );
        return MI355X_BZ2_ERR_OUTPUT_CAPACITY;
    }
    return MI355X_BZ2_OK;
}

int
mi355x_bz2_compress_block_map( mi355x_bz2_ctx* ctx, uint32_t buffer, uint64_t* bitOffsets, uint64_t* byteOffsets,
                               uint64_t capacity, uint64_t* count )
{
    if ( ctx == nullptr || count == nullptr || ( capacity > 0 && ( bitOffsets == nullptr || byteOffsets == nullptr ) ) ) {
        return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    }
    const void* slot = mi355x::encoderOf( ctx, releaseEncoder );
    const auto* e = static_cast<const Encoder*>( slot );
    if ( e == nullptr || buffer >= e->mapFirst.size() ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    const uint64_t first = e->mapFirst[buffer];
    *count = e->mapCount[buffer];
    for ( uint64_t i = 0; i < *count && i < capacity; ++i ) {
        bitOffsets[i] = e->mapBits[first + i];
        byteOffsets[i] = e->mapBytes[first + i];
    }
    return MI355X_BZ2_OK;
}

int
mi355x_bz2_encoder_memory( mi355x_bz2_ctx* ctx, uint64_t* bytes )
{
    if ( ctx == nullptr || bytes == nullptr ) return MI355X_BZ2_ERR_INVALID_ARGUMENT;
    const void* slot = mi355x::encoderOf( ctx, releaseEncoder );
    *bytes = slot != nullptr ? static_cast<const Encoder*>( slot )->bytes() : 0;
    return MI355X_BZ2_OK;
}

}  // extern "C"
