/**
 * bz2_compress.hpp -- plan of mi355x_bz2_compress_buffers: many buffers compressed in shared GPU launches.
 *
 * Host only, no HIP: bz2_compress.hip runs the plan, tests/native/compress_cases.cpp checks it under ASan/UBSan.
 *   planBlocks    where libbz2 cuts a buffer into blocks.  RLE1 splits the input into pieces (runs of one byte value, cut
 *                 every 255 bytes; a piece of L < 4 bytes takes L bytes of RLE1 output, one of L >= 4 takes 5).  A block
 *                 is a sequence of whole pieces and ends with the first piece that brings its RLE1 size to at least
 *                 100000 * level - 19; the last block takes what remains.  Because a block starts at a piece boundary,
 *                 RLE1 of the block's bytes alone gives the same pieces as RLE1 of the whole buffer.
 *   planLaunches  the blocks of all buffers, in order, cut into launches of at most maxLaunchBlocks blocks and a device
 *                 memory budget; each launch's blocks are laid out back to back (RLE1 positions, symbol slots,
 *                 selectors)
 *   MapLayout     where each buffer's entries start in the block map of the call
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

namespace mi355x::compress
{
constexpr uint32_t DEFAULT_LAUNCH_BLOCKS = 512;
constexpr uint64_t DEFAULT_LAUNCH_BYTES = uint64_t( 12 ) << 30;   /* device scratch budget of one launch */
/* device bytes per RLE1 position: sort keys (2 x 8) and values (2 x 4), rank, active slots (2 x 4), scan, head flags,
 * RLE1 bytes, L column, MTF output (2) */
constexpr uint64_t BYTES_PER_POSITION = 16 + 8 + 4 + 8 + 4 + 1 + 1 + 1 + 2;
constexpr uint32_t GROUP_SIZE = 50;   /* symbols per selector */

/** libbz2's block fill limit (nblockMAX) for a level 1..9. */
inline uint64_t
blockLimit( int level )
{
    return 100000 * (uint64_t)level - 19;
}

struct Block
{
    uint64_t start{ 0 }, size{ 0 };   /* input bytes [start, start + size) of the buffer */
    uint32_t rle{ 0 };                /* RLE1 bytes of the block */
};

/** The blocks of one buffer, appended to `out`. */
inline void
planBlocks( const uint8_t* data, uint64_t size, int level, std::vector<Block>& out )
{
    const uint64_t limit = blockLimit( level );
    uint64_t i = 0, start = 0, rle = 0;
    while ( i < size ) {
        const uint8_t c = data[i];
        uint64_t j = i + 1;
        const uint64_t stop = std::min<uint64_t>( size, i + 255 );
        while ( j < stop && data[j] == c ) ++j;
        const uint64_t piece = j - i;
        rle += piece < 4 ? piece : 5;
        i = j;
        if ( rle >= limit ) {
            out.push_back( { start, i - start, (uint32_t)rle } );
            start = i;
            rle = 0;
        }
    }
    if ( i > start ) out.push_back( { start, i - start, (uint32_t)rle } );
}

/** Symbol slots of a block: nMTF <= RLE1 size + 1 (a zero run of length z takes at most z RUNA/RUNB symbols, plus EOB). */
inline uint64_t
symbolSlots( uint32_t rle )
{
    return (uint64_t)rle + 1;
}

/** Selector slots of a block: one per 50 symbols. */
inline uint64_t
selectorSlots( uint32_t rle )
{
    return ( symbolSlots( rle ) + GROUP_SIZE - 1 ) / GROUP_SIZE;
}

/** Device bytes one block needs in a launch: its positions plus its input span. */
inline uint64_t
blockBytes( const Block& b )
{
    return (uint64_t)b.rle * BYTES_PER_POSITION + b.size + selectorSlots( b.rle ) * 8;
}

struct Launch
{
    uint32_t first{ 0 }, count{ 0 };   /* blocks [first, first + count) of the call, in buffer order */
    uint64_t positions{ 0 };           /* RLE1 bytes of the launch */
    uint64_t symbols{ 0 }, selectors{ 0 };
    uint64_t inputStart{ 0 }, inputBytes{ 0 };   /* the launch's input span in the buffers packed back to back */
    uint64_t bytes{ 0 };               /* device bytes (blockBytes summed) */
};

/** Launches of at most maxLaunchBlocks blocks (0: DEFAULT_LAUNCH_BLOCKS) whose blockBytes sum to at most `budget`
 * (0: DEFAULT_LAUNCH_BYTES); a single block over the budget gets a launch of its own. */
inline std::vector<Launch>
planLaunches( const std::vector<Block>& blocks, uint32_t maxLaunchBlocks, uint64_t budget )
{
    const uint32_t cap = maxLaunchBlocks == 0 ? DEFAULT_LAUNCH_BLOCKS : maxLaunchBlocks;
    const uint64_t limit = budget == 0 ? DEFAULT_LAUNCH_BYTES : budget;
    std::vector<Launch> launches;
    uint64_t input = 0;
    for ( uint32_t i = 0; i < blocks.size(); ++i ) {
        const Block& b = blocks[i];
        const uint64_t need = blockBytes( b );
        if ( launches.empty() || launches.back().count == cap || launches.back().bytes + need > limit ) {
            Launch l;
            l.first = i;
            l.inputStart = input;
            launches.push_back( l );
        }
        Launch& l = launches.back();
        l.count += 1;
        l.positions += b.rle;
        l.symbols += symbolSlots( b.rle );
        l.selectors += selectorSlots( b.rle );
        l.inputBytes += b.size;
        l.bytes += need;
        input += b.size;
    }
    return launches;
}

/** Block map entries of a buffer with `blocks` data blocks: one per block, the end-of-stream block and the end of the
 * file -- or, for an empty stream, the single entry {0: 0}. */
inline uint64_t
mapEntries( uint32_t blocks )
{
    return blocks == 0 ? 1 : (uint64_t)blocks + 2;
}

/** Bits of a buffer's stream: "BZh<level>", the blocks, the end-of-stream magic and combined CRC. */
inline uint64_t
streamBits( uint64_t blockBits )
{
    return 32 + blockBits + 48 + 32;
}

/** Bytes of a stream of `bits` bits: zero padded to a byte. */
inline uint64_t
streamBytes( uint64_t bits )
{
    return ( bits + 7 ) / 8;
}

/** bzip2's stream CRC: crc = rotl( crc, 1 ) ^ blockCrc over its blocks in order. */
inline uint32_t
combineCrc( uint32_t streamCrc, uint32_t blockCrc )
{
    return ( ( streamCrc << 1 ) | ( streamCrc >> 31 ) ) ^ blockCrc;
}
}  // namespace mi355x::compress
