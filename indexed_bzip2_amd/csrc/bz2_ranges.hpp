/**
 * bz2_ranges.hpp -- how a batch of byte ranges of the decoded file (pread semantics, mi355x_bz2_reader_read_ranges) is
 * turned into GPU launches and gather pieces.  Host arithmetic only, no HIP: the reader calls it, and
 * tests/native/ranges_cases.cpp pins every decision on the CPU.
 *
 *   input   the block map as the reader holds it -- sorted {compressed bit offset -> decoded byte offset}, end-of-stream
 *           entries included (an entry followed by an equal decoded offset), the last entry is the end of what is known
 *           (the end-of-file entry once the map is complete) -- the ranges in caller order, and the cap on blocks per
 *           launch (the reader's batch size).
 *   output  launches: ascending lists of distinct data blocks.  The blocks that any range needs are listed once, in file
 *           order, and cut into launches of at most `cap` blocks; the blocks a range spans are therefore neighbours in
 *           that list, and its bytes are one contiguous stretch of a launch's ragged output unless a launch boundary falls
 *           inside it -- then the range becomes one piece per launch.
 *           pieces: {launch, src offset in that launch's output, dst offset, size}.  Range i goes to dst offset
 *           sizes[0] + ... + sizes[i - 1] (packed by REQUESTED size); n_read[i] is what the file holds of it, short only
 *           at the end of the file, and the bytes of the destination behind n_read[i] are not touched.
 *
 * End-of-stream blocks decode to nothing and are not launched: the output of a launch is the exclusive prefix sum of its
 * blocks' sizes in launch order (k_offsets), so a range that crosses a stream boundary stays contiguous without them.
 *
 * Bounded residency (the compressed file is not kept on the GPU): a launch brings only its own blocks.  Each block's
 * window is [the 4-byte word of its magic, the byte of the next map entry's bit offset + RANGE_WINDOW_SLACK), clipped to
 * the file; windows that touch or overlap (consecutive blocks) are merged, and the merged windows are packed back to
 * back at 4-byte aligned positions of one input buffer.  Every block's bit offset is rebased into that buffer.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <stdexcept>
#include <utility>
#include <vector>

namespace bz2gpu
{
/* How far past a block's last bit the decoder reads to decode it: the Huffman decoder peeks at the longest code length of
 * the block (at most 20 bits) from the position of its end-of-block symbol, and decides between "end of input" and
 * "invalid code" by `pos + maxLen > size_bits` (bz2_hscan.hip.h, k_hsym's end-of-input rule); the bit reader loads whole
 * 32-bit words.  So 3 bytes behind the block's last bit are read, rounded up to 8 here.  Loads beyond that (the 16-byte
 * loads and the word look-ahead) fall into the next window or the zero padding of the context's input buffer, and do not
 * change what a valid block decodes to.  (A DAMAGED block may report MI355X_BZ2_ERR_EOF where the whole file would let it
 * run on into the next block's bits and report another status.) */
constexpr uint64_t RANGE_WINDOW_SLACK = 8;

struct RangeWindow
{
    uint64_t from{ 0 }, to{ 0 };   /* file bytes [from, to) */
    uint64_t at{ 0 };              /* where they go in the launch's packed input */
};

struct RangeLaunch
{
    std::vector<uint64_t> bits;            /* ascending bit offsets of the blocks, in the file */
    std::vector<uint64_t> sizes;           /* decoded size of each block, as the map says */
    std::vector<uint64_t> outOffsets;      /* where each block's bytes land in the launch's output */
    uint64_t outBytes{ 0 };
    /* bounded residency only */
    std::vector<RangeWindow> windows;
    std::vector<uint64_t> packedBits;      /* the blocks' bit offsets inside the packed input */
    uint64_t packedBytes{ 0 };
};

struct GatherPiece
{
    uint32_t launch{ 0 };
    uint64_t src{ 0 }, dst{ 0 }, size{ 0 };
};

struct RangePlan
{
    std::vector<RangeLaunch> launches;
    std::vector<GatherPiece> pieces;       /* in caller order of the ranges, and front to back within a range */
    std::vector<uint64_t> nRead;           /* per range */
    uint64_t dstBytes{ 0 };                /* sum of the requested sizes */
    size_t distinctBlocks{ 0 };
};

/**
 * map: sorted {bits, decoded offset} pairs as described above (may be empty: then every range reads 0 bytes).
 * cap: blocks per launch (>= 1).  packed: plan the bounded-residency input (fileBytes: size of the compressed file).
 * Throws std::invalid_argument if the requested sizes do not add up within 64 bits, or the map is not sorted.
 */
inline RangePlan
planRanges( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* offsets, const uint64_t* sizes,
            size_t n, size_t cap, bool packed, uint64_t fileBytes )
{
    if ( cap == 0 ) {
        throw std::invalid_argument( "planRanges: a launch holds at least one block" );
    }
    RangePlan plan;
    plan.nRead.assign( n, 0 );

    /* data blocks: entries whose successor starts at a larger decoded offset */
    std::vector<uint64_t> starts, lengths, bits, nextBits;
    for ( size_t i = 0; i + 1 < map.size(); ++i ) {
        if ( map[i + 1].first <= map[i].first || map[i + 1].second < map[i].second ) {
            throw std::invalid_argument( "planRanges: the block map is not sorted" );
        }
        if ( map[i + 1].second > map[i].second ) {
            starts.push_back( map[i].second );
            lengths.push_back( map[i + 1].second - map[i].second );
            bits.push_back( map[i].first );
            nextBits.push_back( map[i + 1].first );
        }
    }
    const uint64_t total = map.empty() ? 0 : map.back().second;
    const auto blockOf = [&starts] ( uint64_t byteOffset ) {
        return static_cast<size_t>( std::upper_bound( starts.begin(), starts.end(), byteOffset ) - starts.begin() ) - 1;
    };

    /* the blocks every range spans: [first, last] per range, marked */
    constexpr uint32_t NONE = std::numeric_limits<uint32_t>::max();
    std::vector<uint32_t> ordinal( starts.size(), NONE );
    std::vector<std::pair<size_t, size_t> > spans( n, { 0, 0 } );
    for ( size_t i = 0; i < n; ++i ) {
        if ( plan.dstBytes > std::numeric_limits<uint64_t>::max() - sizes[i] ) {
            throw std::invalid_argument( "planRanges: the requested sizes exceed 64 bits" );
        }
        plan.dstBytes += sizes[i];
        if ( offsets[i] >= total || sizes[i] == 0 ) continue;
        plan.nRead[i] = std::min( sizes[i], total - offsets[i] );
        spans[i] = { blockOf( offsets[i] ), blockOf( offsets[i] + plan.nRead[i] - 1 ) };
        for ( size_t b = spans[i].first; b <= spans[i].second; ++b ) ordinal[b] = 0;
    }

    /* the marked blocks in file order, cut into launches of `cap` */
    uint32_t count = 0;
    for ( size_t b = 0; b < starts.size(); ++b ) {
        if ( ordinal[b] == NONE ) continue;
        ordinal[b] = count;
        if ( count % cap == 0 ) plan.launches.emplace_back();
        auto& launch = plan.launches.back();
        launch.bits.push_back( bits[b] );
        launch.sizes.push_back( lengths[b] );
        launch.outOffsets.push_back( launch.outBytes );
        launch.outBytes += lengths[b];
        if ( packed ) {
            const uint64_t from = ( bits[b] / 8 ) & ~uint64_t( 3 );
            const uint64_t to = std::min( fileBytes, ( nextBits[b] + 7 ) / 8 + RANGE_WINDOW_SLACK );
            if ( from >= to ) {
                throw std::invalid_argument( "planRanges: the block map names a block behind the end of the file" );
            }
            if ( !launch.windows.empty() && from <= launch.windows.back().to ) {
                launch.windows.back().to = std::max( launch.windows.back().to, to );
            } else {
                const uint64_t at = ( launch.packedBytes + 3 ) & ~uint64_t( 3 );
                launch.windows.push_back( { from, to, at } );
            }
            const auto& window = launch.windows.back();
            launch.packedBits.push_back( 8 * window.at + ( bits[b] - 8 * window.from ) );
            launch.packedBytes = window.at + ( window.to - window.from );
        }
        ++count;
    }
    plan.distinctBlocks = count;

    /* the pieces: a range walks through its blocks, one piece per launch it touches */
    uint64_t dst = 0;
    for ( size_t i = 0; i < n; dst += sizes[i], ++i ) {
        if ( plan.nRead[i] == 0 ) continue;
        const uint64_t end = offsets[i] + plan.nRead[i];
        uint64_t at = offsets[i];
        for ( size_t b = spans[i].first; at < end; ) {
            const uint32_t launch = ordinal[b] / (uint32_t)cap;
            /* the blocks b, b + 1, ... of the range have consecutive ordinals: those up to the launch's last one are here */
            const size_t inLaunch = std::min<size_t>( spans[i].second - b, ( launch + 1 ) * cap - 1 - ordinal[b] );
            const size_t last = b + inLaunch;
            const uint64_t pieceEnd = std::min( end, starts[last] + lengths[last] );
            const auto& l = plan.launches[launch];
            plan.pieces.push_back( { launch, l.outOffsets[ordinal[b] % cap] + ( at - starts[b] ), dst + ( at - offsets[i] ),
                                     pieceEnd - at } );
            at = pieceEnd;
            b = last + 1;
        }
    }
    return plan;
}
}  // namespace bz2gpu
