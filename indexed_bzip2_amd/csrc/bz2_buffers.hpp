/**
 * bz2_buffers.hpp -- plan of mi355x_bz2_decompress_buffers: many independent bzip2 buffers decoded in shared GPU batches.
 *
 * Host only, no HIP: bz2_buffers.cpp runs the plan, tests/native/buffers_cases.cpp checks it under ASan/UBSan.
 *   planWindows   buffers packed back to back, in order, into upload windows of at most a byte budget
 *   planWindow    the block-magic matches of a window assigned to their buffers (a match that straddles two buffers is
 *                 dropped) and cut into launches of at most maxLaunchBlocks; every candidate carries its buffer's end
 *   ChainWalk     after each launch: the block chain of every buffer whose candidates have been decoded, walked like the
 *                 reader at parallelization 1 (stream headers, block after block, end-of-stream blocks with the stream
 *                 CRC, trailing garbage), the buffer's result and the gather pieces that put its blocks in place
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <vector>

#include "../../include/mi355x_bz2.h"

namespace mi355x::buffers
{
constexpr uint64_t WINDOW_BYTES = uint64_t( 1 ) << 30;   /* compressed bytes uploaded at a time */
constexpr uint32_t DEFAULT_LAUNCH_BLOCKS = 512;          /* the reader's batch: 10.1 MB of scratch per block */

struct Window
{
    uint32_t first{ 0 }, count{ 0 };   /* buffers [first, first + count) */
    uint64_t bytes{ 0 };               /* their sizes summed */
};

/** Windows cut only at buffer boundaries; a buffer larger than the budget gets one of its own. */
inline std::vector<Window>
planWindows( const uint64_t* sizes, uint32_t n, uint64_t budget )
{
    std::vector<Window> windows;
    for ( uint32_t i = 0; i < n; ++i ) {
        if ( windows.empty() || ( windows.back().count > 0 && windows.back().bytes + sizes[i] > budget ) ) {
            windows.push_back( { i, 0, 0 } );
        }
        windows.back().count += 1;
        windows.back().bytes += sizes[i];
    }
    return windows;
}

struct Launch
{
    uint32_t first{ 0 }, count{ 0 };   /* candidates [first, first + count) */
};

struct WindowPlan
{
    std::vector<uint64_t> start;        /* byte offset of every buffer of the window; start[count] = window size */
    std::vector<uint64_t> bits;         /* candidates: block-magic bit offsets in the window, ascending */
    std::vector<uint64_t> endBytes;     /* candidate i's buffer ends here (byte offset in the window) */
    std::vector<uint32_t> buffer;       /* candidate i's buffer, relative to the window's first */
    std::vector<uint32_t> firstCandidate;   /* of buffer b; firstCandidate[count] = number of candidates */
    std::vector<Launch> launches;
};

/** `matches`: ascending bit offsets of the block magic in the packed window. */
inline WindowPlan
planWindow( const uint64_t* sizes, uint32_t count, const uint64_t* matches, uint64_t nMatches, uint32_t maxLaunchBlocks )
{
    WindowPlan p;
    p.start.resize( count + 1 );
    p.start[0] = 0;
    for ( uint32_t b = 0; b < count; ++b ) p.start[b + 1] = p.start[b] + sizes[b];
    p.firstCandidate.assign( count + 1, 0 );
    uint32_t b = 0;
    for ( uint64_t k = 0; k < nMatches; ++k ) {
        const uint64_t m = matches[k];
        while ( b < count && m >= 8 * p.start[b + 1] ) ++b;
        if ( b == count ) break;
        if ( m + 48 > 8 * p.start[b + 1] ) continue;   /* straddles the end of its buffer */
        p.bits.push_back( m );
        p.endBytes.push_back( p.start[b + 1] );
        p.buffer.push_back( b );
    }
    for ( uint32_t i = 0, c = 0; i <= count; ++i ) {
        while ( c < p.buffer.size() && p.buffer[c] < i ) ++c;
        p.firstCandidate[i] = c;
    }
    const uint32_t cap = maxLaunchBlocks == 0 ? DEFAULT_LAUNCH_BLOCKS : maxLaunchBlocks;
    for ( uint32_t c = 0; c < p.bits.size(); c += cap ) {
        p.launches.push_back( { c, std::min<uint32_t>( cap, (uint32_t)p.bits.size() - c ) } );
    }
    return p;
}

/** What the chain walk needs of a decoded candidate (from mi355x_bz2_block_result). */
struct Record
{
    uint64_t encodedSizeBits{ 0 }, decodedSize{ 0 }, dataOffset{ 0 };   /* dataOffset: in its launch's output */
    uint32_t computedCrc{ 0 };
    int32_t status{ MI355X_BZ2_OK };
};

/** Bytes [src, src + size) of a launch's output go to [dst, dst + size) of the result. */
struct Piece
{
    uint64_t src{ 0 }, dst{ 0 }, size{ 0 };
};

struct BufferResult
{
    uint64_t outputOffset{ 0 }, decodedSize{ 0 }, errorOffsetBits{ 0 };
    uint32_t blocks{ 0 }, streams{ 0 };
    bool trailingGarbage{ false };
    int32_t status{ MI355X_BZ2_OK };
};

/** Big-endian bits [pos, pos + count) of bytes[0, size), count <= 57; false if they run past the end. */
inline bool
peekBits( const uint8_t* bytes, uint64_t size, uint64_t pos, unsigned count, uint64_t& value )
{
    if ( pos + count > 8 * size ) return false;
    value = 0;
    for ( unsigned i = 0; i < count; ++i, ++pos ) value = ( value << 1 ) | ( ( bytes[pos >> 3] >> ( 7 - ( pos & 7 ) ) ) & 1u );
    return true;
}

/** readBzip2Header (bzip2.hpp:114-142) at byte `at`: "BZh" and a level '1'..'9'. */
inline bool
streamHeaderAt( const uint8_t* bytes, uint64_t size, uint64_t at )
{
    return at + 4 <= size && bytes[at] == 'B' && bytes[at + 1] == 'Z' && bytes[at + 2] == 'h' && bytes[at + 3] >= '1'
           && bytes[at + 3] <= '9';
}

/**
 * The block chains of the buffers of one window, walked launch by launch.  Buffers are walked in order; a buffer whose
 * chain reaches a candidate of a launch that has not run yet waits for it.  Its decoded blocks are placed behind the
 * buffers before it, so each piece is known the moment its launch has run.  A buffer that fails takes 0 bytes: the
 * next buffer is placed where it began, over whatever of it had been gathered already.
 */
class ChainWalk
{
public:
    /** `data[b]`: buffer b's bytes (b relative to the window); `outputBase`: where the window's first buffer goes. */
    ChainWalk( const WindowPlan& plan, const uint8_t* const* data, uint64_t outputBase ) :
        m_plan( plan ), m_data( data ), m_count( (uint32_t)plan.start.size() - 1 ), m_records( plan.bits.size() ),
        m_results( m_count ), m_next( outputBase )
    {}

    /** Records of launch `launch` (its candidates, in order) are in; returns the pieces of that launch's output. */
    std::vector<Piece>
    advance( uint32_t launch, const Record* records )
    {
        const Launch& l = m_plan.launches[launch];
        std::copy( records, records + l.count, m_records.begin() + l.first );
        m_decodedUpTo = l.first + l.count;
        walkAll();
        return m_pieces;
    }

    /** All launches have run (or there were none): walks what is left; every buffer then has its result. */
    const std::vector<BufferResult>&
    finish()
    {
        m_decodedUpTo = (uint32_t)m_plan.bits.size();
        walkAll();
        return m_results;
    }

    /** Where the buffer behind the last finished one goes. */
    uint64_t end() const { return m_next; }

private:
    enum class State { START, AFTER_STREAM_HEADER, AFTER_BLOCK };

    void
    walkAll()
    {
        m_pieces.clear();
        m_ownPieces = 0;   /* (a piece may run on from the buffer before into this one's bytes) */
        while ( m_buffer < m_count && walk() ) {
            m_next = m_results[m_buffer].outputOffset + m_results[m_buffer].decodedSize;
            ++m_buffer;
            m_state = State::START;
            m_ownPieces = m_pieces.size();
        }
    }

    /** Walks buffer m_buffer as far as the decoded candidates go; true when it has its result. */
    bool
    walk()
    {
        const uint32_t b = m_buffer;
        const uint8_t* const bytes = m_data[b];
        const uint64_t size = m_plan.start[b + 1] - m_plan.start[b];
        const uint64_t base = 8 * m_plan.start[b];
        BufferResult& r = m_results[b];
        const auto fail = [&] ( int32_t status, uint64_t at ) {
            r.status = status;
            r.errorOffsetBits = at;
            r.decodedSize = 0;
            /* its pieces of this launch would race with the next buffer's for the same bytes; earlier launches' pieces
             * have been gathered already and are simply overwritten */
            m_pieces.resize( m_ownPieces );
            if ( !m_pieces.empty() && m_pieces.back().dst + m_pieces.back().size > r.outputOffset ) {
                m_pieces.back().size = r.outputOffset - m_pieces.back().dst;   /* merged into the buffer before */
            }
            return true;
        };
        if ( m_state == State::START ) {
            r = BufferResult{};
            r.outputOffset = m_next;
            if ( size == 0 ) return true;   /* nothing to decode: b"", as the reader and bz2.decompress return */
            /* (the reader only looks at the header once its scan has found a block; any other bytes fail here) */
            if ( !streamHeaderAt( bytes, size, 0 ) ) return fail( MI355X_BZ2_ERR_STREAM_HEADER, 0 );
            m_pos = 32;
            m_crc = 0;
            m_state = State::AFTER_STREAM_HEADER;
        }
        for ( ;; ) {
            uint64_t magic = 0, stored = 0;
            const bool whole = peekBits( bytes, size, m_pos, 48, magic ) && peekBits( bytes, size, m_pos + 48, 32, stored );
            /* candidates of this buffer at or behind m_pos */
            const uint64_t at = base + m_pos;
            const auto begin = m_plan.bits.begin() + m_plan.firstCandidate[b];
            const auto last = m_plan.bits.begin() + m_plan.firstCandidate[b + 1];
            const auto it = std::lower_bound( begin, last, at );
            if ( whole && magic == MI355X_BZ2_MAGIC_EOS ) {
                if ( (uint32_t)stored != m_crc ) return fail( MI355X_BZ2_ERR_STREAM_CRC, m_pos );
                ++r.streams;
                m_pos = ( m_pos + 80 + 7 ) & ~uint64_t( 7 );
                m_crc = 0;
                if ( m_pos >= 8 * size ) return true;
                if ( !streamHeaderAt( bytes, size, m_pos / 8 ) ) {
                    r.trailingGarbage = true;   /* ignored, as the reader ignores it */
                    return true;
                }
                m_pos += 32;
                m_state = State::AFTER_STREAM_HEADER;
                continue;
            }
            if ( !whole || magic != MI355X_BZ2_MAGIC_BLOCK ) {
                /* Behind a stream header the reader takes the next block its magic scan found, and ends the file without
                 * complaint if there is none; behind a block it reads the header and fails. */
                if ( m_state == State::AFTER_STREAM_HEADER && it == last ) return true;
                return fail( whole ? MI355X_BZ2_ERR_BAD_MAGIC : MI355X_BZ2_ERR_EOF, m_pos );
            }
            /* a whole block magic inside the buffer is always a candidate: the scan finds every match */
            if ( it == last || *it != at ) return fail( MI355X_BZ2_ERR_LOGIC, m_pos );
            const uint32_t c = (uint32_t)( it - m_plan.bits.begin() );
            if ( c >= m_decodedUpTo ) return false;   /* in a launch still to come */
            const Record& rec = m_records[c];
            if ( rec.status != MI355X_BZ2_OK ) return fail( rec.status, m_pos );
            if ( rec.decodedSize > 0 ) {
                const uint64_t dst = r.outputOffset + r.decodedSize;
                if ( !m_pieces.empty() && m_pieces.back().src + m_pieces.back().size == rec.dataOffset
                     && m_pieces.back().dst + m_pieces.back().size == dst ) {
                    m_pieces.back().size += rec.decodedSize;
                } else {
                    m_pieces.push_back( { rec.dataOffset, dst, rec.decodedSize } );
                }
            }
            r.decodedSize += rec.decodedSize;
            r.blocks += 1;
            m_crc = ( ( m_crc << 1 ) | ( m_crc >> 31 ) ) ^ rec.computedCrc;
            m_pos += rec.encodedSizeBits;
            m_state = State::AFTER_BLOCK;
        }
    }

    const WindowPlan& m_plan;
    const uint8_t* const* m_data;
    uint32_t m_count;
    std::vector<Record> m_records;
    std::vector<BufferResult> m_results;
    std::vector<Piece> m_pieces;
    uint32_t m_decodedUpTo{ 0 };
    size_t m_ownPieces{ 0 };   /* m_pieces from here on are the current buffer's */
    uint32_t m_buffer{ 0 };
    State m_state{ State::START };
    uint64_t m_pos{ 0 };
    uint32_t m_crc{ 0 };
    uint64_t m_next{ 0 };
};
}  // namespace mi355x::buffers
