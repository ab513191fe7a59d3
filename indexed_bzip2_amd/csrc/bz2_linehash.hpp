/**
 * bz2_linehash.hpp -- one 61-bit hash per line of the decoded file (mi355x_bz2_reader_line_hashes, _distinct_lines): the
 * hash, the summary of a stretch of bytes under it, the rule that stitches the summaries of stretches that lie back to
 * back, and the plan of the blocks a range of lines needs.  Host code only, no HIP: the reader and the context call it,
 * and tests/native/linehash_cases.cpp pins it on the CPU.
 *
 * The hash.  p = 2^61 - 1.  splitmix64( s ): z = s + 0x9E3779B97F4A7C15; z = ( z ^ z >> 30 ) * 0xBF58476D1CE4E5B9;
 * z = ( z ^ z >> 27 ) * 0x94D049BB133111EB; z ^ z >> 31, all mod 2^64.  The base of a 64-bit seed is
 * x = 256 + splitmix64( seed ) mod ( p - 256 ).  The hash of a line is the hash of its CONTENT, its bytes without the
 * closing delimiter: h = 0, then h = ( h * x + b + 1 ) mod p for every byte b; the canonical value in [0, p).  The + 1
 * makes contents of different lengths different polynomials in x: "\0" and "\0\0" differ and the empty line hashes to 0.
 * Two distinct contents of at most L bytes are the same for at most L of the p - 256 bases: the hash tells lines apart
 * with that probability, not with certainty, and a second seed is an independent check.
 *
 * Lines are numbered as grep numbers them (D = the decoded file, nl = the delimiter byte): line k is closed by the k-th
 * nl, counted from 0; a non-empty unterminated tail is one more line, an empty one is none.
 *
 * Composition.  Beside each hash goes xl = x^len mod p, so that nobody exponentiates: ( h1, xl1 ) followed by
 * ( h2, xl2 ) is ( h1 * xl2 + h2, xl1 * xl2 ); the empty string is ( 0, 1 ).  The summary of a stretch S:
 *     head          ( h, xl ) of the bytes in front of its first nl, of all of S if it holds none;
 *     hasDelimiter;
 *     tail          ( h, xl ) of the bytes behind its last nl; ( 0, 1 ) without one;
 *     tailNonEmpty  S is not empty and its last byte is not nl;
 *     hashes        of the lines S closes, in order, the first computed as if S were entered with hash 0.
 * Stitching S_0, S_1, ... that lie back to back, the carry starting at ( 0, 1 ): with a delimiter, the first closed line
 * of S_i becomes carry.h * head.xl + head.h and the carry becomes the tail; without one the carry becomes the carry
 * followed by the head.  At the end of D a carry over at least one byte is the unterminated tail's hash.  One rule serves
 * between the chunks of a tile, between the tiles of a span (bz2_linehash.hip.h, and summarise here) and between the
 * launches of a file (stitchSummaries).
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bz2_lines.hpp"

namespace bz2gpu
{
constexpr uint64_t LINEHASH_P = ( uint64_t( 1 ) << 61 ) - 1;
constexpr uint32_t LINEHASH_CHUNK_BYTES = 256;    /* of the kernels, for mi355x_bz2_line_hash_chunk_bytes */

[[nodiscard]] constexpr uint64_t
splitmix64( uint64_t s )
{
    uint64_t z = s + 0x9E3779B97F4A7C15ull;
    z = ( z ^ ( z >> 30 ) ) * 0xBF58476D1CE4E5B9ull;
    z = ( z ^ ( z >> 27 ) ) * 0x94D049BB133111EBull;
    return z ^ ( z >> 31 );
}

/** The base x of a seed: in [256, p). */
[[nodiscard]] constexpr uint64_t
lineHashBase( uint64_t seed )
{
    return 256 + splitmix64( seed ) % ( LINEHASH_P - 256 );
}

/** a * b mod p for a, b < 2^61 ... in fact for any a * b < 2^122: the canonical value in [0, p). */
[[nodiscard]] inline uint64_t
mulmod( uint64_t a, uint64_t b )
{
    const unsigned __int128 product = (unsigned __int128)a * b;
    const uint64_t lo = (uint64_t)product, hi = (uint64_t)( product >> 64 );
    uint64_t r = ( lo & LINEHASH_P ) + ( ( lo >> 61 ) | ( hi << 3 ) );
    r = ( r & LINEHASH_P ) + ( r >> 61 );
    return r >= LINEHASH_P ? r - LINEHASH_P : r;
}

/** ( a + b ) mod p for a, b < p. */
[[nodiscard]] inline uint64_t
addmod( uint64_t a, uint64_t b )
{
    const uint64_t r = a + b;
    return r >= LINEHASH_P ? r - LINEHASH_P : r;
}

/** A string under the hash: its hash and x^length. */
struct HashPart
{
    uint64_t h{ 0 }, xl{ 1 };

    [[nodiscard]] bool operator==( const HashPart& o ) const { return h == o.h && xl == o.xl; }
};

/** a followed by b. */
[[nodiscard]] inline HashPart
followedBy( const HashPart& a, const HashPart& b )
{
    return { addmod( mulmod( a.h, b.xl ), b.h ), mulmod( a.xl, b.xl ) };
}

[[nodiscard]] inline HashPart
hashPart( uint64_t x, const uint8_t* bytes, size_t size )
{
    HashPart part;
    for ( size_t i = 0; i < size; ++i ) {
        part.h = addmod( mulmod( part.h, x ), uint64_t( bytes[i] ) + 1 );
        part.xl = mulmod( part.xl, x );
    }
    return part;
}

/** The hash of a line's content under the base of `seed`. */
[[nodiscard]] inline uint64_t
lineHash( const uint8_t* bytes, size_t size, uint64_t seed )
{
    return hashPart( lineHashBase( seed ), bytes, size ).h;
}

/** The summary of a stretch (the header says what the fields mean).  `count` is the number of lines the stretch closes,
 * whether or not `hashes` lists them all. */
struct HashSummary
{
    HashPart head, tail;
    bool hasDelimiter{ false }, tailNonEmpty{ false };
    uint64_t count{ 0 };
    std::vector<uint64_t> hashes;
};

/** The summary of one chunk, as a lane of k_linehash_chunks computes it. */
inline HashSummary
summariseChunk( uint64_t x, const uint8_t* bytes, size_t size, uint8_t nl )
{
    HashSummary s;
    HashPart part;
    for ( size_t at = 0; at < size; ++at ) {
        if ( bytes[at] != nl ) {
            part = followedBy( part, { uint64_t( bytes[at] ) + 1, x } );
            continue;
        }
        if ( !s.hasDelimiter ) s.head = part;
        s.hasDelimiter = true;
        s.hashes.push_back( part.h );
        part = {};
    }
    ( s.hasDelimiter ? s.tail : s.head ) = part;
    s.tailNonEmpty = size > 0 && bytes[size - 1] != nl;
    s.count = s.hashes.size();
    return s;
}

/** `all` followed by `part`, both with all their hashes listed: the rule of the header between two stretches. */
inline void
appendSummary( HashSummary& all, const HashSummary& part )
{
    HashPart& carry = all.hasDelimiter ? all.tail : all.head;
    if ( part.hasDelimiter ) {
        all.hashes.push_back( followedBy( carry, part.head ).h );
        all.hashes.insert( all.hashes.end(), part.hashes.begin() + 1, part.hashes.end() );
        if ( !all.hasDelimiter ) all.head = followedBy( all.head, part.head );
        all.tail = part.tail;
        all.hasDelimiter = true;
        all.tailNonEmpty = part.tailNonEmpty;
    } else {
        carry = followedBy( carry, part.head );
        /* a part without a delimiter is empty or ends in a byte of its head */
        all.tailNonEmpty = all.tailNonEmpty || part.tailNonEmpty;
    }
    all.count = all.hashes.size();
}

/** The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as the kernels compose them.  The result
 * does not depend on `chunk`. */
inline HashSummary
summarise( uint64_t x, const uint8_t* bytes, size_t size, uint8_t nl, size_t chunk )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summarise: the chunk size must not be 0" );
    HashSummary all;
    for ( size_t at = 0; at < size; at += chunk ) {
        appendSummary( all, summariseChunk( x, bytes + at, std::min( chunk, size - at ), nl ) );
    }
    return all;
}

/** A stretch of D for stitchSummaries: where it lies and its summary.  The summary may list fewer hashes than
 * summary.count, or none: the reader's launches write theirs to device memory and report the count. */
struct HashStretch
{
    uint64_t fileOffset{ 0 }, size{ 0 };
    HashSummary summary;
};

/** What stitchSummaries found: the number of lines the stretches close, and the unterminated tail behind them. */
struct StitchedHashes
{
    uint64_t closed{ 0 };
    bool hasTail{ false };
    uint64_t tailHash{ 0 };
};

/**
 * The rule of the header over stretches that lie back to back (checked: std::invalid_argument) from the offset of the
 * first one, which must be entered with an empty carry: offset 0 or the byte behind a delimiter.  The closed lines are
 * numbered from 0 in the order the stretches close them.  patch( k, hash ), if given, is called for every closed line k
 * whose hash the carry changes -- the first closed line of every stretch but the first that has a delimiter, as long as
 * its summary lists a hash at all -- with the hash it has in D; every other line keeps the hash its stretch lists.
 */
template<typename Patch>
inline StitchedHashes
stitchSummaries( const std::vector<HashStretch>& stretches, const Patch& patch )
{
    StitchedHashes result;
    HashPart carry;
    bool carryNonEmpty = false;
    uint64_t end = stretches.empty() ? 0 : stretches.front().fileOffset;
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchSummaries: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        if ( stretch.size > ~uint64_t( 0 ) - end ) throw std::invalid_argument( "stitchSummaries: the stretches overflow 64 bits" );
        end += stretch.size;
        if ( stretch.size == 0 ) continue;
        const auto& s = stretch.summary;
        if ( s.hasDelimiter ) {
            if ( s.count == 0 ) throw std::invalid_argument( "stitchSummaries: a stretch with a delimiter closes no line" );
            if ( carryNonEmpty ) patch( result.closed, addmod( mulmod( carry.h, s.head.xl ), s.head.h ) );
            result.closed += s.count;
            carry = s.tail;
            carryNonEmpty = s.tailNonEmpty;
        } else {
            carry = followedBy( carry, s.head );
            carryNonEmpty = true;
        }
    }
    result.hasTail = carryNonEmpty;
    result.tailHash = carryNonEmpty ? carry.h : 0;
    return result;
}

/** stitchSummaries into one list: every closed line's hash, then the tail's if there is one.  Every stretch must list
 * all its hashes. */
inline std::vector<uint64_t>
stitchedHashes( const std::vector<HashStretch>& stretches )
{
    std::vector<uint64_t> hashes;
    for ( const auto& stretch : stretches ) {
        if ( stretch.summary.hashes.size() != stretch.summary.count ) {
            throw std::invalid_argument( "stitchedHashes: a stretch does not list all its hashes" );
        }
        hashes.insert( hashes.end(), stretch.summary.hashes.begin(), stretch.summary.hashes.end() );
    }
    const auto stitched = stitchSummaries( stretches, [&] ( uint64_t k, uint64_t hash ) { hashes[(size_t)k] = hash; } );
    if ( stitched.hasTail ) hashes.push_back( stitched.tailHash );
    return hashes;
}

/**
 * Which blocks the lines [first, first + count) need, and what their hashes are once the blocks' stretches are stitched.
 * The blocks are those planLines decodes for the range (first, count): the block that holds the delimiter in front of
 * line `first` (the first block for first == 0) through the block that holds the delimiter that closes the range's last
 * line (the last block where the range reaches the unterminated tail), each once.  stretches[k] is the k-th piece of
 * those blocks: launch, place in the launch's output, offset in D.  The stretches lie back to back, and the first one
 * starts at a block: the lines it closes are numbered from firstClosed = the delimiters in front of that block, so line
 * `first` is closed line first - firstClosed of the stitched stretches -- and if first > firstClosed, the closed lines in
 * front of it, whose first one may have begun in an earlier block, are not asked for.  N = the delimiters of D;
 * reachesEnd: the range goes past line N - 1, so the unterminated tail, if D has one, is its last line.
 */
struct LineHashPlan
{
    struct Piece
    {
        uint32_t launch{ 0 };
        uint64_t src{ 0 }, size{ 0 }, fileOffset{ 0 };
    };

    std::vector<RangeLaunch> launches;
    std::vector<Piece> stretches;
    uint64_t firstClosed{ 0 }, N{ 0 };
    uint64_t first{ 0 }, count{ 0 };     /* the range, count clipped to N + 1 - first (the tail may turn out empty) */
    bool reachesEnd{ false };

    /** The lines of the range that a delimiter closes: all of them but the unterminated tail. */
    [[nodiscard]] uint64_t wantedClosed() const { return reachesEnd ? N - first : count; }
};

inline LineHashPlan
planLineHashes( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* lineBytes, const uint64_t* lineLines,
                size_t nIndex, uint64_t first, uint64_t count, size_t cap, bool packed, uint64_t fileBytes )
{
    auto lines = planLines( map, lineBytes, lineLines, nIndex, &first, &count, 1, /* startsOnly */ false, cap, packed, fileBytes );
    LineHashPlan plan;
    plan.N = lineLines[nIndex - 1];
    plan.first = first;
    plan.count = first > plan.N ? 0 : std::min( count, plan.N + 1 - first );
    plan.reachesEnd = plan.count > 0 && plan.count > plan.N - first;
    plan.launches = std::move( lines.launches );
    if ( lines.segments.empty() ) {
        plan.count = 0;
        plan.launches.clear();
        return plan;
    }
    /* the first block of the range, as planLines finds it */
    size_t block = 0;
    if ( first > 0 ) block = static_cast<size_t>( std::lower_bound( lineLines, lineLines + nIndex, first ) - lineLines ) - 1;
    plan.firstClosed = lineLines[block];
    uint64_t at = lineBytes[block];
    for ( const auto& segment : lines.segments ) {
        plan.stretches.push_back( { segment.launch, segment.src, segment.size, at } );
        at += segment.size;
    }
    return plan;
}

/** A stretch's place in a column with one entry per line of the range: the stretch closes `closed` lines, the index says;
 * of those, `take` lines behind the first `skip` are wanted, and they are entries [at, at + take) of the column. */
struct ColumnPlace
{
    uint64_t skip{ 0 }, take{ 0 }, at{ 0 }, closed{ 0 };
};

/**
 * The place of every stretch of `plan`, from the line index the plan was made with: every launch knows where its lines go
 * before any has run.  The closed lines of the stretches are numbered from plan.firstClosed on, the wanted ones are
 * [first, first + wantedClosed()), and a stretch that closes none of them has take == 0.  The places tile the column
 * [0, wantedClosed()) in the order of the stretches; the unterminated tail, if the range reaches it, comes behind them.
 */
[[nodiscard]] inline std::vector<ColumnPlace>
placeLineColumn( const LineHashPlan& plan, const uint64_t* lineBytes, const uint64_t* lineLines, size_t nIndex )
{
    std::vector<ColumnPlace> places( plan.stretches.size() );
    const uint64_t first = plan.first, wantedClosed = plan.wantedClosed();
    uint64_t closedBefore = plan.firstClosed;
    for ( size_t k = 0; k < places.size(); ++k ) {
        const auto& piece = plan.stretches[k];
        const auto from = std::upper_bound( lineBytes, lineBytes + nIndex, piece.fileOffset ) - lineBytes - 1;
        const auto to = std::lower_bound( lineBytes, lineBytes + nIndex, piece.fileOffset + piece.size ) - lineBytes;
        auto& place = places[k];
        place.closed = lineLines[to] - lineLines[from];
        const uint64_t begin = std::max( closedBefore, first ), end = std::min( closedBefore + place.closed, first + wantedClosed );
        if ( end > begin ) place = { begin - closedBefore, end - begin, begin - first, place.closed };
        closedBefore += place.closed;
    }
    return places;
}
}  // namespace bz2gpu
