/**
 * bz2_search.hpp -- how a search for a byte string in a range of the decoded file (mi355x_bz2_reader_search) is turned
 * into GPU launches, and how the matches that no launch can see are found.  Host arithmetic only, no HIP: the reader
 * calls it, and tests/native/search_cases.cpp pins every decision on the CPU.
 *
 * Semantics (D = the decoded file, P = the pattern, m = len(P), 1 <= m <= SEARCH_MAX_PATTERN): a match is every offset p
 * with D[p : p + m] == P, start <= p and p + m <= end, start and end clipped to [0, size of D].  Matches that overlap
 * themselves all count (b"abab" in b"abababab": 0, 2 and 4).
 *
 *   launches  planRanges' launches for the single range [start, end): every data block that intersects the range once,
 *             in file order, at most `cap` per launch, with the packed windows of bounded residency when asked for.
 *   extents   one per launch: the part of the launch's output that lies inside [start, end) -- planRanges' piece of the
 *             range in that launch.  The blocks of a launch are neighbours in the file, so the extent is one stretch of
 *             the output, and offset in the output -> offset in D is one addition (fileOffset - src).  The extents lie
 *             back to back in D: extent l + 1 starts where extent l ends, the first at `start`, the last ends at `end`.
 *
 * Inside an extent the GPU finds every match (a span of mi355x_bz2_find_bytes).  A match whose m bytes do not lie inside
 * ONE extent -- at a cap of 1 every block boundary is such a seam, and with blocks of a few bytes one match crosses
 * several launches -- is found here, from the first and the last min(m - 1, size) bytes of every extent (ExtentSeam):
 *
 *   Such a match [p, p + m) holds bytes of at least two extents.  Let q be any of its bytes and j the extent that holds q.
 *   The match is not inside j, so it reaches beyond j's first byte or beyond j's last one.  If p < the start of j, then
 *   q < p + m <= start of j + m - 1: q is among the first m - 1 bytes of j.  Otherwise p + m > the end of j, and
 *   q >= p > end of j - m: q is among the last m - 1 bytes of j.  Head and tail of every extent therefore hold every
 *   byte of every such match (an extent shorter than 2 (m - 1) is given whole by the two together), and no byte of the
 *   inside of an extent decides one.
 *
 * seamMatches lists each of them once: under the extent that holds its first byte p.  For that extent i the match crosses
 * i's end b, so p lies in [max( start of i, b - m + 1 ), b), and its bytes are the tail of i from p on followed by the
 * heads of i + 1, i + 2, ... -- a head that is shorter than m - 1 is its whole extent, so the heads in front of the
 * first full one lie back to back in D, and m - 1 bytes behind b are always enough.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <utility>
#include <vector>

#include "bz2_ranges.hpp"

namespace bz2gpu
{
constexpr uint32_t SEARCH_PATTERN_MAX = 256;

struct SearchExtent
{
    uint64_t src{ 0 }, size{ 0 };      /* in the launch's output */
    uint64_t fileOffset{ 0 };          /* of its first byte in D */
};

struct SearchPlan
{
    std::vector<RangeLaunch> launches;
    std::vector<SearchExtent> extents; /* one per launch */
    uint64_t start{ 0 }, end{ 0 };     /* clipped; start == end if the range cannot hold a match */
};

/** What a launch hands back of its extent (beside its count and positions). */
struct ExtentSeam
{
    uint64_t fileOffset{ 0 }, size{ 0 };
    std::vector<uint8_t> head, tail;   /* the first and the last seamLength( m, size ) bytes */
};

[[nodiscard]] inline uint32_t
seamLength( uint32_t m, uint64_t size )
{
    return (uint32_t)std::min<uint64_t>( m - 1, size );
}

/**
 * map, cap, packed, fileBytes: as planRanges (the map complete as far as `end` reaches).  Throws std::invalid_argument
 * for m == 0 or m > SEARCH_PATTERN_MAX.  A range that is empty or shorter than m after the clip has no launches.
 */
inline SearchPlan
planSearch( const std::vector<std::pair<uint64_t, uint64_t> >& map, uint64_t start, uint64_t end, uint32_t m, size_t cap,
            bool packed, uint64_t fileBytes )
{
    if ( m == 0 || m > SEARCH_PATTERN_MAX ) {
        throw std::invalid_argument( "search: the pattern must have 1 to " + std::to_string( SEARCH_PATTERN_MAX ) + " bytes" );
    }
    const uint64_t total = map.empty() ? 0 : map.back().second;
    SearchPlan plan;
    plan.end = std::min( end, total );
    plan.start = std::min( start, plan.end );
    if ( plan.end - plan.start < m ) {
        plan.end = plan.start;
        return plan;
    }
    const uint64_t size = plan.end - plan.start;
    auto ranges = planRanges( map, &plan.start, &size, 1, cap, packed, fileBytes );
    if ( ranges.pieces.size() != ranges.launches.size() || ranges.nRead[0] != size ) {
        throw std::logic_error( "planSearch: the range does not have one piece per launch" );
    }
    plan.launches = std::move( ranges.launches );
    for ( const auto& piece : ranges.pieces ) {
        /* the destination of the one range is packed from 0: dst is the offset inside [start, end) */
        plan.extents.push_back( { piece.src, piece.size, plan.start + piece.dst } );
    }
    return plan;
}

/**
 * Every p, ascending and once, with D[p : p + m] == P whose bytes lie inside the extents' union but not inside a single
 * extent.  `seams`: the extents in file order, back to back (checked: std::invalid_argument), each with its head and
 * tail of seamLength( m, size ) bytes.
 */
inline std::vector<uint64_t>
seamMatches( const uint8_t* pattern, uint32_t m, const std::vector<ExtentSeam>& seams )
{
    if ( m == 0 || m > SEARCH_PATTERN_MAX ) throw std::invalid_argument( "seamMatches: the pattern must have 1 to 256 bytes" );
    for ( size_t i = 0; i < seams.size(); ++i ) {
        const auto n = seamLength( m, seams[i].size );
        if ( seams[i].head.size() != n || seams[i].tail.size() != n
             || ( i > 0 && seams[i].fileOffset != seams[i - 1].fileOffset + seams[i - 1].size ) ) {
            throw std::invalid_argument( "seamMatches: extent " + std::to_string( i ) + " does not follow the one in front of it, "
                                         "or its head and tail have the wrong size" );
        }
    }
    std::vector<uint64_t> matches;
    if ( m == 1 || seams.empty() ) return matches;
    const uint64_t unionEnd = seams.back().fileOffset + seams.back().size;
    std::vector<uint8_t> window;
    for ( size_t i = 0; i + 1 < seams.size(); ++i ) {
        const auto& extent = seams[i];
        if ( extent.size == 0 ) continue;
        const uint64_t b = extent.fileOffset + extent.size;
        if ( b == unionEnd ) break;    /* nothing but empty extents follows */
        /* the tail of i, then the heads behind b until m - 1 bytes are there or the extents end */
        window.assign( extent.tail.begin(), extent.tail.end() );
        const size_t inFront = window.size();
        for ( size_t j = i + 1; j < seams.size() && window.size() - inFront < m - 1; ++j ) {
            window.insert( window.end(), seams[j].head.begin(), seams[j].head.end() );
        }
        /* starts in the tail; the match reaches behind b (inFront <= m - 1 < m) and must fit into the window */
        for ( size_t at = 0; at < inFront && at + m <= window.size(); ++at ) {
            if ( std::memcmp( window.data() + at, pattern, m ) == 0 ) matches.push_back( b - inFront + at );
        }
    }
    return matches;
}
}  // namespace bz2gpu
