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
 *
 * A SET of patterns S = (P_0 .. P_{k-1}) (mi355x_bz2_reader_search_set; 1 <= k <= SET_MAX_PATTERNS, 1 <= m_i <=
 * SEARCH_PATTERN_MAX, sum of the m_i <= SET_MAX_BYTES, m_min and m_max their extremes; equal patterns and prefixes of one
 * another allowed) is searched in one pass over the same launches: a match is a PAIR (p, i) with D[p : p + m_i] == P_i,
 * start <= p and p + m_i <= end -- the end rule per pattern --, and a result is ordered by ascending p, then ascending i.
 * planSearchSet is planSearch with m_min deciding whether the clipped range can hold any match.  Heads and tails have
 * seamLength( m_max, size ) bytes, and pattern i uses the last m_i - 1 bytes of a tail and the first m_i - 1 bytes of a
 * head: the argument above holds for every pattern on its own, with m = m_i, and m_i - 1 <= m_max - 1.
 *
 * The limit is the one place where a set differs.  With one pattern, every match that crosses the end b of the launches
 * at the front starts behind every match inside them (p > b - m against p' <= b - m).  With a set this is false: a long
 * pattern can cross b from p = b - 100 while a short one matches entirely inside the front at p' = b - 50, and (p, long)
 * sorts in front of (p', short).  A pair that the front launches cannot see has p + m_i > b, hence p > b - m_max; a pair
 * with p + m_max <= b therefore sorts in front of every unseen one.  So the launches behind the front may be skipped only
 * once the finished front launches hold >= limit pairs with p + m_max <= b (safePairs counts them per extent, with the
 * extent's own end for b, which is never behind the front's), and the merged result -- the extents' pairs and the seam
 * pairs really merged by (p, i), since inside one extent seam pairs no longer all follow the extent's own pairs -- is
 * cut to `limit` afterwards.  The invariant: the result with a limit is the first `limit` pairs of the result without.
 *
 * Ignoring case (SEARCH_IGNORE_CASE, `fold` below) changes one thing: two bytes are equal if foldAscii makes them equal.
 * foldAscii( b ) = b | 0x20 for 'A' <= b <= 'Z' and b for every other byte -- bytes.lower() of Python, `LC_ALL=C grep -i`;
 * the bytes 0x80 .. 0xFF are never changed.  A match of P at p is then foldAscii( D[p + j] ) == foldAscii( P[j] ) for all
 * j < m.  No size, range, order or limit depends on it: the plans are the same plans, the seam bytes come back raw and
 * are folded here, and patterns of a set that are equal under folding each report their own pairs.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bz2_ranges.hpp"

namespace bz2gpu
{
constexpr uint32_t SEARCH_PATTERN_MAX = 256;
constexpr uint32_t SET_MAX_PATTERNS = 1024;
constexpr uint32_t SET_MAX_BYTES = 16384;

/* The flags of a search (MI355X_BZ2_SEARCH_* of the C ABI).  Every later option of grep gets its bit here. */
constexpr uint32_t SEARCH_IGNORE_CASE = 1u;
constexpr uint32_t SEARCH_KNOWN_FLAGS = SEARCH_IGNORE_CASE;

/** b | 0x20 for 'A' .. 'Z', every other byte as it is. */
[[nodiscard]] constexpr uint8_t
foldAscii( uint8_t b )
{
    return b >= 'A' && b <= 'Z' ? (uint8_t)( b | 0x20 ) : b;
}

/** bytes[0, n) under foldAscii if `fold`, else as they are. */
[[nodiscard]] inline std::vector<uint8_t>
foldedBytes( const uint8_t* bytes, size_t n, bool fold )
{
    std::vector<uint8_t> result( bytes, bytes + n );
    if ( fold ) {
        for ( auto& byte : result ) byte = foldAscii( byte );
    }
    return result;
}

/* The set as the kernels read it (bz2_search_set.hip.h), one image that a workgroup copies into LDS:
 *   [0, SET_MAX_BYTES)      the pattern bytes, concatenated in set order;
 *   SET_TABLE_AT            one uint32 per pattern, ordered by (first byte, id):
 *                           offset of its bytes | (m_i - 1) << SET_ENTRY_SIZE_SHIFT | id << SET_ENTRY_ID_SHIFT;
 *   SET_FIRST_AT            one uint32 per first byte: begin of its bucket in the table | length << 16; 0 = none.
 * For a search that ignores case (writeSetImage with fold) the pattern bytes are stored under foldAscii and "first byte"
 * reads "folded first byte": a bucket holds every pattern whose first byte folds to its index, in id order, and the buckets
 * of 'A' .. 'Z' are empty. */
constexpr uint32_t SET_TABLE_AT = SET_MAX_BYTES;
constexpr uint32_t SET_FIRST_AT = SET_TABLE_AT + SET_MAX_PATTERNS * 4;
constexpr uint32_t SET_IMAGE_BYTES = SET_FIRST_AT + 256 * 4;
constexpr uint32_t SET_ENTRY_SIZE_SHIFT = 14, SET_ENTRY_ID_SHIFT = 22;

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
 * tail of seamLength( m, size ) bytes, raw.  With `fold`, equal reads equal under foldAscii; the pattern in any case.
 */
inline std::vector<uint64_t>
seamMatches( const uint8_t* pattern, uint32_t m, const std::vector<ExtentSeam>& seams, bool fold = false )
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
    const auto compared = foldedBytes( pattern, m, fold );
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
        if ( fold ) {
            for ( auto& byte : window ) byte = foldAscii( byte );
        }
        /* starts in the tail; the match reaches behind b (inFront <= m - 1 < m) and must fit into the window */
        for ( size_t at = 0; at < inFront && at + m <= window.size(); ++at ) {
            if ( std::memcmp( window.data() + at, compared.data(), m ) == 0 ) matches.push_back( b - inFront + at );
        }
    }
    return matches;
}

/* ------------------------------------------------------------------------------------------------ sets of patterns */

struct PatternSet
{
    std::vector<uint8_t> bytes;             /* the patterns, concatenated in set order */
    std::vector<uint32_t> offsets, sizes;   /* per pattern */
    uint32_t mMin{ 0 }, mMax{ 0 };
    bool fold{ false };                     /* the search ignores case ... */
    std::vector<uint8_t> folded;            /* ... and compares these: `bytes` under foldAscii (empty without fold) */

    [[nodiscard]] uint32_t count() const { return (uint32_t)sizes.size(); }
    [[nodiscard]] const uint8_t* pattern( uint32_t i ) const { return bytes.data() + offsets[i]; }
};

/** A (position, pattern id) pair; ordered by position, then id. */
using SetMatch = std::pair<uint64_t, uint32_t>;

/** Empty if (sizes, n) is a set the search takes, else the sentence that names the limit that was broken. */
[[nodiscard]] inline std::string
patternSetError( const uint32_t* sizes, uint64_t n )
{
    if ( n == 0 || n > SET_MAX_PATTERNS ) {
        return "the set must have 1 to " + std::to_string( SET_MAX_PATTERNS ) + " patterns, not " + std::to_string( n );
    }
    uint64_t sum = 0;
    for ( uint64_t i = 0; i < n; ++i ) {
        if ( sizes[i] == 0 || sizes[i] > SEARCH_PATTERN_MAX ) {
            return "every pattern must have 1 to " + std::to_string( SEARCH_PATTERN_MAX ) + " bytes, pattern "
                   + std::to_string( i ) + " has " + std::to_string( sizes[i] );
        }
        sum += sizes[i];
    }
    if ( sum > SET_MAX_BYTES ) {
        return "the patterns must have at most " + std::to_string( SET_MAX_BYTES ) + " bytes in total, not " + std::to_string( sum );
    }
    return {};
}

/** `patterns`: the concatenation of the patterns in set order.  Throws std::invalid_argument with patternSetError.  `fold`
 * changes neither ids, sizes nor m_min and m_max. */
inline PatternSet
makePatternSet( const uint8_t* patterns, const uint32_t* sizes, uint64_t n, bool fold = false )
{
    const auto why = patternSetError( sizes, n );
    if ( !why.empty() ) throw std::invalid_argument( why );
    PatternSet set;
    set.sizes.assign( sizes, sizes + n );
    set.offsets.resize( n );
    uint32_t at = 0;
    for ( uint64_t i = 0; i < n; ++i ) {
        set.offsets[i] = at;
        at += sizes[i];
    }
    set.bytes.assign( patterns, patterns + at );
    set.fold = fold;
    if ( fold ) set.folded = foldedBytes( patterns, at, true );
    set.mMin = *std::min_element( set.sizes.begin(), set.sizes.end() );
    set.mMax = *std::max_element( set.sizes.begin(), set.sizes.end() );
    return set;
}

/** The image of the set for the kernels: SET_IMAGE_BYTES bytes at `image` (4-byte aligned), laid out as described at
 * SET_TABLE_AT; with `fold`, the image of the set under foldAscii (whether or not the set itself was made with it). */
inline void
writeSetImage( const PatternSet& set, uint8_t* image, bool fold = false )
{
    std::memset( image, 0, SET_IMAGE_BYTES );
    std::memcpy( image, set.bytes.data(), set.bytes.size() );
    if ( fold ) {
        for ( size_t i = 0; i < set.bytes.size(); ++i ) image[i] = foldAscii( image[i] );
    }
    std::vector<uint32_t> order( set.count() );
    for ( uint32_t i = 0; i < set.count(); ++i ) order[i] = i;
    /* the image holds the bytes that are compared: ordered by their first one, equal first bytes by id */
    std::stable_sort( order.begin(), order.end(), [&set, image] ( uint32_t a, uint32_t b ) { return image[set.offsets[a]] < image[set.offsets[b]]; } );
    auto* const table = reinterpret_cast<uint32_t*>( image + SET_TABLE_AT );
    auto* const first = reinterpret_cast<uint32_t*>( image + SET_FIRST_AT );
    for ( uint32_t e = 0; e < set.count(); ++e ) {
        const uint32_t id = order[e], byte = image[set.offsets[id]];
        table[e] = set.offsets[id] | ( ( set.sizes[id] - 1 ) << SET_ENTRY_SIZE_SHIFT ) | ( id << SET_ENTRY_ID_SHIFT );
        first[byte] = first[byte] == 0 ? ( e | ( 1u << 16 ) ) : first[byte] + ( 1u << 16 );
    }
}

/** planSearch for a set: m_min decides whether the clipped range can hold any match. */
inline SearchPlan
planSearchSet( const std::vector<std::pair<uint64_t, uint64_t> >& map, uint64_t start, uint64_t end, const PatternSet& set,
               size_t cap, bool packed, uint64_t fileBytes )
{
    if ( !patternSetError( set.sizes.data(), set.count() ).empty() ) throw std::invalid_argument( "search: not a set of patterns" );
    return planSearch( map, start, end, set.mMin, cap, packed, fileBytes );
}

/**
 * Every pair (p, i), in (p, i) order and once, with D[p : p + m_i] == P_i whose bytes lie inside the extents' union but not
 * inside a single extent.  `seams` as for seamMatches, each with its head and tail of seamLength( m_max, size ) bytes.
 * With `fold`, equal reads equal under foldAscii.
 */
inline std::vector<SetMatch>
seamMatchesSet( const PatternSet& set, const std::vector<ExtentSeam>& seams, bool fold )
{
    if ( !patternSetError( set.sizes.data(), set.count() ).empty() ) throw std::invalid_argument( "seamMatchesSet: not a set of patterns" );
    for ( size_t i = 0; i < seams.size(); ++i ) {
        const auto n = seamLength( set.mMax, seams[i].size );
        if ( seams[i].head.size() != n || seams[i].tail.size() != n
             || ( i > 0 && seams[i].fileOffset != seams[i - 1].fileOffset + seams[i - 1].size ) ) {
            throw std::invalid_argument( "seamMatchesSet: extent " + std::to_string( i ) + " does not follow the one in front of "
                                         "it, or its head and tail have the wrong size" );
        }
    }
    std::vector<SetMatch> matches;
    if ( set.mMax == 1 || seams.empty() ) return matches;
    const uint64_t unionEnd = seams.back().fileOffset + seams.back().size;
    const uint32_t reach = set.mMax - 1;
    const auto folded = fold && !set.fold ? foldedBytes( set.bytes.data(), set.bytes.size(), true ) : std::vector<uint8_t>{};
    const uint8_t* const compared = !fold ? set.bytes.data() : set.fold ? set.folded.data() : folded.data();
    std::vector<uint8_t> window;
    for ( size_t i = 0; i + 1 < seams.size(); ++i ) {
        const auto& extent = seams[i];
        if ( extent.size == 0 ) continue;
        const uint64_t b = extent.fileOffset + extent.size;
        if ( b == unionEnd ) break;    /* nothing but empty extents follows */
        /* the tail of i, then the heads behind b until m_max - 1 bytes are there or the extents end: the same window as
         * seamMatches builds for m_max, of which pattern i looks at the m_i - 1 bytes on either side of b */
        window.assign( extent.tail.begin(), extent.tail.end() );
        const size_t inFront = window.size();
        for ( size_t j = i + 1; j < seams.size() && window.size() - inFront < reach; ++j ) {
            window.insert( window.end(), seams[j].head.begin(), seams[j].head.end() );
        }
        if ( fold ) {
            for ( auto& byte : window ) byte = foldAscii( byte );
        }
        /* ascending p, then ascending id: a pair starts in the tail, reaches behind b and fits into the window */
        for ( size_t at = 0; at < inFront; ++at ) {
            for ( uint32_t id = 0; id < set.count(); ++id ) {
                const uint32_t m = set.sizes[id];
                if ( at + m <= inFront || at + m > window.size() ) continue;
                if ( std::memcmp( window.data() + at, compared + set.offsets[id], m ) == 0 ) matches.push_back( { b - inFront + at, id } );
            }
        }
    }
    return matches;
}

/** seamMatchesSet as the set was made: folded if makePatternSet was given fold. */
inline std::vector<SetMatch>
seamMatchesSet( const PatternSet& set, const std::vector<ExtentSeam>& seams )
{
    return seamMatchesSet( set, seams, set.fold );
}

/** Of the pairs of one extent (ascending positions in D), how many have p + m_max <= the extent's end: each sorts in
 * front of every pair that needs a byte behind the extent, whatever its pattern (the file's header says why). */
[[nodiscard]] inline uint64_t
safePairs( const uint64_t* positions, uint64_t n, uint64_t extentEnd, uint32_t mMax )
{
    if ( extentEnd < mMax ) return 0;
    return (uint64_t)( std::upper_bound( positions, positions + n, extentEnd - mMax ) - positions );
}
}  // namespace bz2gpu
