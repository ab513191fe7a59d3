/**
 * bz2_lines.hpp -- how a batch of line ranges of the decoded file (mi355x_bz2_reader_read_line_ranges, _line_starts) is
 * turned into GPU launches, boundary queries and gather pieces.  Host arithmetic only, no HIP: the reader calls it, and
 * tests/native/lines_cases.cpp pins every decision on the CPU.  The inverse direction -- byte offsets to line numbers,
 * planLineNumbers, under mi355x_bz2_reader_line_numbers and _grep -- is at the end of the file, pinned by
 * tests/native/linenum_cases.cpp.
 *
 * Semantics (D = the decoded file, nl = the delimiter, N = the number of nl bytes in D): line k starts at s(k), s(0) = 0
 * and s(k) = 1 + the position of the k-th nl for 1 <= k <= N; line N is the unterminated tail.  The range (first, count)
 * is D[s(first) : s(first + count)] if first + count <= N, D[s(first):] if first <= N < first + count, nothing if
 * first > N or count == 0.
 *
 *   input   the complete block map (bz2_ranges.hpp), the line index -- one entry per data block plus the end:
 *           {decoded offset of the block's first byte -> nl bytes in front of it}, ..., {size of D -> N} --, the ranges in
 *           caller order and the cap on blocks per launch.
 *   output  launches: planRanges' launches for the blocks every range spans -- the block that holds the first-th nl (the
 *           first block for first == 0) through the block that holds the (first + count)-th nl (the last block when there
 *           is none), every block between included; each block once, in file order, at most `cap` per launch, with the
 *           packed windows of bounded residency when asked for.  The launches and the whole-block pieces ARE planRanges':
 *           it is called with the byte ranges that cover those blocks.
 *           queries: {launch, span of one block in that launch's output, rank}: "where is the rank-th nl of this block".
 *           One per distinct {block, rank}.  Boundary 0 needs none (s(0) = 0) and a boundary beyond N needs none (the
 *           end of the file); no other boundary is known without looking: the index only counts.
 *           segments: per range and launch it touches, the stretch of that launch's output that covers its blocks
 *           there, and which query cuts its front (the range's first segment) or its back (its last one).
 *   then    resolveSegment turns a segment and the positions the GPU found into the piece to gather.  A launch resolves
 *           its own segments without knowing any other launch; only the destination offsets need all sizes.
 *
 * One case spelled out: the k-th nl is the LAST byte of block b.  Line k then starts at the first byte of block b + 1.
 * The query is {b, k - lines[b]}, its position p is the last byte of b's span, and the piece starts at p + 1: the first
 * byte behind b's span, which is block b + 1's first byte if that block follows in the same launch (blocks of a range
 * are neighbours in the launch list) -- or the end of the segment, which then is empty, and the range goes on with its
 * next segment at the start of the next launch.  Block b is decoded although it gives no byte: nobody knew before.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <map>
#include <stdexcept>
#include <utility>
#include <vector>

#include "bz2_ranges.hpp"

namespace bz2gpu
{
constexpr uint32_t NO_QUERY = std::numeric_limits<uint32_t>::max();
constexpr uint64_t NOT_FOUND = std::numeric_limits<uint64_t>::max();   /* what k_find_byte answers for "fewer" */

struct LineQuery
{
    uint32_t launch{ 0 };
    uint64_t spanOffset{ 0 }, spanSize{ 0 };   /* the block in the launch's output */
    uint64_t rank{ 0 };                        /* 1-based, within the block */
    uint64_t blockStart{ 0 };                  /* decoded offset of the block's first byte */
    uint64_t blockCount{ 0 };                  /* delimiters the index gives the block: the caller may check it */
};

struct LineSegment
{
    uint32_t range{ 0 }, launch{ 0 };
    uint64_t src{ 0 }, size{ 0 };              /* whole blocks of the launch's output */
    uint32_t startQuery{ NO_QUERY };           /* set: the piece starts behind that query's position */
    uint32_t endQuery{ NO_QUERY };             /* set: the piece ends behind that query's position */
};

struct LineStart
{
    uint64_t fixed{ 0 };                       /* s(k) if query == NO_QUERY */
    uint32_t query{ NO_QUERY };                /* else s(k) = lineStartOf( query, position ) */
};

struct LinePlan
{
    std::vector<RangeLaunch> launches;
    std::vector<LineQuery> queries;
    std::vector<LineSegment> segments;         /* in caller order of the ranges, front to back within a range */
    std::vector<LineStart> starts;             /* per range: s(first) (with segments: of the ranges that have bytes) */
    size_t distinctBlocks{ 0 };
};

/** The data blocks of a map: entries whose successor starts at a larger decoded offset (as planRanges sees them). */
inline void
dataBlocksOf( const std::vector<std::pair<uint64_t, uint64_t> >& map, std::vector<uint64_t>& starts,
              std::vector<uint64_t>& lengths )
{
    for ( size_t i = 0; i + 1 < map.size(); ++i ) {
        if ( map[i + 1].second > map[i].second ) {
            starts.push_back( map[i].second );
            lengths.push_back( map[i + 1].second - map[i].second );
        }
    }
}

/** Throws std::invalid_argument unless the line index fits the (complete) block map: its keys are the data blocks'
 * decoded offsets plus the size, its values start at 0, do not decrease, and give no block more delimiters than bytes. */
inline void
checkLineIndex( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* bytes, const uint64_t* lines, size_t n )
{
    std::vector<uint64_t> starts, lengths;
    dataBlocksOf( map, starts, lengths );
    const uint64_t total = map.empty() ? 0 : map.back().second;
    if ( n != starts.size() + 1 ) {
        throw std::invalid_argument( "line index: " + std::to_string( n ) + " entries for " + std::to_string( starts.size() )
                                     + " data blocks (one per block and the end are needed)" );
    }
    if ( lines[0] != 0 ) throw std::invalid_argument( "line index: the first entry must count 0 lines" );
    for ( size_t b = 0; b < starts.size(); ++b ) {
        if ( bytes[b] != starts[b] ) {
            throw std::invalid_argument( "line index: entry " + std::to_string( b ) + " is not at a block's decoded offset" );
        }
        if ( lines[b + 1] < lines[b] || lines[b + 1] - lines[b] > lengths[b] ) {
            throw std::invalid_argument( "line index: entry " + std::to_string( b + 1 )
                                         + " decreases, or gives its block more delimiters than bytes" );
        }
    }
    if ( bytes[n - 1] != total ) throw std::invalid_argument( "line index: the last entry is not at the decoded size" );
}

/**
 * map: the complete block map; lineBytes / lineLines: the line index (nIndex entries, checked against the map).
 * first / count: the ranges.  startsOnly: only s(first) of every range is wanted (line_starts): the launches then hold
 * just the blocks with a boundary to look for, and there are no segments.
 * cap, packed, fileBytes: as planRanges.
 */
inline LinePlan
planLines( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* lineBytes, const uint64_t* lineLines,
           size_t nIndex, const uint64_t* first, const uint64_t* count, size_t n, bool startsOnly, size_t cap, bool packed,
           uint64_t fileBytes )
{
    checkLineIndex( map, lineBytes, lineLines, nIndex );
    std::vector<uint64_t> starts, lengths;
    dataBlocksOf( map, starts, lengths );
    const size_t B = starts.size();
    const uint64_t total = map.empty() ? 0 : map.back().second;
    const uint64_t N = lineLines[B];
    /* the block that holds the k-th delimiter, 1 <= k <= N: lines[b] < k <= lines[b + 1] */
    const auto blockOf = [&] ( uint64_t k ) {
        return static_cast<size_t>( std::lower_bound( lineLines, lineLines + B + 1, k ) - lineLines ) - 1;
    };

    LinePlan plan;
    plan.starts.assign( n, {} );
    struct Ends { size_t firstBlock{ 0 }, lastBlock{ 0 }; uint64_t startRank{ 0 }, endRank{ 0 }; bool any{ false }; };
    std::vector<Ends> ends( n );
    std::vector<uint64_t> coverOffsets( n, 0 ), coverSizes( n, 0 );
    for ( size_t i = 0; i < n; ++i ) {
        auto& e = ends[i];
        if ( first[i] == 0 ) {
            plan.starts[i].fixed = 0;
        } else if ( first[i] > N ) {
            plan.starts[i].fixed = total;
        } else {
            e.firstBlock = blockOf( first[i] );
            e.startRank = first[i] - lineLines[e.firstBlock];
        }
        if ( startsOnly ) {
            e.any = e.startRank != 0;
            e.lastBlock = e.firstBlock;
        } else {
            if ( first[i] > N || count[i] == 0 || B == 0 ) continue;
            e.any = true;
            const uint64_t last = count[i] > N - first[i] ? NOT_FOUND : first[i] + count[i];   /* beyond N: to the end */
            e.lastBlock = last == NOT_FOUND ? B - 1 : blockOf( last );
            e.endRank = last == NOT_FOUND ? 0 : last - lineLines[e.lastBlock];
        }
        if ( e.any ) {
            coverOffsets[i] = starts[e.firstBlock];
            coverSizes[i] = starts[e.lastBlock] + lengths[e.lastBlock] - starts[e.firstBlock];
        }
    }

    /* launches and whole-block pieces: planRanges over the byte ranges that cover each range's blocks */
    auto cover = planRanges( map, coverOffsets.data(), coverSizes.data(), n, cap, packed, fileBytes );
    plan.launches = std::move( cover.launches );
    plan.distinctBlocks = cover.distinctBlocks;

    std::map<std::pair<size_t, uint64_t>, uint32_t> known;   /* {block, rank} -> query */
    const auto queryFor = [&] ( size_t block, uint64_t rank, uint32_t launch, uint64_t spanOffset ) {
        const auto [entry, isNew] = known.emplace( std::make_pair( block, rank ), (uint32_t)plan.queries.size() );
        if ( isNew ) plan.queries.push_back( { launch, spanOffset, lengths[block], rank, starts[block],
                                               lineLines[block + 1] - lineLines[block] } );
        return entry->second;
    };
    size_t piece = 0;
    uint64_t dst = 0;
    for ( size_t i = 0; i < n; dst += coverSizes[i], ++i ) {
        const auto& e = ends[i];
        if ( !e.any ) continue;
        /* the pieces of range i: those whose destination lies in its stretch (they come in caller order) */
        const size_t firstPiece = piece;
        while ( piece < cover.pieces.size() && cover.pieces[piece].dst < dst + coverSizes[i] ) ++piece;
        if ( piece == firstPiece ) throw std::logic_error( "planLines: a range without pieces" );
        const auto& front = cover.pieces[firstPiece];
        const auto& back = cover.pieces[piece - 1];
        const uint32_t startQuery = e.startRank == 0 ? NO_QUERY : queryFor( e.firstBlock, e.startRank, front.launch, front.src );
        plan.starts[i].query = startQuery;
        if ( startsOnly ) continue;
        const uint32_t endQuery = e.endRank == 0 ? NO_QUERY
                                                 : queryFor( e.lastBlock, e.endRank, back.launch,
                                                             back.src + back.size - lengths[e.lastBlock] );
        for ( size_t p = firstPiece; p < piece; ++p ) {
            const auto& g = cover.pieces[p];
            plan.segments.push_back( { (uint32_t)i, g.launch, g.src, g.size, p == firstPiece ? startQuery : NO_QUERY,
                                       p + 1 == piece ? endQuery : NO_QUERY } );
        }
    }
    return plan;
}

/** s(k) from the position (in the launch's output) the GPU found for a boundary query. */
inline uint64_t
lineStartOf( const LineQuery& query, uint64_t position )
{
    return query.blockStart + ( position - query.spanOffset ) + 1;
}

/**
 * The piece of a launch's output that a segment stands for, once the positions of its queries are known
 * (positions[q] for query q; NOT_FOUND = the block holds fewer delimiters than the index says).
 * False if the positions contradict the plan: not found, outside the query's span, or an end in front of the start.
 */
inline bool
resolveSegment( const LinePlan& plan, const LineSegment& segment, const uint64_t* positions, uint64_t* src, uint64_t* size )
{
    uint64_t from = segment.src, to = segment.src + segment.size;
    for ( const bool front : { true, false } ) {
        const uint32_t q = front ? segment.startQuery : segment.endQuery;
        if ( q == NO_QUERY ) continue;
        const auto& query = plan.queries[q];
        const uint64_t p = positions[q];
        if ( p == NOT_FOUND || p < query.spanOffset || p - query.spanOffset >= query.spanSize ) return false;
        ( front ? from : to ) = p + 1;
    }
    if ( to < from ) return false;
    *src = from;
    *size = to - from;
    return true;
}

/* ------------------------------------------------------------------------------------------------ line numbers
 * The inverse of line_starts (mi355x_bz2_reader_line_numbers): L(p) = the number of nl bytes in D[0 : min( p, size )],
 * i.e. the 0-based line that holds byte p, and N for every p at or behind the size.  The index gives lines[b] for the
 * block b that holds p; what is missing is the number of nl bytes in [the block's first byte, p): a rank query, answered
 * by k_rank_byte in the decoded block.
 *
 *   launches  planRanges' launches for the blocks that hold a queried offset, each block once, in file order: planRanges
 *             is called with the 1-byte ranges (p, 1), and the one piece of such a range is the launch and the position
 *             of p in that launch's output.
 *   queries   one per distinct {block, offset in block}, sorted by block and position; and behind the queries of every
 *             block one at the end of its span, whose rank must be the count the index gives the block (`expected`): an
 *             imported index that does not fit the data is found out without another kernel.
 *   answers   per input, in caller order: L(p) = fixed, plus the rank of `query` if there is one.  No query for the
 *             first byte of a block (lines[b]), an offset at or behind the size (N), or an empty file (0).
 */
struct RankQuery
{
    uint32_t launch{ 0 };
    uint64_t spanOffset{ 0 }, spanSize{ 0 };   /* the block in the launch's output */
    uint64_t position{ 0 };                    /* in the launch's output: spanOffset <= position <= spanOffset + spanSize */
    uint64_t blockStart{ 0 };                  /* decoded offset of the block's first byte */
    uint64_t expected{ NOT_FOUND };            /* set (end of the span): the delimiters the index gives the block */
};

struct LineNumber
{
    uint64_t fixed{ 0 };
    uint32_t query{ NO_QUERY };
};

struct LineNumberPlan
{
    std::vector<RangeLaunch> launches;
    std::vector<RankQuery> queries;
    std::vector<LineNumber> answers;
    size_t distinctBlocks{ 0 };
};

/** map, lineBytes / lineLines / nIndex, cap, packed, fileBytes: as planLines.  offsets: in caller order, any order. */
inline LineNumberPlan
planLineNumbers( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* lineBytes, const uint64_t* lineLines,
                 size_t nIndex, const uint64_t* offsets, size_t n, size_t cap, bool packed, uint64_t fileBytes )
{
    checkLineIndex( map, lineBytes, lineLines, nIndex );
    std::vector<uint64_t> starts, lengths;
    dataBlocksOf( map, starts, lengths );
    const size_t B = starts.size();
    const uint64_t total = map.empty() ? 0 : map.back().second;
    const uint64_t N = lineLines[B];

    LineNumberPlan plan;
    plan.answers.assign( n, {} );
    std::vector<uint64_t> sizes( n, 0 );       /* 1: the offset needs a query */
    std::vector<size_t> asking;
    for ( size_t i = 0; i < n; ++i ) {
        if ( offsets[i] >= total ) {
            plan.answers[i].fixed = N;
            continue;
        }
        const size_t b = static_cast<size_t>( std::upper_bound( starts.begin(), starts.end(), offsets[i] ) - starts.begin() ) - 1;
        plan.answers[i].fixed = lineLines[b];
        if ( offsets[i] == starts[b] ) continue;
        sizes[i] = 1;
        asking.push_back( i );
    }
    if ( asking.size() >= NO_QUERY / 2 ) throw std::invalid_argument( "planLineNumbers: too many offsets for one call" );
    auto cover = planRanges( map, offsets, sizes.data(), n, cap, packed, fileBytes );
    plan.launches = std::move( cover.launches );
    plan.distinctBlocks = cover.distinctBlocks;
    if ( cover.pieces.size() != asking.size() ) throw std::logic_error( "planLineNumbers: an offset without its piece" );

    /* piece k belongs to asking[k] (both in caller order); the queries in file order, one per distinct offset */
    std::vector<size_t> order( asking.size() );
    for ( size_t k = 0; k < order.size(); ++k ) order[k] = k;
    /* (grep hands over the search's positions, which are ascending already: then there is nothing to sort) */
    const auto before = [&] ( size_t a, size_t b ) { return offsets[asking[a]] < offsets[asking[b]]; };
    if ( !std::is_sorted( order.begin(), order.end(), before ) ) std::sort( order.begin(), order.end(), before );
    size_t block = B;   /* of the queries being added */
    const auto closeBlock = [&] () {
        if ( block == B ) return;
        auto end = plan.queries.back();
        end.position = end.spanOffset + end.spanSize;
        end.expected = lineLines[block + 1] - lineLines[block];
        plan.queries.push_back( end );
    };
    for ( size_t j = 0; j < order.size(); ++j ) {
        const size_t i = asking[order[j]];
        if ( j > 0 && offsets[i] == offsets[asking[order[j - 1]]] ) {
            plan.answers[i].query = plan.answers[asking[order[j - 1]]].query;
            continue;
        }
        const auto& piece = cover.pieces[order[j]];
        const size_t b = static_cast<size_t>( std::upper_bound( starts.begin(), starts.end(), offsets[i] ) - starts.begin() ) - 1;
        if ( b != block ) {
            closeBlock();
            block = b;
        }
        plan.answers[i].query = (uint32_t)plan.queries.size();
        plan.queries.push_back( { piece.launch, piece.src - ( offsets[i] - starts[b] ), lengths[b], piece.src, starts[b], NOT_FOUND } );
    }
    closeBlock();
    return plan;
}

/** L(p) of an answer, once the ranks of the plan's queries are known. */
inline uint64_t
lineNumberOf( const LineNumber& answer, const uint64_t* ranks )
{
    return answer.fixed + ( answer.query == NO_QUERY ? 0 : ranks[answer.query] );
}
}  // namespace bz2gpu
