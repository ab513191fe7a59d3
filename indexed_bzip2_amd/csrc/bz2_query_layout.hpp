/**
 * bz2_query_layout.hpp -- the arithmetic of the calls that read a finished batch's output (bz2_queries.hip.h): how spans
 * are cut into tiles, and where the lists of one call lie in its staging buffers.  Pure host code, no HIP:
 * tests/native/query_layout_cases.cpp checks the tiler against its definition and every layout against the expressions it
 * replaced.
 *
 * A call has ONE page-locked and ONE device buffer with the same offsets in both: what goes up first ([0, resultsAt) in
 * one H2D), what comes down behind it, and behind that what only the kernels use; the host buffer ends where that
 * begins, the device buffer holds all `bytes`.  The layouts are listed as "up, down; device only", and each lay function
 * adds its regions in the order of its struct's members (a braced list is evaluated left to right).
 */
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace bz2gpu
{
/** f( s, offsetInSpan, length ) for every tile of at most `tileBytes` of the size - m + 1 positions at which a string of m
 * bytes can start inside span s (m = 1: every byte of the span; a span shorter than m has none), spans in order, tiles
 * ascending.  Returns the number of tiles. */
template<typename Span, typename F>
uint64_t
forEachTile( const Span* spans, size_t n, uint64_t tileBytes, uint64_t m, F&& f )
{
    uint64_t count = 0;
    for ( size_t s = 0; s < n; ++s ) {
        if ( spans[s].size < m ) continue;
        const uint64_t starts = spans[s].size - m + 1;
        for ( uint64_t k = 0; k < starts; k += tileBytes, ++count ) f( s, k, std::min( tileBytes, starts - k ) );
    }
    return count;
}

/** first[s]: the number of span s's first tile among forEachTile's; first[n]: how many there are. */
template<typename Span>
std::vector<uint64_t>
firstTiles( const Span* spans, size_t n, uint64_t tileBytes, uint64_t m )
{
    std::vector<uint64_t> first( n + 1, 0 );
    const auto count = [] ( size_t, uint64_t, uint64_t ) {};
    for ( size_t s = 0; s < n; ++s ) first[s + 1] = first[s] + forEachTile( spans + s, 1, tileBytes, m, count );
    return first;
}

/** Regions one behind the other: add returns where the next one starts, at a multiple of `alignment` (a power of two). */
class Regions
{
public:
    uint64_t
    add( uint64_t bytes, uint64_t alignment = 1 )
    {
        const uint64_t at = ( m_size + alignment - 1 ) & ~( alignment - 1 );
        m_size = at + bytes;
        return at;
    }

    [[nodiscard]] uint64_t size() const { return m_size; }

private:
    uint64_t m_size{ 0 };
};

/** sizeof of the records that only device code knows and the kernels' constants, filled in by bz2_queries.hip.h (which
 * pins the values). */
struct QuerySizes
{
    uint64_t countTile, findQuery, rankTile;                              /* bz2_lines.hip.h */
    uint64_t pattern, setTile, setImage;                                  /* SEARCH_MAX_PATTERN, bz2_search_set.hip.h */
    uint64_t chunksPerTile;                                               /* of the three per-line calls */
    uint64_t regexSpan, regexStates;                                      /* bz2_regex.hip.h */
    uint64_t lineHashSpan, lineHashSummary, lineHashTile, lineHashPrefix; /* bz2_linehash.hip.h */
    uint64_t fieldSpan, fieldSummary, fieldTile;                          /* bz2_fields.hip.h */
};

/* count_byte (nQueries = 0, a result per distinct span) and find_byte (a query and a result per query):
 * [tiles][queries] up, [results] down; [tile counts] */
struct SelectLayout { uint64_t tilesAt, queriesAt, resultsAt, countsAt, bytes; };
inline SelectLayout
laySelect( const QuerySizes& s, uint64_t nTiles, uint64_t nQueries, uint64_t nResults )
{
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( nQueries * s.findQuery ), r.add( nResults * 8 ), r.add( nTiles * 4 ), r.size() };
}

/* rank_byte: [tiles][tiles with queries][ends, padded to 8 bytes] up, [ranks] down; [tile counts] */
struct RankLayout { uint64_t tilesAt, workAt, endsAt, resultsAt, countsAt, bytes; };
inline RankLayout
layRank( const QuerySizes& s, uint64_t nTiles, uint64_t nWork, uint64_t nAsked )
{
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( nWork * s.rankTile ), r.add( nAsked * 4 ), r.add( nAsked * 8, 8 ),
             r.add( nTiles * 4 ), r.size() };
}

/* count_bytes / find_bytes: [tiles][pattern] up, [span counts][seam bytes] down; [tile counts][tile places] */
struct SearchLayout { uint64_t tilesAt, patternAt, resultsAt, seamAt, countsAt, placesAt, bytes; };
inline SearchLayout
laySearch( const QuerySizes& s, uint64_t nTiles, uint64_t n )
{
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( s.pattern ), r.add( n * 8 ), r.add( 2 * s.pattern ),
             r.add( nTiles * 4 ), r.add( nTiles * 8, 8 ), r.size() };
}

/* count_bytes_set / find_bytes_set with k patterns: [tiles][set image, 16-byte loads] up,
 * [span counts][pattern counts][seam bytes] down; [tile counts][tile places] */
struct SearchSetLayout { uint64_t tilesAt, imageAt, resultsAt, eachAt, seamAt, countsAt, placesAt, bytes; };
inline SearchSetLayout
laySearchSet( const QuerySizes& s, uint64_t nTiles, uint64_t n, uint64_t k )
{
    Regions r;
    return { r.add( nTiles * s.setTile ), r.add( s.setImage, 16 ), r.add( n * 8 ), r.add( k * 8 ), r.add( 2 * s.pattern ),
             r.add( nTiles * 4 ), r.add( nTiles * 8, 8 ), r.size() };
}

/* match_lines with an automaton of `states` states: [tiles][spans][table, 16-byte loads][accepts] up,
 * [span maps][span info][span counts] down; [chunk maps, 16-byte stores][chunk info][chunk counts][chunk places] */
struct RegexLayout
{
    uint64_t tilesAt, spansAt, tableAt, acceptsAt, resultsAt, spanInfoAt, spanCountsAt, mapsAt, infoAt, countsAt, placesAt, bytes;
};
inline RegexLayout
layRegex( const QuerySizes& s, uint64_t nTiles, uint64_t n, uint64_t states )
{
    const uint64_t slots = nTiles * s.chunksPerTile, mapStride = ( states + 15 ) & ~uint64_t( 15 );
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.regexSpan ), r.add( states * 256, 16 ), r.add( s.regexStates ),
             r.add( n * s.regexStates, 16 ), r.add( n * 4 ), r.add( n * 8, 16 ),
             r.add( slots * mapStride, 16 ), r.add( slots * 4 ), r.add( slots * 4 ), r.add( slots * 8, 16 ), r.size() };
}

/* hash_lines: [tiles][spans] up, [span summaries] down; [tile summaries][chunk prefixes][chunk places][chunk counts] */
struct LineHashLayout { uint64_t tilesAt, spansAt, resultsAt, tileSummariesAt, prefixesAt, placesAt, countsAt, bytes; };
inline LineHashLayout
layLineHash( const QuerySizes& s, uint64_t nTiles, uint64_t n )
{
    const uint64_t slots = nTiles * s.chunksPerTile;
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.lineHashSpan, 16 ), r.add( n * s.lineHashSummary, 16 ),
             r.add( nTiles * s.lineHashTile, 16 ), r.add( slots * s.lineHashPrefix, 16 ), r.add( slots * 8 ), r.add( slots * 4 ),
             r.size() };
}

/* field_spans for field `field`: [tiles][spans] up, [span summaries][head positions, field + 1 per span] down;
 * [tile summaries][chunk places][chunk prefixes][chunk counts] */
struct FieldLayout { uint64_t tilesAt, spansAt, resultsAt, headsAt, tileSummariesAt, placesAt, prefixesAt, countsAt, bytes; };
inline FieldLayout
layFields( const QuerySizes& s, uint64_t nTiles, uint64_t n, uint64_t field )
{
    const uint64_t slots = nTiles * s.chunksPerTile;
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.fieldSpan, 16 ), r.add( n * s.fieldSummary, 16 ),
             r.add( n * ( field + 1 ) * 8, 16 ), r.add( nTiles * s.fieldTile, 16 ), r.add( slots * 8, 16 ), r.add( slots * 4 ),
             r.add( slots * 4 ), r.size() };
}

/* field_spans_quoted for field `field`: field_spans' lists with a summary of `summaryBytes` and the head positions of both
 * entry hypotheses, 2 * ( field + 1 ) per span */
inline FieldLayout
layQuotedFields( const QuerySizes& s, uint64_t summaryBytes, uint64_t nTiles, uint64_t n, uint64_t field )
{
    const uint64_t slots = nTiles * s.chunksPerTile;
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.fieldSpan, 16 ), r.add( n * summaryBytes, 16 ),
             r.add( n * 2 * ( field + 1 ) * 8, 16 ), r.add( nTiles * s.fieldTile, 16 ), r.add( slots * 8, 16 ), r.add( slots * 4 ),
             r.add( slots * 4 ), r.size() };
}

/* field_numbers for field `field`: field_spans' lists, and for k_field_texts where every span lies in the output and the
 * texts of 20 bytes it writes: [tiles][spans][extents, 16 bytes per span] up, [span summaries][head positions, field + 1 per
 * span][head texts, field + 1 per span][tail texts, one per span] down;
 * [tile summaries][chunk places][chunk prefixes][chunk counts] */
struct FieldNumberLayout
{
    uint64_t tilesAt, spansAt, extentsAt, resultsAt, headsAt, headTextsAt, tailTextsAt, tileSummariesAt, placesAt, prefixesAt,
             countsAt, bytes;
};
inline FieldNumberLayout
layFieldNumbers( const QuerySizes& s, uint64_t nTiles, uint64_t n, uint64_t field )
{
    const uint64_t slots = nTiles * s.chunksPerTile;
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.fieldSpan, 16 ), r.add( n * 16, 16 ), r.add( n * s.fieldSummary, 16 ),
             r.add( n * ( field + 1 ) * 8, 16 ), r.add( n * ( field + 1 ) * 20, 16 ), r.add( n * 20, 16 ),
             r.add( nTiles * s.fieldTile, 16 ), r.add( slots * 8, 16 ), r.add( slots * 4 ), r.add( slots * 4 ), r.size() };
}

/* match_fields over lines whose columns are in device memory already, against a value table whose image has `imageBytes`
 * bytes, a multiple of 4 (bz2_fieldmatch.hpp): [image] up, nothing down; nothing for the kernel alone */
struct FieldMatchLayout
{
    uint64_t imageAt, bytes;
};
inline FieldMatchLayout
layFieldMatch( uint64_t imageBytes )
{
    Regions r;
    return { r.add( imageBytes, 16 ), r.size() };
}

/* match_fields_regex over lines whose columns are in device memory already, under an automaton of `states` states
 * (bz2_regex.hpp): [table, 256 bytes per state][acceptsAtEnd, `maxStates` bytes, zero behind the states] up, nothing down;
 * nothing for the kernel alone */
struct FieldRegexLayout
{
    uint64_t tableAt, acceptsAt, bytes;
};
inline FieldRegexLayout
layFieldRegex( uint64_t states, uint64_t maxStates )
{
    Regions r;
    return { r.add( states * 256, 16 ), r.add( maxStates, 16 ), r.size() };
}

/* field_hashes for field `field`: field_spans' and hash_lines' lists side by side, since both first passes run as they
 * are: [tiles][field spans][hash spans] up, [field summaries][hash summaries][tail hashes, 16 bytes per span]
 * [head positions][head hashes, field + 1 per span each] down; [field tile summaries][hash tile summaries][chunk places]
 * [hash prefixes][field prefixes][field counts][hash counts] */
struct FieldHashLayout
{
    uint64_t tilesAt, spansAt, hashSpansAt, resultsAt, hashSummariesAt, tailsAt, headsAt, headHashesAt, tileSummariesAt,
             hashTilesAt, placesAt, hashPrefixesAt, prefixesAt, countsAt, hashCountsAt, bytes;
};
inline FieldHashLayout
layFieldHashes( const QuerySizes& s, uint64_t nTiles, uint64_t n, uint64_t field )
{
    const uint64_t slots = nTiles * s.chunksPerTile;
    Regions r;
    return { r.add( nTiles * s.countTile ), r.add( n * s.fieldSpan, 16 ), r.add( n * s.lineHashSpan, 16 ),
             r.add( n * s.fieldSummary, 16 ), r.add( n * s.lineHashSummary, 16 ), r.add( n * 16, 16 ),
             r.add( n * ( field + 1 ) * 8, 16 ), r.add( n * ( field + 1 ) * 8, 16 ),
             r.add( nTiles * s.fieldTile, 16 ), r.add( nTiles * s.lineHashTile, 16 ), r.add( slots * 8, 16 ),
             r.add( slots * s.lineHashPrefix, 16 ), r.add( slots * 4 ), r.add( slots * 4 ), r.add( slots * 4 ), r.size() };
}

/* gather_fields over n spans that are in device memory already, scanned in tiles of `scanTile` spans: nothing up,
 * [the check: offenders, first offender, total; 24 bytes] down; [tile sums][tile prefixes] */
struct FieldColumnLayout { uint64_t checkAt, tileSumsAt, tilePrefixesAt, bytes, scanTiles; };
inline FieldColumnLayout
layFieldColumn( uint64_t n, uint64_t scanTile )
{
    const uint64_t scanTiles = ( n + scanTile - 1 ) / scanTile;
    Regions r;
    return { r.add( 24 ), r.add( scanTiles * 8, 16 ), r.add( scanTiles * 8, 16 ), r.size(), scanTiles };
}

/** The workgroups of k_field_gather for `total` bytes to a destination whose address is `lead` mod 16: it cuts the
 * destination at multiples of tileBytes counted from the 16-byte boundary in front of it. */
inline uint64_t
fieldGatherTiles( uint64_t total, uint64_t lead, uint64_t tileBytes )
{
    return total == 0 ? 0 : ( lead + total + tileBytes - 1 ) / tileBytes;
}
}  // namespace bz2gpu
