/**
 * bz2_fields.hpp -- where field j of every line of the decoded file lies (mi355x_bz2_reader_field_spans): the definition,
 * the summary of a stretch of bytes for field j, the rule that composes the summaries of stretches that lie back to back,
 * and the plan of the blocks a range of lines needs.  Host code only, no HIP: the reader and the context call it, and
 * tests/native/fields_cases.cpp pins it on the CPU.
 *
 * The definition.  D = the decoded file, nl = the one byte between lines, dl = the one byte between fields, dl != nl.
 * Lines are numbered as line_hashes numbers them: line k is closed by the k-th nl, counted from 0; a non-empty
 * unterminated tail is one more line, an empty one is none.  C = a line's content, without its nl, s = the offset of its
 * first byte in D.  parts = C.split( dl ), as Python's bytes.split splits: the empty content has one field, the empty one.
 * Field j, counted from 0, is present iff j < len( parts ); then
 *     start = s + sum( len( p ) + 1 for p in parts[:j] ),  size = len( parts[j] ).
 * A missing field has start = s + len( C ) -- the offset of the closing nl, or of the end of D for the tail -- and
 * size = -1.  0 <= j <= FIELD_MAX = 1023.  There is no quoting and no escaping: this is cut -f / awk -F / bytes.split, not
 * a CSV parser.
 *
 * What a stretch knows.  A line that is open where a stretch begins brings a carry: the dl bytes it has passed, saturated
 * at j + 1 (more never matter), where its field j starts if that is reached, and where it ends if that is reached.  Field
 * j starts behind the j-th dl (at the line's start for j = 0) and ends at the ( j + 1 )-th dl or at the nl.  So the summary
 * of a stretch S, all positions relative to S:
 *     size;  hasDelimiter  S holds an nl;  count  the lines S closes;
 *     firstNl        the first nl (UNKNOWN without one);
 *     headPositions  the first min( j + 1, their number ) dl bytes in front of firstNl, in all of S without an nl;
 *                    headDelims is their number;
 *     tailStart      the byte behind the last nl, 0 without one;
 *     tailDelims     the dl bytes from tailStart on, saturated at j + 1;
 *     tailFieldStart, tailFieldEnd   of the line that starts at tailStart, UNKNOWN where S does not reach them;
 *     tailNonEmpty   S is not empty and its last byte is not nl;
 *     starts, sizes  of field j in the lines S closes, in order, the first computed as if S were entered at a line start.
 * Stitching S_0, S_1, ... that lie back to back, the carry starting as that of a line start: the head of S_i continues
 * the carry (its ( j - d )-th dl starts the field of a carry with d < j delimiters, its ( j + 1 - d )-th ends it); with
 * an nl the first closed line of S_i is the carry closed at firstNl and the carry becomes S_i's tail; without one the
 * carry goes on.  At the end of D a carry over at least one byte is the unterminated tail.  The count alone composes as
 * ( resets, delims ) . ( resets', delims' ) = resets' ? ( 1, delims' ) : ( resets, delims + delims' ) with the sum
 * saturated at j + 1, which is associative: the kernels scan it (bz2_fields.hip.h).  One rule serves between the chunks
 * of a tile and the tiles of a span (summarise here), and between the launches of a file (stitchFields).
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bz2_linehash.hpp"

namespace bz2gpu
{
constexpr uint32_t FIELD_MAX = 1023;
constexpr uint32_t FIELD_CHUNK_BYTES = 256;     /* of the kernels, for mi355x_bz2_field_chunk_bytes */
constexpr uint64_t FIELD_UNKNOWN = ~uint64_t( 0 );

/** Why ( nl, dl, field ) cannot be served; empty if it can. */
[[nodiscard]] inline std::string
fieldArgumentsError( uint8_t nl, uint8_t dl, uint64_t field )
{
    if ( field > FIELD_MAX ) return "the field number must be at most " + std::to_string( FIELD_MAX );
    if ( nl == dl ) return "the field delimiter must differ from the line delimiter";
    return {};
}

/** Field j of one line: `size` -1 says it is missing, and `start` is then where the line's content ends. */
struct FieldSpan
{
    uint64_t start{ 0 };
    int64_t size{ -1 };

    [[nodiscard]] bool operator==( const FieldSpan& o ) const { return start == o.start && size == o.size; }
};

/** An open line: the dl bytes passed, saturated at j + 1, and field j's start and end where they are reached. */
struct FieldCarry
{
    uint32_t delims{ 0 };
    uint64_t start{ FIELD_UNKNOWN }, end{ FIELD_UNKNOWN };
};

/** The carry of a line that starts at `at`. */
[[nodiscard]] inline FieldCarry
fieldLineStart( uint32_t j, uint64_t at )
{
    return { 0, j == 0 ? at : FIELD_UNKNOWN, FIELD_UNKNOWN };
}

/** The carry behind `n` more dl bytes at positions[0, n) + offset; n is saturated at j + 1 by whoever counted. */
inline void
fieldContinue( FieldCarry& carry, uint32_t j, const uint64_t* positions, uint32_t n, uint64_t offset )
{
    const uint32_t d = carry.delims;
    /* an unknown start says d < j, an unknown end d <= j: checked, since summaries come from outside too */
    if ( carry.start == FIELD_UNKNOWN && d < j && d + n >= j ) carry.start = offset + positions[j - d - 1] + 1;
    if ( carry.end == FIELD_UNKNOWN && d <= j && d + n >= j + 1 ) carry.end = offset + positions[j - d];
    carry.delims = std::min( d + n, j + 1 );
}

/** The open line closed by an nl, or by the end of D, at `at`. */
[[nodiscard]] inline FieldSpan
fieldClose( const FieldCarry& carry, uint64_t at )
{
    if ( carry.start == FIELD_UNKNOWN ) return { at, -1 };
    return { carry.start, (int64_t)( ( carry.end != FIELD_UNKNOWN ? carry.end : at ) - carry.start ) };
}

/** The summary of a stretch for field j (the header says what the members mean).  `count` is the number of lines the
 * stretch closes, whether or not `starts` and `sizes` list them all. */
struct FieldSummary
{
    uint64_t size{ 0 };
    bool hasDelimiter{ false }, tailNonEmpty{ false };
    uint64_t count{ 0 };
    uint64_t firstNl{ FIELD_UNKNOWN };
    std::vector<uint64_t> headPositions;
    uint64_t tailStart{ 0 };
    uint32_t tailDelims{ 0 };
    uint64_t tailFieldStart{ FIELD_UNKNOWN }, tailFieldEnd{ FIELD_UNKNOWN };
    std::vector<uint64_t> starts;
    std::vector<int64_t> sizes;

    [[nodiscard]] uint32_t headDelims() const { return (uint32_t)headPositions.size(); }
    [[nodiscard]] FieldCarry tail() const { return { tailDelims, tailFieldStart, tailFieldEnd }; }

    void
    setTail( const FieldCarry& carry )
    {
        tailDelims = carry.delims;
        tailFieldStart = carry.start;
        tailFieldEnd = carry.end;
    }
};

/** The summary of no bytes at all. */
[[nodiscard]] inline FieldSummary
emptyFieldSummary( uint32_t j )
{
    FieldSummary s;
    s.setTail( fieldLineStart( j, 0 ) );
    return s;
}

/** The summary of one chunk, as a lane that enters it at a line start walks it. */
inline FieldSummary
summariseFieldChunk( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j )
{
    FieldSummary s = emptyFieldSummary( j );
    s.size = size;
    FieldCarry carry = s.tail();
    for ( size_t at = 0; at < size; ++at ) {
        if ( bytes[at] == nl ) {
            const auto field = fieldClose( carry, at );
            s.starts.push_back( field.start );
            s.sizes.push_back( field.size );
            if ( !s.hasDelimiter ) s.firstNl = at;
            s.hasDelimiter = true;
            s.tailStart = at + 1;
            carry = fieldLineStart( j, at + 1 );
        } else if ( bytes[at] == dl ) {
            const uint64_t position = at;
            if ( !s.hasDelimiter && s.headPositions.size() <= j ) s.headPositions.push_back( position );
            if ( carry.delims <= j ) fieldContinue( carry, j, &position, 1, 0 );
        }
    }
    s.setTail( carry );
    s.tailNonEmpty = size > 0 && bytes[size - 1] != nl;
    s.count = s.starts.size();
    return s;
}

/** `all` followed by `part`, both for field j and with all their lines listed: the rule of the header between two
 * stretches. */
inline void
appendFieldSummary( FieldSummary& all, const FieldSummary& part, uint32_t j )
{
    const uint64_t offset = all.size;
    FieldCarry carry = all.tail();
    fieldContinue( carry, j, part.headPositions.data(), part.headDelims(), offset );
    if ( !all.hasDelimiter ) {
        for ( size_t i = 0; i < part.headPositions.size() && all.headPositions.size() <= j; ++i ) {
            all.headPositions.push_back( offset + part.headPositions[i] );
        }
    }
    const auto shifted = [offset] ( uint64_t position ) { return position == FIELD_UNKNOWN ? position : offset + position; };
    if ( part.hasDelimiter ) {
        const auto field = fieldClose( carry, offset + part.firstNl );
        all.starts.push_back( field.start );
        all.sizes.push_back( field.size );
        for ( size_t i = 1; i < part.starts.size(); ++i ) {
            all.starts.push_back( offset + part.starts[i] );
            all.sizes.push_back( part.sizes[i] );
        }
        if ( !all.hasDelimiter ) all.firstNl = offset + part.firstNl;
        all.hasDelimiter = true;
        all.tailStart = offset + part.tailStart;
        all.setTail( { part.tailDelims, shifted( part.tailFieldStart ), shifted( part.tailFieldEnd ) } );
        all.tailNonEmpty = part.tailNonEmpty;
    } else {
        all.setTail( carry );
        /* a part without an nl is empty or ends in a byte of its head */
        all.tailNonEmpty = all.tailNonEmpty || part.tailNonEmpty;
    }
    all.size += part.size;
    all.count = all.starts.size();
}

/** The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as the kernels compose them.  The result
 * does not depend on `chunk`. */
inline FieldSummary
summariseFields( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j, size_t chunk )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summariseFields: the chunk size must not be 0" );
    FieldSummary all = emptyFieldSummary( j );
    for ( size_t at = 0; at < size; at += chunk ) {
        appendFieldSummary( all, summariseFieldChunk( bytes + at, std::min( chunk, size - at ), nl, dl, j ), j );
    }
    return all;
}

/** A stretch of D for stitchFields: where it lies and its summary, whose size is the stretch's.  The summary may list
 * fewer lines than summary.count, or none: the reader's launches write theirs to device memory and report the count. */
struct FieldStretch
{
    uint64_t fileOffset{ 0 };
    FieldSummary summary;
};

/** What stitchFields found: the number of lines the stretches close, and the unterminated tail behind them. */
struct StitchedFields
{
    uint64_t closed{ 0 };
    bool hasTail{ false };
    FieldSpan tail;
};

/**
 * The rule of the header over stretches that lie back to back (checked: std::invalid_argument) from the offset of the
 * first one, which must be a line's start: offset 0 or the byte behind an nl.  The closed lines are numbered from 0 in
 * the order the stretches close them.  patch( k, field ) is called for every closed line k that began in front of the
 * stretch that closes it -- the first closed line of a stretch entered by a non-empty carry -- with its field in D;
 * every other line has the field its stretch lists, moved by the stretch's offset.
 */
template<typename Patch>
inline StitchedFields
stitchFields( const std::vector<FieldStretch>& stretches, uint32_t j, const Patch& patch )
{
    StitchedFields result;
    uint64_t end = stretches.empty() ? 0 : stretches.front().fileOffset;
    FieldCarry carry = fieldLineStart( j, end );
    bool carryNonEmpty = false;
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        const auto& s = stretch.summary;
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchFields: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        if ( s.size > ~uint64_t( 0 ) - end ) throw std::invalid_argument( "stitchFields: the stretches overflow 64 bits" );
        const uint64_t offset = end;
        end += s.size;
        if ( s.size == 0 ) continue;
        if ( s.headDelims() > j + 1 ) throw std::invalid_argument( "stitchFields: a stretch lists too many head positions" );
        fieldContinue( carry, j, s.headPositions.data(), s.headDelims(), offset );
        if ( s.hasDelimiter ) {
            if ( s.count == 0 || s.firstNl >= s.size ) throw std::invalid_argument( "stitchFields: a stretch with a delimiter closes no line" );
            if ( carryNonEmpty ) patch( result.closed, fieldClose( carry, offset + s.firstNl ) );
            result.closed += s.count;
            carry = { s.tailDelims, s.tailFieldStart == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + s.tailFieldStart,
                      s.tailFieldEnd == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + s.tailFieldEnd };
            carryNonEmpty = s.tailNonEmpty;
        } else {
            carryNonEmpty = true;
        }
    }
    result.hasTail = carryNonEmpty;
    if ( carryNonEmpty ) result.tail = fieldClose( carry, end );
    return result;
}

/** stitchFields into one list: every closed line's field, then the tail's if there is one.  Every stretch must list all
 * its lines. */
inline std::vector<FieldSpan>
stitchedFields( const std::vector<FieldStretch>& stretches, uint32_t j )
{
    std::vector<FieldSpan> fields;
    for ( const auto& stretch : stretches ) {
        const auto& s = stretch.summary;
        if ( s.starts.size() != s.count || s.sizes.size() != s.count ) {
            throw std::invalid_argument( "stitchedFields: a stretch does not list all its lines" );
        }
        for ( size_t i = 0; i < s.starts.size(); ++i ) fields.push_back( { stretch.fileOffset + s.starts[i], s.sizes[i] } );
    }
    const auto stitched = stitchFields( stretches, j, [&] ( uint64_t k, const FieldSpan& field ) { fields[(size_t)k] = field; } );
    if ( stitched.hasTail ) fields.push_back( stitched.tail );
    return fields;
}

/** Which blocks the lines [first, first + count) need: the blocks, launches and stretches of planLineHashes, whose
 * comment says how the closed lines of the stitched stretches are numbered. */
using FieldPlan = LineHashPlan;

inline FieldPlan
planFields( const std::vector<std::pair<uint64_t, uint64_t> >& map, const uint64_t* lineBytes, const uint64_t* lineLines,
            size_t nIndex, uint64_t first, uint64_t count, size_t cap, bool packed, uint64_t fileBytes )
{
    return planLineHashes( map, lineBytes, lineLines, nIndex, first, count, cap, packed, fileBytes );
}
}  // namespace bz2gpu
