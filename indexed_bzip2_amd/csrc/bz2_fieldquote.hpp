/**
 * bz2_fieldquote.hpp -- field j of every line when fields may be quoted (the quote= of field_spans, read_fields and
 * read_columns): the definition, the summary of a stretch, and the rule that composes summaries of stretches that lie back
 * to back.  The quoted twin of bz2_fields.hpp, whose structs and functions stay as they are.  Host code only, no HIP:
 * tests/native/fields_quoted_cases.cpp pins it on the CPU.
 *
 * The definition.  D, nl, dl, the lines and their numbers are bz2_fields.hpp's; q is one more byte, q != nl and q != dl.
 * Within a line's content C every q toggles "inside quotes", and C is parted at the dl bytes that lie outside:
 *     parts, inq, s = [], 0, 0
 *     for i, b in enumerate( C ):
 *         if b == q: inq ^= 1
 *         elif b == dl and not inq: parts.append( ( s, i ) ); s = i + 1
 *     parts.append( ( s, len( C ) ) )
 * A doubled quote inside a quoted field toggles twice, so it needs no rule of its own.  An unbalanced quote makes the rest
 * of the line one field; the nl ALWAYS closes the line and resets the state -- a quoted field cannot hold an nl, so lines,
 * their numbers, the line index and planFields are what they were.  The RAW field j is parts[j]; presence and "missing"
 * are bz2_fields.hpp's.  The CONTENT of a raw field of at least 2 bytes whose first and last bytes are both q is the raw
 * field without those two bytes (quotedFieldContent); every other raw field is its own content: "" is the empty field one
 * byte further on, a lone " stays.  Doubled quotes inside stay doubled: spans of the file are returned, no byte is
 * rewritten.
 *
 * What a stretch knows.  A carry is bz2_fields.hpp's plus inQuote.  Whether a dl in front of a stretch's first nl counts
 * depends on the state the stretch is entered with, which the stretch cannot know: so it lists its head positions under
 * BOTH hypotheses, headPositions[0] entered outside quotes and headPositions[1] entered inside, at most j + 1 each, and
 * headQuoteParity, the parity of the q bytes in front of firstNl (of all of them without an nl), which takes the entering
 * state to the one at firstNl.  Behind an nl a line starts outside quotes: the tail members need no hypothesis and are
 * those of a stretch entered outside; tailInQuote is the parity of the q bytes from tailStart on.  starts and sizes list
 * RAW fields, the first closed line as if the stretch were entered at a line start, outside quotes.
 *
 * The count composes as an element ( reset, p, a0, a1 ): reset says the stretch holds an nl, p is the parity of the q
 * bytes behind its last nl (of all without one), a0 / a1 the counted dl bytes behind the last nl when the stretch is
 * entered outside / inside quotes, saturated at j + 1; with reset a1 == a0.  composeQuotedElement is associative: the
 * kernels scan it (bz2_fieldquote.hip.h), 32 bits as the unquoted element is.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "bz2_fields.hpp"

namespace bz2gpu
{
/** Why ( nl, dl, q, field ) cannot be served; empty if it can. */
[[nodiscard]] inline std::string
quotedFieldArgumentsError( uint8_t nl, uint8_t dl, uint8_t q, uint64_t field )
{
    auto why = fieldArgumentsError( nl, dl, field );
    if ( !why.empty() ) return why;
    if ( q == nl ) return "the quote must differ from the line delimiter";
    if ( q == dl ) return "the quote must differ from the field delimiter";
    return {};
}

/** The content of a raw field whose first and last bytes are `first` and `last` (not read for fewer than 2 bytes). */
[[nodiscard]] inline FieldSpan
quotedFieldContent( const FieldSpan& raw, uint8_t first, uint8_t last, uint8_t q )
{
    if ( raw.size >= 2 && first == q && last == q ) return { raw.start + 1, raw.size - 2 };
    return raw;
}

/** An open line: bz2_fields.hpp's carry, and whether the line is inside quotes. */
struct QuotedFieldCarry
{
    FieldCarry fields;
    bool inQuote{ false };
};

/** The carry of a line that starts at `at`: outside quotes. */
[[nodiscard]] inline QuotedFieldCarry
quotedFieldLineStart( uint32_t j, uint64_t at )
{
    return { fieldLineStart( j, at ), false };
}

/** The stretch's scanned element, as the kernels pack it into 32 bits. */
struct QuotedElement
{
    bool reset{ false }, p{ false };
    uint32_t a0{ 0 }, a1{ 0 };

    [[nodiscard]] bool operator==( const QuotedElement& o ) const { return reset == o.reset && p == o.p && a0 == o.a0 && a1 == o.a1; }
};

/** `first` followed by `second`, counts saturated at `cap`. */
[[nodiscard]] inline QuotedElement
composeQuotedElement( const QuotedElement& first, const QuotedElement& second, uint32_t cap )
{
    if ( second.reset ) return second;
    /* the state `second` is entered with when `first` is entered outside ( e0 ) and inside ( e1 ) */
    const bool e0 = first.p, e1 = first.reset ? first.p : !first.p;
    return { first.reset, first.p != second.p, std::min( first.a0 + ( e0 ? second.a1 : second.a0 ), cap ),
             std::min( first.a1 + ( e1 ? second.a1 : second.a0 ), cap ) };
}

/** The element of bytes[0, size) by a walk over its bytes. */
[[nodiscard]] inline QuotedElement
quotedElementOf( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint8_t q, uint32_t cap )
{
    QuotedElement e;
    for ( size_t at = 0; at < size; ++at ) {
        if ( bytes[at] == nl ) {
            e = { true, false, 0, 0 };
        } else if ( bytes[at] == q ) {
            e.p = !e.p;
        } else if ( bytes[at] == dl ) {
            /* entered outside, the state here is p; entered inside it is !p until an nl, and p behind one */
            if ( !e.p ) e.a0 = std::min( e.a0 + 1, cap );
            if ( e.reset ) e.a1 = e.a0;
            else if ( e.p ) e.a1 = std::min( e.a1 + 1, cap );
        }
    }
    return e;
}

/** The summary of a stretch for field j under the quote q (the header says what the members mean). */
struct QuotedFieldSummary
{
    uint64_t size{ 0 };
    bool hasDelimiter{ false }, tailNonEmpty{ false };
    uint64_t count{ 0 };
    uint64_t firstNl{ FIELD_UNKNOWN };
    std::vector<uint64_t> headPositions[2];
    bool headQuoteParity{ false };
    uint64_t tailStart{ 0 };
    uint32_t tailDelims{ 0 };
    uint64_t tailFieldStart{ FIELD_UNKNOWN }, tailFieldEnd{ FIELD_UNKNOWN };
    bool tailInQuote{ false };
    std::vector<uint64_t> starts;
    std::vector<int64_t> sizes;

    [[nodiscard]] uint32_t headDelims( int h ) const { return (uint32_t)headPositions[h].size(); }
    [[nodiscard]] QuotedFieldCarry tail() const { return { { tailDelims, tailFieldStart, tailFieldEnd }, tailInQuote }; }

    void
    setTail( const QuotedFieldCarry& carry )
    {
        tailDelims = carry.fields.delims;
        tailFieldStart = carry.fields.start;
        tailFieldEnd = carry.fields.end;
        tailInQuote = carry.inQuote;
    }
};

/** The carry behind the head of a stretch that lies at `offset`: the list of the state the carry is in, then the parity. */
inline void
quotedFieldContinue( QuotedFieldCarry& carry, uint32_t j, const QuotedFieldSummary& s, uint64_t offset )
{
    const auto& positions = s.headPositions[carry.inQuote ? 1 : 0];
    fieldContinue( carry.fields, j, positions.data(), (uint32_t)positions.size(), offset );
    carry.inQuote = carry.inQuote != s.headQuoteParity;
}

/** The summary of no bytes at all. */
[[nodiscard]] inline QuotedFieldSummary
emptyQuotedFieldSummary( uint32_t j )
{
    QuotedFieldSummary s;
    s.setTail( quotedFieldLineStart( j, 0 ) );
    return s;
}

/** The summary of one chunk, as a lane that enters it at a line start walks it. */
inline QuotedFieldSummary
summariseQuotedFieldChunk( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint8_t q, uint32_t j )
{
    QuotedFieldSummary s = emptyQuotedFieldSummary( j );
    s.size = size;
    QuotedFieldCarry carry = s.tail();
    for ( size_t at = 0; at < size; ++at ) {
        const uint8_t b = bytes[at];
        if ( b == nl ) {
            const auto field = fieldClose( carry.fields, at );
            s.starts.push_back( field.start );
            s.sizes.push_back( field.size );
            if ( !s.hasDelimiter ) s.firstNl = at;
            s.hasDelimiter = true;
            s.tailStart = at + 1;
            carry = quotedFieldLineStart( j, at + 1 );
        } else if ( b == q ) {
            carry.inQuote = !carry.inQuote;
            if ( !s.hasDelimiter ) s.headQuoteParity = !s.headQuoteParity;
        } else if ( b == dl ) {
            const uint64_t position = at;
            /* in front of the first nl a stretch entered inside quotes is in the opposite state */
            auto& head = s.headPositions[carry.inQuote ? 1 : 0];
            if ( !s.hasDelimiter && head.size() <= j ) head.push_back( position );
            if ( !carry.inQuote && carry.fields.delims <= j ) fieldContinue( carry.fields, j, &position, 1, 0 );
        }
    }
    s.setTail( carry );
    s.tailNonEmpty = size > 0 && bytes[size - 1] != nl;
    s.count = s.starts.size();
    return s;
}

/** `all` followed by `part`, both for field j and with all their lines listed. */
inline void
appendQuotedFieldSummary( QuotedFieldSummary& all, const QuotedFieldSummary& part, uint32_t j )
{
    const uint64_t offset = all.size;
    QuotedFieldCarry carry = all.tail();
    quotedFieldContinue( carry, j, part, offset );
    if ( !all.hasDelimiter ) {
        /* `all` entered in state h reaches `part` in state h ^ all.headQuoteParity */
        for ( int h = 0; h < 2; ++h ) {
            const auto& from = part.headPositions[( h != 0 ) != all.headQuoteParity ? 1 : 0];
            auto& to = all.headPositions[h];
            for ( size_t i = 0; i < from.size() && to.size() <= j; ++i ) to.push_back( offset + from[i] );
        }
        all.headQuoteParity = all.headQuoteParity != part.headQuoteParity;
    }
    const auto shifted = [offset] ( uint64_t position ) { return position == FIELD_UNKNOWN ? position : offset + position; };
    if ( part.hasDelimiter ) {
        const auto field = fieldClose( carry.fields, offset + part.firstNl );
        all.starts.push_back( field.start );
        all.sizes.push_back( field.size );
        for ( size_t i = 1; i < part.starts.size(); ++i ) {
            all.starts.push_back( offset + part.starts[i] );
            all.sizes.push_back( part.sizes[i] );
        }
        if ( !all.hasDelimiter ) all.firstNl = offset + part.firstNl;
        all.hasDelimiter = true;
        all.tailStart = offset + part.tailStart;
        all.setTail( { { part.tailDelims, shifted( part.tailFieldStart ), shifted( part.tailFieldEnd ) }, part.tailInQuote } );
        all.tailNonEmpty = part.tailNonEmpty;
    } else {
        all.setTail( carry );
        all.tailNonEmpty = all.tailNonEmpty || part.tailNonEmpty;
    }
    all.size += part.size;
    all.count = all.starts.size();
}

/** The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as the kernels compose them.  The result
 * does not depend on `chunk`. */
inline QuotedFieldSummary
summariseQuotedFields( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint8_t q, uint32_t j, size_t chunk )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summariseQuotedFields: the chunk size must not be 0" );
    QuotedFieldSummary all = emptyQuotedFieldSummary( j );
    for ( size_t at = 0; at < size; at += chunk ) {
        appendQuotedFieldSummary( all, summariseQuotedFieldChunk( bytes + at, std::min( chunk, size - at ), nl, dl, q, j ), j );
    }
    return all;
}

/** A stretch of D for stitchQuotedFields: FieldStretch with a quoted summary. */
struct QuotedFieldStretch
{
    uint64_t fileOffset{ 0 };
    QuotedFieldSummary summary;
};

/**
 * stitchFields for quoted summaries, with its arguments, checks, numbering and result.  patch( k, field ) receives the RAW
 * field of every closed line that began in front of the stretch that closes it, and the result's tail is raw too: whoever
 * has the bytes applies quotedFieldContent.
 */
template<typename Patch>
inline StitchedFields
stitchQuotedFields( const std::vector<QuotedFieldStretch>& stretches, uint32_t j, const Patch& patch )
{
    StitchedFields result;
    uint64_t end = stretches.empty() ? 0 : stretches.front().fileOffset;
    QuotedFieldCarry carry = quotedFieldLineStart( j, end );
    bool carryNonEmpty = false;
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        const auto& s = stretch.summary;
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchQuotedFields: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        if ( s.size > ~uint64_t( 0 ) - end ) throw std::invalid_argument( "stitchQuotedFields: the stretches overflow 64 bits" );
        const uint64_t offset = end;
        end += s.size;
        if ( s.size == 0 ) continue;
        if ( s.headDelims( 0 ) > j + 1 || s.headDelims( 1 ) > j + 1 ) {
            throw std::invalid_argument( "stitchQuotedFields: a stretch lists too many head positions" );
        }
        quotedFieldContinue( carry, j, s, offset );
        if ( s.hasDelimiter ) {
            if ( s.count == 0 || s.firstNl >= s.size ) throw std::invalid_argument( "stitchQuotedFields: a stretch with a delimiter closes no line" );
            if ( carryNonEmpty ) patch( result.closed, fieldClose( carry.fields, offset + s.firstNl ) );
            result.closed += s.count;
            carry = { { s.tailDelims, s.tailFieldStart == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + s.tailFieldStart,
                        s.tailFieldEnd == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + s.tailFieldEnd }, s.tailInQuote };
            carryNonEmpty = s.tailNonEmpty;
        } else {
            carryNonEmpty = true;
        }
    }
    result.hasTail = carryNonEmpty;
    if ( carryNonEmpty ) result.tail = fieldClose( carry.fields, end );
    return result;
}

/** stitchQuotedFields into one list of RAW fields: every closed line's, then the tail's if there is one.  Every stretch
 * must list all its lines. */
inline std::vector<FieldSpan>
stitchedQuotedFields( const std::vector<QuotedFieldStretch>& stretches, uint32_t j )
{
    std::vector<FieldSpan> fields;
    for ( const auto& stretch : stretches ) {
        const auto& s = stretch.summary;
        if ( s.starts.size() != s.count || s.sizes.size() != s.count ) {
            throw std::invalid_argument( "stitchedQuotedFields: a stretch does not list all its lines" );
        }
        for ( size_t i = 0; i < s.starts.size(); ++i ) fields.push_back( { stretch.fileOffset + s.starts[i], s.sizes[i] } );
    }
    const auto stitched = stitchQuotedFields( stretches, j, [&] ( uint64_t k, const FieldSpan& field ) { fields[(size_t)k] = field; } );
    if ( stitched.hasTail ) fields.push_back( stitched.tail );
    return fields;
}
}  // namespace bz2gpu
