/**
 * bz2_fieldnum.hpp -- field j of every line of the decoded file as a number (mi355x_bz2_reader_field_numbers,
 * _field_sums): the definition, the summary of a stretch of bytes, and the rule that stitches the summaries of stretches
 * that lie back to back.  Host code only, no HIP: the reader and the context call it, and tests/native/fieldnum_cases.cpp
 * pins it on the CPU.  The fields are those of bz2_fields.hpp and the block plan is planLineHashes as it is.
 *
 * The definition.  The bytes b of a field are a NUMBER iff they match [+-]?[0-9]{1,18} from end to end; the value is the
 * decimal integer they spell.  No whitespace, no '_', no hex, no floats; leading zeros count towards the 18 digits; "-0"
 * is 0; the empty field, "+", "-" and 19 or more digits are no numbers.  This is not awk's strtod and not Python's int():
 * both accept more.  18 digits always fit int64, so nothing overflows, and a number has at most 19 bytes.  Per line one
 * int64 word: the value; FIELD_NOT_A_NUMBER = -2^63 where the field is present and no number; FIELD_NUMBER_MISSING =
 * -2^63 + 1 where the line has fewer than j + 1 fields.  No value takes either.
 *
 * What a stretch knows: its FieldSummary, and as a FieldText -- the first 19 bytes of a byte string and its size,
 * saturated at 20: all that the definition can ask of it --
 *     headTexts[k]    k <= headDelims, at most j + 1 of them: the bytes between head position k - 1 (or the stretch's
 *                     start) and head position k (or firstNl, or the stretch's end);
 *     tailText        field j of the line that starts at tailStart as far as the stretch reaches: from tailFieldStart to
 *                     tailFieldEnd or to the stretch's end, empty where the field's start is not reached;
 *     numbers         of the lines it closes, the first computed as if the stretch were entered at a line start.
 * The carry of an open line is its FieldCarry and the FieldText of field j so far.  Across a seam a carry with d dl bytes
 * whose field has not ended takes headTexts[j - d] behind its text, if the head has that many: for d = j that continues
 * the field, for d < j it begins it.  Where the line is closed, the number is parseFieldNumber of the text.  The text is
 * preferred to an arithmetic carry (value, digits, sign, validity): it is 20 bytes, it is exact, and the one definition
 * is applied to it, on the host.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "bz2_fields.hpp"

namespace bz2gpu
{
constexpr int64_t FIELD_NOT_A_NUMBER = INT64_MIN;
constexpr int64_t FIELD_NUMBER_MISSING = INT64_MIN + 1;
constexpr uint32_t FIELD_NUMBER_DIGITS = 18;
constexpr uint32_t FIELD_NUMBER_BYTES = 19;      /* a sign and 18 digits */
constexpr uint32_t FIELD_TEXT_LONG = 20;         /* the size of a FieldText that is too long to be a number */

/** The definition: the value of the `size` bytes at `bytes`, or FIELD_NOT_A_NUMBER. */
[[nodiscard]] inline int64_t
parseFieldNumber( const uint8_t* bytes, uint64_t size )
{
    if ( size == 0 || size > FIELD_NUMBER_BYTES ) return FIELD_NOT_A_NUMBER;
    const bool negative = bytes[0] == '-', sign = negative || bytes[0] == '+';
    const uint64_t digits = size - ( sign ? 1 : 0 );
    if ( digits == 0 || digits > FIELD_NUMBER_DIGITS ) return FIELD_NOT_A_NUMBER;
    int64_t value = 0;
    for ( uint64_t i = sign ? 1 : 0; i < size; ++i ) {
        if ( bytes[i] < '0' || bytes[i] > '9' ) return FIELD_NOT_A_NUMBER;
        value = value * 10 + ( bytes[i] - '0' );
    }
    return negative ? -value : value;
}

/** The first 19 bytes of a byte string and its size, saturated at 20; the bytes behind `size` are 0. */
struct FieldText
{
    uint8_t size{ 0 };
    uint8_t bytes[FIELD_NUMBER_BYTES]{};

    void
    append( uint8_t b )
    {
        if ( size < FIELD_NUMBER_BYTES ) bytes[size] = b;
        if ( size < FIELD_TEXT_LONG ) ++size;
    }

    [[nodiscard]] bool operator==( const FieldText& o ) const { return size == o.size && std::memcmp( bytes, o.bytes, sizeof( bytes ) ) == 0; }
    [[nodiscard]] bool operator!=( const FieldText& o ) const { return !( *this == o ); }
};
static_assert( sizeof( FieldText ) == 20, "mi355x_bz2_field_text" );

/** The text of at most `size` bytes at `bytes`. */
[[nodiscard]] inline FieldText
fieldText( const uint8_t* bytes, uint64_t size )
{
    FieldText text;
    for ( uint64_t i = 0; i < std::min<uint64_t>( size, FIELD_NUMBER_BYTES ); ++i ) text.bytes[i] = bytes[i];
    text.size = (uint8_t)std::min<uint64_t>( size, FIELD_TEXT_LONG );
    return text;
}

/** `first` followed by `second`: the size saturates. */
[[nodiscard]] inline FieldText
followedBy( FieldText first, const FieldText& second )
{
    for ( uint32_t i = 0; i < std::min<uint32_t>( second.size, FIELD_NUMBER_BYTES ); ++i ) first.append( second.bytes[i] );
    if ( second.size >= FIELD_TEXT_LONG ) first.size = FIELD_TEXT_LONG;
    return first;
}

/** The number a text spells. */
[[nodiscard]] inline int64_t
parseFieldNumber( const FieldText& text )
{
    return parseFieldNumber( text.bytes, text.size );
}

/** The number of field j of one line's content, by the definition: split, then parse. */
[[nodiscard]] inline int64_t
fieldNumber( const uint8_t* content, size_t size, uint8_t dl, uint32_t j )
{
    size_t at = 0;
    for ( uint32_t k = 0; k < j; ++k ) {
        while ( at < size && content[at] != dl ) ++at;
        if ( at == size ) return FIELD_NUMBER_MISSING;
        ++at;
    }
    size_t end = at;
    while ( end < size && content[end] != dl ) ++end;
    return parseFieldNumber( content + at, end - at );
}

/** An open line: its FieldCarry and the text of field j so far. */
struct FieldNumberCarry
{
    FieldCarry field;
    FieldText text;
};

/** The number of texts a head with n dl bytes (saturated at j + 1) lists. */
[[nodiscard]] inline uint32_t
headTextCount( uint32_t n, uint32_t j )
{
    return std::min( n + 1, j + 1 );
}

/** The carry over the head of a stretch at `offset`: n head positions and headTextCount( n, j ) head texts. */
inline void
fieldNumberContinue( FieldNumberCarry& carry, uint32_t j, const uint64_t* positions, const FieldText* texts, uint32_t n, uint64_t offset )
{
    const uint32_t d = carry.field.delims;
    if ( carry.field.end == FIELD_UNKNOWN && d <= j && j - d < headTextCount( n, j ) ) carry.text = followedBy( carry.text, texts[j - d] );
    fieldContinue( carry.field, j, positions, n, offset );
}

/** The open line closed at `at`: *field receives where the field lies. */
[[nodiscard]] inline int64_t
fieldNumberClose( const FieldNumberCarry& carry, uint64_t at, FieldSpan* field )
{
    *field = fieldClose( carry.field, at );
    if ( field->size < 0 ) return FIELD_NUMBER_MISSING;
    return (uint64_t)field->size > FIELD_NUMBER_BYTES ? FIELD_NOT_A_NUMBER : parseFieldNumber( carry.text );
}

/** The summary of a stretch for field j (the header says what the members mean).  fields.count is the number of lines the
 * stretch closes, whether or not `numbers`, fields.starts and fields.sizes list them all. */
struct FieldNumberSummary
{
    FieldSummary fields;
    std::vector<FieldText> headTexts;
    FieldText tailText;
    std::vector<int64_t> numbers;

    [[nodiscard]] FieldNumberCarry tailCarry() const { return { fields.tail(), tailText }; }
};

[[nodiscard]] inline FieldNumberSummary
emptyFieldNumberSummary( uint32_t j )
{
    FieldNumberSummary s;
    s.fields = emptyFieldSummary( j );
    s.headTexts.resize( 1 );
    return s;
}

/** The summary of one chunk, as a lane that enters it at a line start walks it. */
inline FieldNumberSummary
summariseFieldNumberChunk( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j )
{
    FieldNumberSummary s = emptyFieldNumberSummary( j );
    s.fields = summariseFieldChunk( bytes, size, nl, dl, j );
    FieldNumberCarry carry{ fieldLineStart( j, 0 ), {} };
    bool inHead = true;
    size_t segment = 0;      /* of the head: the dl bytes passed in front of the first nl, saturated at j + 1 */
    for ( size_t at = 0; at < size; ++at ) {
        const uint8_t b = bytes[at];
        if ( b == nl ) {
            FieldSpan field;
            s.numbers.push_back( fieldNumberClose( carry, at, &field ) );
            inHead = false;
            carry = { fieldLineStart( j, at + 1 ), {} };
        } else if ( b == dl ) {
            if ( inHead && segment <= j ) {
                ++segment;
                if ( segment <= j ) s.headTexts.emplace_back();
            }
            const uint64_t position = at;
            if ( carry.field.delims <= j ) fieldContinue( carry.field, j, &position, 1, 0 );
        } else {
            if ( inHead && segment < s.headTexts.size() ) s.headTexts[segment].append( b );
            if ( carry.field.start != FIELD_UNKNOWN && carry.field.end == FIELD_UNKNOWN ) carry.text.append( b );
        }
    }
    s.tailText = carry.text;
    return s;
}

/** `all` followed by `part`, both for field j and with all their lines listed: the rule of the header between two
 * stretches. */
inline void
appendFieldNumberSummary( FieldNumberSummary& all, const FieldNumberSummary& part, uint32_t j )
{
    const auto& g = part.fields;
    const uint64_t offset = all.fields.size;
    FieldNumberCarry carry = all.tailCarry();
    if ( !all.fields.hasDelimiter && !part.headTexts.empty() ) {
        /* the last text is open unless the ( j + 1 )-th dl closed it */
        if ( all.headTexts.size() == (size_t)all.fields.headDelims() + 1 ) {
            all.headTexts.back() = followedBy( all.headTexts.back(), part.headTexts.front() );
            for ( size_t i = 1; i < part.headTexts.size() && all.headTexts.size() <= j; ++i ) all.headTexts.push_back( part.headTexts[i] );
        }
    }
    fieldNumberContinue( carry, j, g.headPositions.data(), part.headTexts.data(), g.headDelims(), offset );
    if ( g.hasDelimiter ) {
        FieldSpan field;
        all.numbers.push_back( fieldNumberClose( carry, offset + g.firstNl, &field ) );
        all.numbers.insert( all.numbers.end(), part.numbers.begin() + 1, part.numbers.end() );
        all.tailText = part.tailText;
    } else {
        all.tailText = carry.text;
    }
    appendFieldSummary( all.fields, g, j );
}

/** The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as the kernels compose them.  The result
 * does not depend on `chunk`. */
inline FieldNumberSummary
summariseFieldNumbers( const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j, size_t chunk )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summariseFieldNumbers: the chunk size must not be 0" );
    FieldNumberSummary all = emptyFieldNumberSummary( j );
    for ( size_t at = 0; at < size; at += chunk ) {
        appendFieldNumberSummary( all, summariseFieldNumberChunk( bytes + at, std::min( chunk, size - at ), nl, dl, j ), j );
    }
    return all;
}

/** A stretch of D for stitchFieldNumbers: where it lies and its summary, whose fields.size is the stretch's.  The summary
 * may list fewer lines than fields.count, or none. */
struct FieldNumberStretch
{
    uint64_t fileOffset{ 0 };
    FieldNumberSummary summary;
};

/** What stitchFieldNumbers found: the number of lines the stretches close, and the unterminated tail behind them. */
struct StitchedFieldNumbers
{
    uint64_t closed{ 0 };
    bool hasTail{ false };
    int64_t tailNumber{ FIELD_NUMBER_MISSING };
    FieldSpan tail;
};

/**
 * The rule of the header over stretches that lie back to back (checked: std::invalid_argument) from the offset of the
 * first one, which must be a line's start.  The closed lines are numbered from 0 in the order the stretches close them.
 * patch( k, number, field ) is called for every closed line k that began in front of the stretch that closes it, with its
 * number and its field in D; every other line has the number its stretch lists and the field it lists, moved by the
 * stretch's offset.
 */
template<typename Patch>
inline StitchedFieldNumbers
stitchFieldNumbers( const std::vector<FieldNumberStretch>& stretches, uint32_t j, const Patch& patch )
{
    StitchedFieldNumbers result;
    uint64_t end = stretches.empty() ? 0 : stretches.front().fileOffset;
    FieldNumberCarry carry{ fieldLineStart( j, end ), {} };
    bool carryNonEmpty = false;
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        const auto& s = stretch.summary;
        const auto& f = s.fields;
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchFieldNumbers: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        if ( f.size > ~uint64_t( 0 ) - end ) throw std::invalid_argument( "stitchFieldNumbers: the stretches overflow 64 bits" );
        const uint64_t offset = end;
        end += f.size;
        if ( f.size == 0 ) continue;
        if ( f.headDelims() > j + 1 ) throw std::invalid_argument( "stitchFieldNumbers: a stretch lists too many head positions" );
        if ( s.headTexts.size() != headTextCount( f.headDelims(), j ) ) {
            throw std::invalid_argument( "stitchFieldNumbers: a stretch does not list the texts of its head" );
        }
        fieldNumberContinue( carry, j, f.headPositions.data(), s.headTexts.data(), f.headDelims(), offset );
        if ( f.hasDelimiter ) {
            if ( f.count == 0 || f.firstNl >= f.size ) throw std::invalid_argument( "stitchFieldNumbers: a stretch with a delimiter closes no line" );
            if ( carryNonEmpty ) {
                FieldSpan field;
                const int64_t number = fieldNumberClose( carry, offset + f.firstNl, &field );
                patch( result.closed, number, field );
            }
            result.closed += f.count;
            carry = { { f.tailDelims, f.tailFieldStart == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + f.tailFieldStart,
                        f.tailFieldEnd == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + f.tailFieldEnd },
                      s.tailText };
            carryNonEmpty = f.tailNonEmpty;
        } else {
            carryNonEmpty = true;
        }
    }
    result.hasTail = carryNonEmpty;
    if ( carryNonEmpty ) result.tailNumber = fieldNumberClose( carry, end, &result.tail );
    return result;
}

/** A line's number and where its field lies. */
struct FieldNumber
{
    int64_t number{ FIELD_NUMBER_MISSING };
    FieldSpan field;

    [[nodiscard]] bool operator==( const FieldNumber& o ) const { return number == o.number && field == o.field; }
};

/** stitchFieldNumbers into one list: every closed line's number and field, then the tail's if there is one.  Every
 * stretch must list all its lines. */
inline std::vector<FieldNumber>
stitchedFieldNumbers( const std::vector<FieldNumberStretch>& stretches, uint32_t j )
{
    std::vector<FieldNumber> numbers;
    for ( const auto& stretch : stretches ) {
        const auto& s = stretch.summary;
        if ( s.numbers.size() != s.fields.count || s.fields.starts.size() != s.fields.count || s.fields.sizes.size() != s.fields.count ) {
            throw std::invalid_argument( "stitchedFieldNumbers: a stretch does not list all its lines" );
        }
        for ( size_t i = 0; i < s.numbers.size(); ++i ) {
            numbers.push_back( { s.numbers[i], { stretch.fileOffset + s.fields.starts[i], s.fields.sizes[i] } } );
        }
    }
    const auto stitched = stitchFieldNumbers( stretches, j, [&] ( uint64_t k, int64_t number, const FieldSpan& field ) {
        numbers[(size_t)k] = { number, field };
    } );
    if ( stitched.hasTail ) numbers.push_back( { stitched.tailNumber, stitched.tail } );
    return numbers;
}
}  // namespace bz2gpu
