/**
 * bz2_fieldmatch.hpp -- lines selected by the value of a field (mi355x_bz2_reader_field_matches, _field_in_range,
 * _select_lines; Python: where_field, count_where_field, select_lines).  Pure host code, no HIP.
 *
 * The definition.  Lines, fields, dl, nl, first / count and line numbers are field_spans' (bz2_fields.hpp): no quoting, no
 * escaping, this is not a CSV parser.  A predicate on field j is one of two kinds.
 *
 *   VALUES    a set of 1 to FIELDMATCH_MAX_VALUES byte strings of 0 to FIELDMATCH_MAX_VALUE_BYTES bytes each and at most
 *             FIELDMATCH_MAX_BYTES in total.  A line matches iff it has field j and content.split( dl )[j] is byte for
 *             byte one of the values.  The empty value matches an empty field that is present, never a missing one.
 *             Equal values count once.
 *   RANGE     lo <= n <= hi with n = parseFieldNumber( the field's bytes ) (bz2_fieldnum.hpp): a field that is no number
 *             and a line without the field never match.  Bounds are clipped to [-(10^18 - 1), 10^18 - 1], the numbers
 *             there are; lo > hi is the empty range.
 *
 * Inverted, a predicate selects the complement within the line range (grep -v): then also the lines without the field
 * and, for a range, the fields that are no numbers.
 *
 * The key of a field (bz2_fieldhash.hpp: lineHash of its bytes under a seed) is only a FILTER in front of the comparison
 * of the bytes: the answer does not depend on the seed.  The GPU looks a line's key up in a table of the values' keys,
 * sorted ascending, and compares the bytes where the key and the size hit (bz2_fieldmatch.hip.h: k_field_match).  The
 * table holds every key once: two DIFFERENT values with equal keys are refused by buildValueTable, with the advice to pass
 * another seed, so that one probe per line is enough.  A line that crosses a launch seam and the unterminated tail come
 * from stitchFieldHashes as ( key, start, size ) without bytes: where key and size hit the table (candidateValue), the
 * reader fetches the field's bytes and compares them on the host (ValueTable::holds).
 *
 * The image k_field_match reads, for k distinct values:
 *
 *   [0, 8 k)                        the keys, ascending, uint64 each
 *   [8 k, 8 k + 4 ( k + 1 ))        offsets[0 .. k], uint32 each: value i is bytes[offsets[i], offsets[i + 1])
 *   [8 k + 4 ( k + 1 ), ...)        the values' bytes in that order, padded with zeros to a multiple of 4
 *
 * at most FIELDMATCH_IMAGE_MAX bytes.
 */
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <numeric>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bz2_linehash.hpp"

namespace bz2gpu
{
constexpr uint32_t FIELDMATCH_MAX_VALUES = 1024;        /* SET_MAX_PATTERNS */
constexpr uint32_t FIELDMATCH_MAX_VALUE_BYTES = 256;
constexpr uint32_t FIELDMATCH_MAX_BYTES = 16384;        /* SET_MAX_BYTES */
constexpr uint32_t FIELDMATCH_IMAGE_MAX = FIELDMATCH_MAX_VALUES * 8 + ( FIELDMATCH_MAX_VALUES + 1 ) * 4 + FIELDMATCH_MAX_BYTES;
constexpr int64_t FIELDMATCH_NUMBER_MAX = 999999999999999999ll;   /* 10^18 - 1: the largest number a field can be */

/** What is wrong with the values of a predicate; empty: nothing.  sizes[i] is the size of value i of n. */
[[nodiscard]] inline std::string
valueSetError( const uint32_t* sizes, uint64_t n )
{
    if ( n == 0 || n > FIELDMATCH_MAX_VALUES ) {
        return "the set must have 1 to " + std::to_string( FIELDMATCH_MAX_VALUES ) + " values, not " + std::to_string( n );
    }
    uint64_t sum = 0;
    for ( uint64_t i = 0; i < n; ++i ) {
        if ( sizes[i] > FIELDMATCH_MAX_VALUE_BYTES ) {
            return "value " + std::to_string( i ) + " has " + std::to_string( sizes[i] ) + " bytes, more than "
                   + std::to_string( FIELDMATCH_MAX_VALUE_BYTES );
        }
        sum += sizes[i];
    }
    if ( sum > FIELDMATCH_MAX_BYTES ) {
        return "the values must have at most " + std::to_string( FIELDMATCH_MAX_BYTES ) + " bytes in total, not " + std::to_string( sum );
    }
    return {};
}

/** A value for a message: printable ASCII as it is, every other byte as \xHH. */
[[nodiscard]] inline std::string
quotedValue( const std::string& value )
{
    static const char* const digits = "0123456789abcdef";
    std::string out = "\"";
    for ( const unsigned char byte : value ) {
        if ( byte >= 0x20 && byte < 0x7F && byte != '"' && byte != '\\' ) {
            out += (char)byte;
        } else {
            out += "\\x";
            out += digits[byte >> 4];
            out += digits[byte & 15];
        }
    }
    return out + "\"";
}

/** The values of a predicate as the GPU looks them up; the header says how `image` is laid out. */
struct ValueTable
{
    std::vector<uint64_t> keys;          /* ascending, distinct */
    std::vector<std::string> values;     /* values[i] has keys[i] */
    std::vector<uint8_t> image;

    [[nodiscard]] uint32_t count() const { return (uint32_t)keys.size(); }

    /** The value with this key, or count(). */
    [[nodiscard]] uint32_t
    find( uint64_t key ) const
    {
        const auto at = std::lower_bound( keys.begin(), keys.end(), key );
        return at != keys.end() && *at == key ? (uint32_t)( at - keys.begin() ) : count();
    }

    /** Key and size hit the table: only the bytes can still tell the field from values[the result]; else count(). */
    [[nodiscard]] uint32_t
    candidateValue( uint64_t key, int64_t size ) const
    {
        if ( size < 0 ) return count();
        const uint32_t at = find( key );
        return at < count() && values[at].size() == (uint64_t)size ? at : count();
    }

    /** What k_field_match computes for a line whose field has this key and these bytes (size < 0: no such field). */
    [[nodiscard]] bool
    holds( uint64_t key, const uint8_t* bytes, int64_t size ) const
    {
        const uint32_t at = candidateValue( key, size );
        return at < count() && ( size == 0 || std::memcmp( values[at].data(), bytes, (size_t)size ) == 0 );
    }
};

/** The table of values[i] with the key keys[i] = lineHash( values[i], seed ): sorted by key, equal values once.  The keys
 * are the caller's so that a test can forge them.  Throws std::invalid_argument for a set that valueSetError refuses and
 * for two different values with equal keys. */
[[nodiscard]] inline ValueTable
buildValueTable( const std::vector<std::string>& values, const std::vector<uint64_t>& keys )
{
    if ( values.size() != keys.size() ) throw std::invalid_argument( "a key per value is needed" );
    std::vector<uint32_t> sizes( values.size() );
    for ( size_t i = 0; i < values.size(); ++i ) sizes[i] = (uint32_t)std::min<size_t>( values[i].size(), 0xFFFFFFFFu );
    const auto why = valueSetError( sizes.data(), sizes.size() );
    if ( !why.empty() ) throw std::invalid_argument( why );
    std::vector<uint32_t> order( values.size() );
    std::iota( order.begin(), order.end(), 0u );
    std::sort( order.begin(), order.end(), [&] ( uint32_t a, uint32_t b ) {
        return keys[a] != keys[b] ? keys[a] < keys[b] : values[a] < values[b];
    } );
    ValueTable table;
    for ( const auto i : order ) {
        if ( !table.keys.empty() && table.keys.back() == keys[i] ) {
            if ( table.values.back() == values[i] ) continue;
            throw std::invalid_argument( "the values " + quotedValue( table.values.back() ) + " and " + quotedValue( values[i] )
                                         + " have the same key under this seed: pass another seed" );
        }
        table.keys.push_back( keys[i] );
        table.values.push_back( values[i] );
    }
    const size_t k = table.keys.size();
    size_t bytes = 0;
    for ( const auto& value : table.values ) bytes += value.size();
    const size_t offsetsAt = k * 8, bytesAt = offsetsAt + ( k + 1 ) * 4;
    table.image.assign( ( bytesAt + bytes + 3 ) / 4 * 4, 0 );
    std::memcpy( table.image.data(), table.keys.data(), k * 8 );
    uint32_t at = 0;
    for ( size_t i = 0; i < k; ++i ) {
        std::memcpy( table.image.data() + offsetsAt + i * 4, &at, 4 );
        if ( !table.values[i].empty() ) std::memcpy( table.image.data() + bytesAt + at, table.values[i].data(), table.values[i].size() );
        at += (uint32_t)table.values[i].size();
    }
    std::memcpy( table.image.data() + offsetsAt + k * 4, &at, 4 );
    return table;
}

/** buildValueTable for the n values that lie one behind the other in `bytes`, value i with sizes[i] bytes, under their
 * keys of `seed`. */
[[nodiscard]] inline ValueTable
valueTableOf( const uint8_t* bytes, const uint32_t* sizes, uint64_t n, uint64_t seed )
{
    const auto why = valueSetError( sizes, n );
    if ( !why.empty() ) throw std::invalid_argument( why );
    std::vector<std::string> values( n );
    std::vector<uint64_t> keys( n );
    uint64_t at = 0;
    for ( uint64_t i = 0; i < n; ++i ) {
        if ( sizes[i] > 0 ) values[i].assign( reinterpret_cast<const char*>( bytes ) + at, sizes[i] );
        keys[i] = lineHash( reinterpret_cast<const uint8_t*>( values[i].data() ), values[i].size(), seed );
        at += sizes[i];
    }
    return buildValueTable( values, keys );
}

/** The plain model beside the table: is field[0, size) one of the values (size < 0: the line has no such field)? */
[[nodiscard]] inline bool
valueMatches( const std::vector<std::string>& values, const uint8_t* field, int64_t size )
{
    if ( size < 0 ) return false;
    for ( const auto& value : values ) {
        if ( value.size() == (uint64_t)size && ( size == 0 || std::memcmp( value.data(), field, (size_t)size ) == 0 ) ) return true;
    }
    return false;
}

/** The bounds of a range predicate as the GPU compares them: an open side is the largest or the least number there is,
 * a bound beyond 18 digits is clipped to it.  lo > hi afterwards: no number is in the range. */
struct NumberRange
{
    int64_t lo{ -FIELDMATCH_NUMBER_MAX }, hi{ FIELDMATCH_NUMBER_MAX };

    /** `number` is a field-number word: the two sentinels are below every lo. */
    [[nodiscard]] bool holds( int64_t number ) const { return number >= lo && number <= hi; }
};

[[nodiscard]] inline NumberRange
clipNumberRange( bool hasLo, int64_t lo, bool hasHi, int64_t hi )
{
    NumberRange range;
    if ( hasLo ) range.lo = std::clamp( lo, -FIELDMATCH_NUMBER_MAX, FIELDMATCH_NUMBER_MAX );
    if ( hasHi ) range.hi = std::clamp( hi, -FIELDMATCH_NUMBER_MAX, FIELDMATCH_NUMBER_MAX );
    return range;
}
}  // namespace bz2gpu
