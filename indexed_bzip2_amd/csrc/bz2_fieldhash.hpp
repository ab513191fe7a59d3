/**
 * bz2_fieldhash.hpp -- the 61-bit hash of field j of every line of the decoded file (mi355x_bz2_reader_field_hashes,
 * _field_groups): the definition, the summary of a stretch of bytes, and the rule that stitches the summaries of
 * stretches that lie back to back.  Host code only, no HIP: the reader and the context call it, and
 * tests/native/fieldhash_cases.cpp pins it on the CPU.  The fields are those of bz2_fields.hpp, the hash is that of
 * bz2_linehash.hpp, and the block plan is planLineHashes as it is (the reader calls it for all three column queries).
 *
 * The definition.  The KEY of a line is lineHash( content.split( dl )[j], seed ); a line with fewer than j + 1 fields has
 * the key FIELD_MISSING = 2^61 - 1 = p, which no hash takes; an empty field is present and hashes to 0.
 *
 * The key as a difference of prefixes.  P( pos ) = the hash of the bytes of a line in front of `pos`: it is 0 at the
 * line's start and it is what the line-hash kernels carry along anyway.  For a field over [start, end):
 *     key = P( end ) - P( start ) * x^( end - start )  mod p,
 * so a field needs no scan of its own: two values of the running line hash and one power.
 *
 * What a stretch knows: its FieldSummary and the head and tail ( h, xl ) of its HashSummary, and
 *     headHashes[k]   the hash of the stretch's bytes in front of headPositions[k], the stretch entered with hash 0;
 *     tailStartHash, tailEndHash   P at tailFieldStart and tailFieldEnd of the line that starts at tailStart, where they
 *                     are reached;
 *     keys            of the lines it closes, the first computed as if the stretch were entered at a line start.
 * The carry of an open line is its FieldCarry, its HashPart and P at the field's start and end where they are reached.
 * Across a seam the true prefix at head position k is carry.line.h * x^headPositions[k] + headHashes[k]; a field that
 * starts behind that dl has this value followed by the dl byte; the line is closed at firstNl with
 * carry.line.h * head.xl + head.h; without an nl the carry's line becomes followedBy( carry.line, head ).  The host
 * computes x^n by squaring: once or twice per seam.
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
constexpr uint64_t FIELD_MISSING = LINEHASH_P;

/** x^n mod p by squaring. */
[[nodiscard]] inline uint64_t
powmod( uint64_t x, uint64_t n )
{
    uint64_t power = 1;
    for ( ; n != 0; n >>= 1, x = mulmod( x, x ) ) {
        if ( ( n & 1 ) != 0 ) power = mulmod( power, x );
    }
    return power;
}

/** ( a - b ) mod p for a, b < p. */
[[nodiscard]] inline uint64_t
submod( uint64_t a, uint64_t b )
{
    return a >= b ? a - b : a + LINEHASH_P - b;
}

/** The key of a field of `size` bytes between the prefixes pStart and pEnd. */
[[nodiscard]] inline uint64_t
fieldKey( uint64_t x, uint64_t pStart, uint64_t pEnd, uint64_t size )
{
    return submod( pEnd, mulmod( pStart, powmod( x, size ) ) );
}

/** The key of field j of one line's content, by the definition: split, then hash. */
[[nodiscard]] inline uint64_t
fieldHash( const uint8_t* content, size_t size, uint8_t dl, uint32_t j, uint64_t seed )
{
    size_t at = 0;
    for ( uint32_t k = 0; k < j; ++k ) {
        while ( at < size && content[at] != dl ) ++at;
        if ( at == size ) return FIELD_MISSING;
        ++at;
    }
    size_t end = at;
    while ( end < size && content[end] != dl ) ++end;
    return lineHash( content + at, end - at, seed );
}

/** A line's key and where its field lies. */
struct FieldKey
{
    uint64_t key{ FIELD_MISSING };
    FieldSpan field;

    [[nodiscard]] bool operator==( const FieldKey& o ) const { return key == o.key && field == o.field; }
};

/** An open line: its FieldCarry, the hash of its bytes so far, and P at the field's start and end where reached. */
struct FieldHashCarry
{
    FieldCarry field;
    HashPart line;
    uint64_t startHash{ 0 }, endHash{ 0 };
};

[[nodiscard]] inline FieldHashCarry
fieldHashLineStart( uint32_t j, uint64_t at )
{
    return { fieldLineStart( j, at ), {}, 0, 0 };
}

/** The carry over the head of a stretch at `offset`: n head positions with their hashes.  carry.line is still the line in
 * front of the stretch; the caller moves it on. */
inline void
fieldHashContinue( FieldHashCarry& carry, uint32_t j, uint64_t x, uint8_t dl, const uint64_t* positions, const uint64_t* hashes,
                   uint32_t n, uint64_t offset )
{
    const uint32_t d = carry.field.delims;
    const auto prefixAt = [&] ( uint32_t k ) { return addmod( mulmod( carry.line.h, powmod( x, positions[k] ) ), hashes[k] ); };
    if ( carry.field.start == FIELD_UNKNOWN && d < j && d + n >= j ) {
        carry.startHash = addmod( mulmod( prefixAt( j - d - 1 ), x ), uint64_t( dl ) + 1 );
    }
    if ( carry.field.end == FIELD_UNKNOWN && d <= j && d + n >= j + 1 ) carry.endHash = prefixAt( j - d );
    fieldContinue( carry.field, j, positions, n, offset );
}

/** The open line closed at `at`, where the hash of its whole content is `lineHashAt`. */
[[nodiscard]] inline FieldKey
fieldHashClose( const FieldHashCarry& carry, uint64_t x, uint64_t at, uint64_t lineHashAt )
{
    FieldKey result;
    result.field = fieldClose( carry.field, at );
    if ( result.field.size < 0 ) return result;
    const uint64_t pEnd = carry.field.end != FIELD_UNKNOWN ? carry.endHash : lineHashAt;
    result.key = fieldKey( x, carry.startHash, pEnd, (uint64_t)result.field.size );
    return result;
}

/** The summary of a stretch for field j under base x (the header says what the members mean).  fields.count is the number
 * of lines the stretch closes, whether or not `keys`, fields.starts and fields.sizes list them all. */
struct FieldHashSummary
{
    FieldSummary fields;
    HashPart head, tail;
    std::vector<uint64_t> headHashes;
    uint64_t tailStartHash{ 0 }, tailEndHash{ 0 };
    std::vector<uint64_t> keys;

    [[nodiscard]] FieldHashCarry
    tailCarry() const
    {
        return { fields.tail(), fields.hasDelimiter ? tail : head, tailStartHash, tailEndHash };
    }
};

[[nodiscard]] inline FieldHashSummary
emptyFieldHashSummary( uint32_t j )
{
    FieldHashSummary s;
    s.fields = emptyFieldSummary( j );
    return s;
}

/** The summary of one chunk, as a lane that enters it at a line start with hash 0 walks it. */
inline FieldHashSummary
summariseFieldHashChunk( uint64_t x, const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j )
{
    FieldHashSummary s = emptyFieldHashSummary( j );
    auto& f = s.fields;
    f.size = size;
    FieldHashCarry carry = fieldHashLineStart( j, 0 );
    for ( size_t at = 0; at < size; ++at ) {
        const uint8_t b = bytes[at];
        if ( b == nl ) {
            const auto closed = fieldHashClose( carry, x, at, carry.line.h );
            f.starts.push_back( closed.field.start );
            f.sizes.push_back( closed.field.size );
            s.keys.push_back( closed.key );
            if ( !f.hasDelimiter ) {
                f.firstNl = at;
                s.head = carry.line;
            }
            f.hasDelimiter = true;
            f.tailStart = at + 1;
            carry = fieldHashLineStart( j, at + 1 );
            continue;
        }
        if ( b == dl ) {
            const uint64_t position = at;
            if ( !f.hasDelimiter && f.headPositions.size() <= j ) {
                f.headPositions.push_back( position );
                s.headHashes.push_back( carry.line.h );
            }
            if ( carry.field.delims <= j ) {
                /* the line so far is the prefix itself: continue a carry whose line is empty, the hash being the prefix */
                FieldHashCarry fresh = carry;
                fresh.line = {};
                const uint64_t prefix = carry.line.h;
                fieldHashContinue( fresh, j, x, dl, &position, &prefix, 1, 0 );
                fresh.line = carry.line;
                carry = fresh;
            }
        }
        carry.line = followedBy( carry.line, { uint64_t( b ) + 1, x } );
    }
    ( f.hasDelimiter ? s.tail : s.head ) = carry.line;
    f.setTail( carry.field );
    s.tailStartHash = carry.startHash;
    s.tailEndHash = carry.endHash;
    f.tailNonEmpty = size > 0 && bytes[size - 1] != nl;
    f.count = f.starts.size();
    return s;
}

/** `all` followed by `part`, both for field j under x and with all their lines listed: the rule of the header between two
 * stretches. */
inline void
appendFieldHashSummary( FieldHashSummary& all, const FieldHashSummary& part, uint64_t x, uint8_t dl, uint32_t j )
{
    auto& f = all.fields;
    const auto& g = part.fields;
    const uint64_t offset = f.size;
    FieldHashCarry carry = all.tailCarry();
    if ( !f.hasDelimiter ) {
        for ( size_t i = 0; i < g.headPositions.size() && f.headPositions.size() <= j; ++i ) {
            f.headPositions.push_back( offset + g.headPositions[i] );
            all.headHashes.push_back( addmod( mulmod( all.head.h, powmod( x, g.headPositions[i] ) ), part.headHashes[i] ) );
        }
    }
    fieldHashContinue( carry, j, x, dl, g.headPositions.data(), part.headHashes.data(), g.headDelims(), offset );
    const auto shifted = [offset] ( uint64_t position ) { return position == FIELD_UNKNOWN ? position : offset + position; };
    const HashPart line = followedBy( carry.line, part.head );
    if ( g.hasDelimiter ) {
        const auto closed = fieldHashClose( carry, x, offset + g.firstNl, line.h );
        f.starts.push_back( closed.field.start );
        f.sizes.push_back( closed.field.size );
        all.keys.push_back( closed.key );
        for ( size_t i = 1; i < g.starts.size(); ++i ) {
            f.starts.push_back( offset + g.starts[i] );
            f.sizes.push_back( g.sizes[i] );
            all.keys.push_back( part.keys[i] );
        }
        if ( !f.hasDelimiter ) {
            f.firstNl = offset + g.firstNl;
            all.head = line;
        }
        f.hasDelimiter = true;
        f.tailStart = offset + g.tailStart;
        f.setTail( { g.tailDelims, shifted( g.tailFieldStart ), shifted( g.tailFieldEnd ) } );
        f.tailNonEmpty = g.tailNonEmpty;
        all.tail = part.tail;
        all.tailStartHash = part.tailStartHash;
        all.tailEndHash = part.tailEndHash;
    } else {
        ( f.hasDelimiter ? all.tail : all.head ) = line;
        f.setTail( carry.field );
        all.tailStartHash = carry.startHash;
        all.tailEndHash = carry.endHash;
        f.tailNonEmpty = f.tailNonEmpty || g.tailNonEmpty;
    }
    f.size += g.size;
    f.count = f.starts.size();
}

/** The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as the kernels compose them.  The result
 * does not depend on `chunk`. */
inline FieldHashSummary
summariseFieldHashes( uint64_t x, const uint8_t* bytes, size_t size, uint8_t nl, uint8_t dl, uint32_t j, size_t chunk )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summariseFieldHashes: the chunk size must not be 0" );
    FieldHashSummary all = emptyFieldHashSummary( j );
    for ( size_t at = 0; at < size; at += chunk ) {
        appendFieldHashSummary( all, summariseFieldHashChunk( x, bytes + at, std::min( chunk, size - at ), nl, dl, j ), x, dl, j );
    }
    return all;
}

/** A stretch of D for stitchFieldHashes: where it lies and its summary, whose fields.size is the stretch's.  The summary
 * may list fewer lines than fields.count, or none. */
struct FieldHashStretch
{
    uint64_t fileOffset{ 0 };
    FieldHashSummary summary;
};

/** What stitchFieldHashes found: the number of lines the stretches close, and the unterminated tail behind them. */
struct StitchedFieldHashes
{
    uint64_t closed{ 0 };
    bool hasTail{ false };
    FieldKey tail;
};

/**
 * The rule of the header over stretches that lie back to back (checked: std::invalid_argument) from the offset of the
 * first one, which must be a line's start.  The closed lines are numbered from 0 in the order the stretches close them.
 * patch( k, key ) is called for every closed line k that began in front of the stretch that closes it, with its FieldKey
 * in D; every other line has the key its stretch lists and the field it lists, moved by the stretch's offset.
 */
template<typename Patch>
inline StitchedFieldHashes
stitchFieldHashes( const std::vector<FieldHashStretch>& stretches, uint64_t x, uint8_t dl, uint32_t j, const Patch& patch )
{
    StitchedFieldHashes result;
    uint64_t end = stretches.empty() ? 0 : stretches.front().fileOffset;
    FieldHashCarry carry = fieldHashLineStart( j, end );
    bool carryNonEmpty = false;
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        const auto& s = stretch.summary;
        const auto& f = s.fields;
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchFieldHashes: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        if ( f.size > ~uint64_t( 0 ) - end ) throw std::invalid_argument( "stitchFieldHashes: the stretches overflow 64 bits" );
        const uint64_t offset = end;
        end += f.size;
        if ( f.size == 0 ) continue;
        if ( f.headDelims() > j + 1 ) throw std::invalid_argument( "stitchFieldHashes: a stretch lists too many head positions" );
        if ( s.headHashes.size() != f.headPositions.size() ) {
            throw std::invalid_argument( "stitchFieldHashes: a stretch lists a head position without its hash" );
        }
        fieldHashContinue( carry, j, x, dl, f.headPositions.data(), s.headHashes.data(), f.headDelims(), offset );
        const HashPart line = followedBy( carry.line, s.head );
        if ( f.hasDelimiter ) {
            if ( f.count == 0 || f.firstNl >= f.size ) throw std::invalid_argument( "stitchFieldHashes: a stretch with a delimiter closes no line" );
            if ( carryNonEmpty ) patch( result.closed, fieldHashClose( carry, x, offset + f.firstNl, line.h ) );
            result.closed += f.count;
            carry = { { f.tailDelims, f.tailFieldStart == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + f.tailFieldStart,
                        f.tailFieldEnd == FIELD_UNKNOWN ? FIELD_UNKNOWN : offset + f.tailFieldEnd },
                      s.tail, s.tailStartHash, s.tailEndHash };
            carryNonEmpty = f.tailNonEmpty;
        } else {
            carry.line = line;
            carryNonEmpty = true;
        }
    }
    result.hasTail = carryNonEmpty;
    if ( carryNonEmpty ) result.tail = fieldHashClose( carry, x, end, carry.line.h );
    return result;
}

/** stitchFieldHashes into one list: every closed line's key and field, then the tail's if there is one.  Every stretch
 * must list all its lines. */
inline std::vector<FieldKey>
stitchedFieldHashes( const std::vector<FieldHashStretch>& stretches, uint64_t x, uint8_t dl, uint32_t j )
{
    std::vector<FieldKey> keys;
    for ( const auto& stretch : stretches ) {
        const auto& s = stretch.summary;
        if ( s.keys.size() != s.fields.count || s.fields.starts.size() != s.fields.count || s.fields.sizes.size() != s.fields.count ) {
            throw std::invalid_argument( "stitchedFieldHashes: a stretch does not list all its lines" );
        }
        for ( size_t i = 0; i < s.keys.size(); ++i ) {
            keys.push_back( { s.keys[i], { stretch.fileOffset + s.fields.starts[i], s.fields.sizes[i] } } );
        }
    }
    const auto stitched = stitchFieldHashes( stretches, x, dl, j, [&] ( uint64_t k, const FieldKey& key ) { keys[(size_t)k] = key; } );
    if ( stitched.hasTail ) keys.push_back( stitched.tail );
    return keys;
}
}  // namespace bz2gpu
