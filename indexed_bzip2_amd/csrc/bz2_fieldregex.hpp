/**
 * bz2_fieldregex.hpp -- does field j of a line match a regular expression (mi355x_bz2_match_fields_regex,
 * mi355x_bz2_reader_field_matches_regex): the definition, as a plain model.  Host code only, no HIP: the reader decides the
 * lines at launch seams and the tail with it, and tests/native/fieldregex_cases.cpp pins it on the CPU.
 *
 * Lines and fields are bz2_fields.hpp's, the automaton is bz2_regex.hpp's: state 0 = no byte yet, state 1 = A = matched and
 * absorbing, acceptsAtEnd decides `$`.  The field is to the pattern what a line's content is to grep_regex:
 *
 *   A line MATCHES iff it has the field and the table, run from state 0 over the field's bytes, reaches A or ends in a
 *   state q with acceptsAtEnd[q].  `^` and `$` so anchor to the field's ends.  An empty field that is present is the empty
 *   content and matches iff acceptsAtEnd[0]; a missing field (size < 0) never matches.  There is no cap on a field's size.
 *
 * The table does not know the line delimiter: a field that holds the byte 0x0A (possible with another `newline`) is run
 * like any other, and `$` does not match in front of it as Python's does.
 *
 * The DEAD state.  A state d != A all of whose 256 transitions lead back to d and that does not accept at the end can never
 * lead to a match: a run that reaches it may stop with the answer "no".  The compiler minimises, so there is at most one
 * such state; `^GET` has one (any first byte but G leads there), an unanchored pattern has none, since every state can
 * start the pattern again.  With the stop at A this bounds the cost of an anchored prefix pattern by the prefix, whatever
 * the field's length; k_field_regex (bz2_fieldregex.hip.h) stops at both.
 */
#pragma once

#include <cstdint>

#include "bz2_regex.hpp"

namespace bz2gpu
{
/** The definition: does the field bytes[0, size) match?  size < 0: the line has no such field. */
[[nodiscard]] inline bool
fieldRegexHolds( const Regex& regex, const uint8_t* bytes, int64_t size )
{
    if ( size < 0 ) return false;
    uint8_t state = REGEX_START;
    for ( int64_t i = 0; i < size; ++i ) {
        state = regex.transitions[(size_t)state * 256 + bytes[i]];
        if ( state == REGEX_MATCHED ) return true;
    }
    return regex.acceptsAtEnd[state] != 0;
}

/** The state from which no match can follow (the header says why there is at most one), or REGEX_MAX_STATES, which no
 * state is, where there is none. */
[[nodiscard]] inline uint32_t
regexDeadState( const Regex& regex )
{
    for ( uint32_t d = 0; d < regex.n; ++d ) {
        if ( d == REGEX_MATCHED || regex.acceptsAtEnd[d] != 0 ) continue;
        bool closed = true;
        for ( uint32_t b = 0; b < 256 && closed; ++b ) closed = regex.transitions[(size_t)d * 256 + b] == d;
        if ( closed ) return d;
    }
    return REGEX_MAX_STATES;
}

/** fieldRegexHolds as k_field_regex runs it: the walk stops at the first byte that leads to A or to `dead` (regexDeadState's
 * answer).  *steps, if given, receives the bytes walked.  The answer is fieldRegexHolds': the tests pin that. */
[[nodiscard]] inline bool
fieldRegexHoldsStopping( const Regex& regex, uint32_t dead, const uint8_t* bytes, int64_t size, uint64_t* steps = nullptr )
{
    if ( steps != nullptr ) *steps = 0;
    if ( size < 0 ) return false;
    uint32_t state = REGEX_START;
    for ( int64_t i = 0; i < size; ++i ) {
        state = regex.transitions[(size_t)state * 256 + bytes[i]];
        if ( steps != nullptr ) ++*steps;
        if ( state == REGEX_MATCHED || state == dead ) break;
    }
    return regex.acceptsAtEnd[state] != 0;
}
}  // namespace bz2gpu
