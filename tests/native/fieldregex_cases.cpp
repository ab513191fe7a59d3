/**
 * fieldregex_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldregex.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: fieldRegexHolds against the table run by hand, regexDeadState on patterns whose
 * answer is known and against its definition on every compiled pattern, that stopping at the dead state never changes an
 * answer (and bounds the walk of an anchored prefix), and the launcher's layout (bz2_query_layout.hpp: layFieldRegex).
 *
 * Without arguments it runs over a list of patterns and fields of its own.  With one argument, a file of records
 * ( kind: 'P' pattern, 'I' pattern with ignore_case, 'F' field; uint32 little-endian size; bytes ), it runs over those too:
 * the test suite hands in regexgen's patterns and the fields of its corpus.  Every field is copied to a buffer of exactly
 * its size, so that a read beyond it is the sanitizer's.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iterator>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fieldregex.hpp"
#include "../../indexed_bzip2_amd/csrc/bz2_query_layout.hpp"

using namespace bz2gpu;

#define CHECK( condition )                                                           \
    do {                                                                             \
        if ( !( condition ) ) {                                                      \
            std::fprintf( stderr, "%s:%d: %s\n", __FILE__, __LINE__, #condition );   \
            std::exit( 1 );                                                          \
        }                                                                            \
    } while ( 0 )

namespace
{
Regex
compiled( const std::string& pattern, bool fold = false )
{
    return compileRegex( reinterpret_cast<const uint8_t*>( pattern.data() ), pattern.size(), fold );
}

/** regex.transitions run by hand, with no early return: the state behind every byte, A being absorbing. */
bool
byHand( const Regex& regex, const std::vector<uint8_t>& field )
{
    uint32_t state = 0;
    bool matched = false;
    for ( const uint8_t byte : field ) {
        CHECK( state < regex.n );
        state = regex.transitions[(size_t)state * 256 + byte];
        matched = matched || state == 1;
    }
    return matched || regex.acceptsAtEnd[state] != 0;
}

/** The definition of the dead state, state by state. */
uint32_t
deadByDefinition( const Regex& regex )
{
    uint32_t found = REGEX_MAX_STATES, count = 0;
    for ( uint32_t d = 0; d < regex.n; ++d ) {
        bool closed = d != 1 && regex.acceptsAtEnd[d] == 0;
        for ( uint32_t b = 0; b < 256; ++b ) closed = closed && regex.transitions[(size_t)d * 256 + b] == d;
        if ( closed ) {
            if ( count++ == 0 ) found = d;
        }
    }
    CHECK( count <= 1 );        /* the compiler minimises: two such states would be one */
    return found;
}

bool
holds( const Regex& regex, const std::string& field )
{
    const std::vector<uint8_t> exact( field.begin(), field.end() );
    return fieldRegexHolds( regex, exact.data(), (int64_t)exact.size() );
}

void
checkPattern( const Regex& regex, const std::vector<std::vector<uint8_t> >& fields, uint64_t* walked, uint64_t* walkedStopping )
{
    CHECK( regex.n >= 2 && regex.n <= REGEX_MAX_STATES && regex.acceptsAtEnd[1] != 0 );
    const uint32_t dead = regexDeadState( regex );
    CHECK( dead == deadByDefinition( regex ) );
    CHECK( dead == REGEX_MAX_STATES || ( dead < regex.n && dead != 1 && regex.acceptsAtEnd[dead] == 0 ) );
    CHECK( !fieldRegexHolds( regex, nullptr, -1 ) && !fieldRegexHoldsStopping( regex, dead, nullptr, -1 ) );
    CHECK( fieldRegexHolds( regex, nullptr, 0 ) == ( regex.acceptsAtEnd[0] != 0 ) );
    for ( const auto& field : fields ) {
        const bool want = byHand( regex, field );
        CHECK( fieldRegexHolds( regex, field.data(), (int64_t)field.size() ) == want );
        uint64_t steps = 0;
        CHECK( fieldRegexHoldsStopping( regex, dead, field.data(), (int64_t)field.size(), &steps ) == want );
        CHECK( steps <= field.size() );
        /* without a dead state the stop is at A alone: still the same answer */
        CHECK( fieldRegexHoldsStopping( regex, REGEX_MAX_STATES, field.data(), (int64_t)field.size() ) == want );
        *walked += field.size();
        *walkedStopping += steps;
    }
}

std::vector<std::vector<uint8_t> >
ownFields()
{
    std::vector<std::vector<uint8_t> > fields;
    const std::string texts[] = { "", "a", "b", "GET", "GE", "GETS", "xGET", "get", "xb", "ab", "ba", "aaa", "-12", "12x", "+7",
                                  std::string( "\x80\xff", 2 ), std::string( "a\nb", 3 ), std::string( "\0", 1 ), "error, fatal",
                                  std::string( 5000, 'a' ), std::string( 257, 'q' ) + "b" };
    for ( const auto& text : texts ) fields.emplace_back( text.begin(), text.end() );
    /* every field of 0 to 3 bytes over a small alphabet */
    const std::string alphabet = "abGET-1\n";
    for ( const char x : alphabet ) {
        for ( const char y : alphabet ) {
            fields.push_back( { (uint8_t)x, (uint8_t)y } );
            for ( const char z : alphabet ) fields.push_back( { (uint8_t)x, (uint8_t)y, (uint8_t)z } );
        }
    }
    return fields;
}
}  // namespace

int
main( int argc, char** argv )
{
    /* the dead state where the answer is known */
    {
        const Regex anchored = compiled( "^GET" );
        const uint32_t dead = regexDeadState( anchored );
        CHECK( dead < anchored.n && dead != 0 && dead != 1 );
        CHECK( anchored.transitions[0 * 256 + 'x'] == dead && anchored.transitions[0 * 256 + 'G'] != dead );
        /* an anchored prefix costs the prefix, whatever the field's length */
        const std::vector<uint8_t> longField( 100000, 'x' );
        uint64_t steps = 0;
        CHECK( !fieldRegexHoldsStopping( anchored, dead, longField.data(), (int64_t)longField.size(), &steps ) && steps == 1 );
        std::vector<uint8_t> hit( 100000, 'x' );
        std::memcpy( hit.data(), "GET", 3 );
        CHECK( fieldRegexHoldsStopping( anchored, dead, hit.data(), (int64_t)hit.size(), &steps ) && steps == 3 );
        CHECK( holds( anchored, "GETS" ) && !holds( anchored, "xGET" ) && !holds( anchored, "" ) && !holds( anchored, "GE" ) );

        CHECK( regexDeadState( compiled( "GET" ) ) == REGEX_MAX_STATES );          /* unanchored: every state can start again */
        const Regex emptyOnly = compiled( "^$" );
        const uint32_t deadOfEmpty = regexDeadState( emptyOnly );
        CHECK( deadOfEmpty < emptyOnly.n && emptyOnly.acceptsAtEnd[0] != 0 );
        for ( uint32_t b = 0; b < 256; ++b ) CHECK( emptyOnly.transitions[b] == deadOfEmpty );
        CHECK( holds( emptyOnly, "" ) && !holds( emptyOnly, "a" ) );
        const Regex anything = compiled( "a*" );                                   /* matches the empty string: none needed */
        CHECK( regexDeadState( anything ) == REGEX_MAX_STATES && anything.acceptsAtEnd[0] != 0 );
        CHECK( holds( anything, "" ) && holds( anything, "zzz" ) );
        /* `^a` alone is dead behind an x, `^a|b$` is not: the b may still come */
        const Regex either = compiled( "^a|b$" );
        CHECK( regexDeadState( either ) == REGEX_MAX_STATES );
        CHECK( holds( either, "xb" ) && holds( either, "ax" ) && !holds( either, "xbx" ) && !holds( either, "" ) );
        const uint32_t deadOfA = regexDeadState( compiled( "^a" ) );
        CHECK( deadOfA < REGEX_MAX_STATES );
        /* the wrong dead state would change the answer: the check below is able to fail */
        const std::vector<uint8_t> xb{ 'x', 'b' };
        CHECK( !fieldRegexHoldsStopping( either, either.transitions[0 * 256 + 'x'], xb.data(), 2 ) );
        CHECK( fieldRegexHoldsStopping( either, regexDeadState( either ), xb.data(), 2 ) );
        const Regex folded = compiled( "^get$", true );
        CHECK( holds( folded, "GeT" ) && !holds( folded, "GeTs" ) && regexDeadState( folded ) < folded.n );
    }

    std::vector<std::pair<std::string, bool> > patterns;
    for ( const char* pattern : { "^GET$", "^GE", "T$", "^$", "a*", "E", "[\\x80-\\xff]", "^-?[0-9]+$", "^a|b$", "(a$|^b)c?", "^(a|b)*c",
                                  "^[^a]", "x.*y", "^(GE|GET|PUT)$", "[a-c]{3}", "^.$", "^a{2,}b" } ) {
        patterns.emplace_back( pattern, false );
        patterns.emplace_back( pattern, true );
    }
    auto fields = ownFields();
    if ( argc > 1 ) {
        std::ifstream in( argv[1], std::ios::binary );
        CHECK( in.good() );
        const std::vector<char> bytes( ( std::istreambuf_iterator<char>( in ) ), std::istreambuf_iterator<char>() );
        size_t at = 0;
        while ( at < bytes.size() ) {
            CHECK( at + 5 <= bytes.size() );
            const char kind = bytes[at];
            uint32_t size = 0;
            for ( int k = 0; k < 4; ++k ) size |= (uint32_t)(uint8_t)bytes[at + 1 + k] << ( 8 * k );
            at += 5;
            CHECK( size <= bytes.size() - at );
            if ( kind == 'F' ) {
                fields.emplace_back( bytes.begin() + at, bytes.begin() + at + size );
            } else {
                CHECK( kind == 'P' || kind == 'I' );
                patterns.emplace_back( std::string( bytes.begin() + at, bytes.begin() + at + size ), kind == 'I' );
            }
            at += size;
        }
    }

    uint64_t nCompiled = 0, nRefused = 0, nDead = 0, walked = 0, walkedStopping = 0;
    for ( const auto& [pattern, fold] : patterns ) {
        Regex regex;
        try {
            regex = compiled( pattern, fold );
        } catch ( const std::invalid_argument& ) {
            ++nRefused;     /* more than 64 states: the random patterns hold a few */
            continue;
        }
        ++nCompiled;
        nDead += regexDeadState( regex ) != REGEX_MAX_STATES ? 1 : 0;
        checkPattern( regex, fields, &walked, &walkedStopping );
    }
    CHECK( nCompiled >= 34 && nDead >= 8 && nDead < nCompiled && walkedStopping < walked );

    /* the launcher's layout: the table at 0, acceptsAtEnd behind it on a 16-byte boundary, 64 bytes of it */
    for ( const uint64_t states : { 2, 3, 17, 64 } ) {
        const FieldRegexLayout l = layFieldRegex( states, REGEX_MAX_STATES );
        CHECK( l.tableAt == 0 && l.acceptsAt == states * 256 && l.acceptsAt % 16 == 0 && l.bytes == states * 256 + REGEX_MAX_STATES );
    }

    std::printf( "fieldregex cases ok: %llu patterns compiled, %llu refused, %llu with a dead state, %llu fields, %llu of %llu bytes walked\n",
                 (unsigned long long)nCompiled, (unsigned long long)nRefused, (unsigned long long)nDead, (unsigned long long)fields.size(),
                 (unsigned long long)walkedStopping, (unsigned long long)walked );
    return 0;
}
