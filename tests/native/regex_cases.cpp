/* The regular-expression compiler and the summaries of bz2_regex.hpp against answers written out by hand and a
 * line-by-line run of the table.
 *
 * The compiler: for a fixed list of (pattern, ignore case) the table is run over a fixed list of lines, and the answer
 * must be the one written next to it (they are Python's: re.search( pattern, line, re.DOTALL [| re.IGNORECASE] ));
 * state counts of four patterns; for every table: state 1 absorbing and accepting, no transition into state 0; the
 * refusals by the word their message must hold; the state cap with its count, the raw cap.
 *
 * summarise + stitchSummaries: short texts over a, b, x, y, ',' and the delimiter, cut at every position and at every pair
 * of positions into stretches, each stretch summarised at chunk sizes 1, 2, 3 and 5 (and whole).  The stitched witnesses
 * must be strictly ascending, exactly one per matching line -- matching decided by running the table over that line
 * alone --, each inside its line.  Texts with and without a final delimiter, empty lines at cuts, a text that is one
 * delimiter, an empty text, and patterns that match the empty string, ^ and $.
 *
 * The stitch beyond 2^32: the same cases once more behind a front stretch of 2^32 - k bytes (k = 0, 1, 300) whose summary
 * is written down and whose bytes are never held, closed by a delimiter or open: fileOffset and witnesses above 2^32, a
 * seam exactly at 2^32, a line across it; the expected lines are the unshifted ones plus the shift, and the front's own.
 * Prints "regex ok". */
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_regex.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
std::string currentCase;

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 20 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase.c_str(), #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

Regex
compiled( const std::string& pattern, bool fold = false )
{
    return compileRegex( reinterpret_cast<const uint8_t*>( pattern.data() ), pattern.size(), fold );
}

bool
lineMatches( const Regex& regex, const uint8_t* line, size_t size )
{
    uint8_t state = REGEX_START;
    for ( size_t i = 0; i < size; ++i ) {
        state = regex.transitions[(size_t)state * 256 + line[i]];
        if ( state == REGEX_MATCHED ) return true;
    }
    return regex.acceptsAtEnd[state] != 0;
}

bool
lineMatches( const Regex& regex, const std::string& line )
{
    return lineMatches( regex, reinterpret_cast<const uint8_t*>( line.data() ), line.size() );
}

void
checkInvariants( const Regex& regex )
{
    CHECK( regex.n >= 2 && regex.n <= REGEX_MAX_STATES );
    CHECK( regex.transitions.size() == (size_t)regex.n * 256 && regex.acceptsAtEnd.size() == regex.n );
    CHECK( regex.acceptsAtEnd[REGEX_MATCHED] == 1 );
    for ( uint32_t q = 0; q < regex.n; ++q ) {
        for ( uint32_t b = 0; b < 256; ++b ) {
            const uint8_t next = regex.transitions[(size_t)q * 256 + b];
            CHECK( next < regex.n && next != REGEX_START );
            if ( q == REGEX_MATCHED ) CHECK( next == REGEX_MATCHED );
        }
    }
}

struct Answer
{
    const char* pattern;
    bool fold;
    const char* matching;      /* lines that match, separated by '|' ... */
    const char* others;        /* ... and lines that do not ("~" stands for the empty line) */
};

/* the answers are Python's */
const Answer ANSWERS[] = {
    { "error", false, "error|an error here|xerrorx", "~|erro|Error|err or" },
    { "error", true, "ERROR|an Error|eRRoR", "~|erro" },
    { "a*", false, "~|b|aaa", "" },
    { "^$", false, "~", "a| " },
    { "a^b", false, "", "~|ab|a^b|b" },
    { "$a", false, "", "~|a|$a" },
    { "(^|,)x(,|$)", false, "x|x,y|y,x|a,x,b", "~|xy|yx|a,xb" },
    { "[^a]", true, "b|ab|1", "~|a|A|aA" },
    { "[^a]", false, "A|b", "~|a|aa" },
    { "\\xe9t\\xe9", false, "\xe9t\xe9|x\xe9t\xe9", "\xc9t\xe9|ete" },
    { "\\xe9T\\xe9", true, "\xe9t\xe9|\xe9T\xe9", "\xc9t\xe9" },
    { "a{,2}b", false, "b|ab|aab|aaab", "~|a" },
    { "^a{,2}b", false, "b|ab|aab", "aaab|~" },
    { "^a+$", false, "a|aaaa", "~|ab|ba|aab" },
    { "x.*y.*z", false, "xyz|axbycz|xxyyzz", "~|xzy|zyx|xy" },
    { "\\d{1,3}\\.\\d{1,3}", false, "1.2|x123.456y|1234.5", "1.|.2|12,3" },
    { "^(GET|POST) /[a-z/]* HTTP/1\\.[01]$", false, "GET / HTTP/1.1|POST /a/b HTTP/1.0", "GET /A HTTP/1.1|GET / HTTP/1.2| GET / HTTP/1.1|GET / HTTP/1.1 " },
    { "\\.$", false, "a.|.", "~|.a" },
    { "^\\s*$", false, "~| |\t \t", "a| a" },
    { "\\w+@\\w+\\.com", false, "a@b.com|xx a_1@b2.com yy", "@b.com|a@.com|a@b,com" },
    { "\\D\\d\\D", false, "a1b| 2 ", "12|a1|111" },
    { "\\W\\w\\W", false, " a |,_,", "aaa|a" },
    { "\\S\\s\\S", false, "a b|a\tb", "a  b|ab" },
    { "(?:ab)+c", false, "abc|ababc", "ac|abab" },
    { "(ab|cd)*ef", false, "ef|abef|abcdef", "e|abe" },
    { "a?b?c?d", false, "d|abcd|xd", "abc|~" },
    { "[a\\-c]b", false, "ab|-b|cb", "bb|b" },
    { "[\\]\\[]", false, "]|[", "~|a" },
    { "\\t|\\r|\\f|\\v", false, "\t|a\rb|\f|\v", "~|a| " },
    { "q|", false, "~|a|q", "" },
    { "(|a)b", false, "b|ab", "a|~" },
    { "}x|]y", false, "}x|]y", "x|y|}y" },
    { "^a|b$", false, "a|ab|xb", "~|ba|xa" },
    { "(a$|^b)c?", false, "a|xa|b|bx", "ax|xbx|~" },
    { "[Qq]u[aeiou]+", false, "qui|Quae", "qu|QUI" },
    { "^\\S+ \\S+$", false, "a b|ab cd", "a|a b c| a b" },
    { "a{2,}b", false, "aab|aaaab", "ab|aa" },
    { "[\\d\\s]x", false, "1x| x", "ax|x" },
    { "[^a-c]{2,}$", false, "xdd|dd", "dda|d|~" },
    { "a.b", false, "a\nb|a b", "ab" },          /* DOTALL: the table does not know the delimiter */
};

/** The items of `list` between '|'; "~" stands for the empty line, and an empty list has no items. */
std::vector<std::string>
splitOn( const char* list )
{
    std::vector<std::string> out;
    if ( *list == '\0' ) return out;
    std::string item;
    for ( const char* p = list;; ++p ) {
        if ( *p == '|' || *p == '\0' ) {
            out.push_back( item == "~" ? std::string() : item );
            item.clear();
            if ( *p == '\0' ) break;
        } else {
            item += *p;
        }
    }
    return out;
}

void
testCompiler()
{
    for ( const auto& answer : ANSWERS ) {
        currentCase = std::string( answer.pattern ) + ( answer.fold ? " (fold)" : "" );
        const auto regex = compiled( answer.pattern, answer.fold );
        checkInvariants( regex );
        for ( const auto& line : splitOn( answer.matching ) ) {
            currentCase = std::string( answer.pattern ) + " must match '" + line + "'";
            CHECK( lineMatches( regex, line ) );
        }
        for ( const auto& line : splitOn( answer.others ) ) {
            currentCase = std::string( answer.pattern ) + " must not match '" + line + "'";
            CHECK( !lineMatches( regex, line ) );
        }
    }
    currentCase = "a pattern with a NUL and the byte 0xFF";
    {
        const std::string pattern( "a\\0[\\xfe-\\xff]" );
        const auto regex = compiled( pattern );
        const uint8_t yes[] = { 'a', 0, 0xFF }, no[] = { 'a', 0, 0xFD };
        CHECK( lineMatches( regex, yes, 3 ) && !lineMatches( regex, no, 3 ) );
    }
    currentCase = "state counts";
    CHECK( compiled( "error" ).n == 7 );
    CHECK( compiled( "(error|warning|fatal)" ).n == 17 );
    CHECK( compiled( "\\d{1,3}\\.\\d{1,3}\\.\\d{1,3}\\.\\d{1,3}" ).n == 13 );
    CHECK( compiled( "^(GET|POST) /[a-z/]* HTTP/1\\.[01]$" ).n == 19 );
    currentCase = "the empty match";
    {
        const auto regex = compiled( "a*" );
        CHECK( regex.acceptsAtEnd[REGEX_START] == 1 );
        for ( uint32_t b = 0; b < 256; ++b ) CHECK( regex.transitions[b] == REGEX_MATCHED );
    }
}

void
testRefusals()
{
    struct Refusal { std::string pattern; const char* word; };
    const Refusal refusals[] = {
        { "(a)\\1", "back-reference" }, { "a(?=b)", "look-around" }, { "a(?!b)", "look-around" }, { "(?<=a)b", "look-around" },
        { "(?<!a)b", "look-around" }, { "(?i)a", "inline flags" }, { "(?P<x>a)", "named group" }, { "a*?", "lazy" },
        { "a+?", "lazy" }, { "a??", "lazy" }, { "a{1,2}?", "lazy" }, { "a*+", "possessive" }, { "a\\b", "\\b" }, { "a\\B", "\\B" },
        { "\\Aa", "\\A" }, { "a\\Z", "\\Z" }, { "", "empty pattern" }, { std::string( 4097, 'a' ), "4096" }, { "a{256}", "255" },
        { "a{3,2}", "min above max" }, { "a{", "'{'" }, { "a{x}", "'{'" }, { "a{,}", "'{'" }, { "*a", "nothing to repeat" },
        { "^*", "nothing to repeat" }, { "a**", "multiple repeat" }, { "(a", "unbalanced" }, { "a)", "unbalanced" },
        { "[a", "unterminated class" }, { "[]a]", "']'" }, { "[z-a]", "range" }, { "[\\d-z]", "range" }, { "\\012", "octal" },
        { "\\x4", "\\xHH" }, { "\\q", "escape \\q" }, { "a\\", "backslash" }, { "a\\ b", "backslash" },
        { "^(a|b)*a(a|b){7}$", "needs 259 states" }, { "(a|b)*a(a|b){20}$", "2048" },
        { "((((a{200}){200}){200}){200})", "NFA states" },
    };
    for ( const auto& refusal : refusals ) {
        currentCase = "refusing '" + refusal.pattern.substr( 0, 40 ) + "'";
        bool refused = false;
        try {
            (void)compiled( refusal.pattern );
        } catch ( const std::invalid_argument& why ) {
            refused = true;
            CHECK( std::strstr( why.what(), refusal.word ) != nullptr );
            /* the parser's refusals name the offset */
            if ( std::strstr( why.what(), "states" ) == nullptr && !refusal.pattern.empty() && refusal.pattern.size() < 4097 ) {
                CHECK( std::strstr( why.what(), "at offset" ) != nullptr );
            }
        }
        CHECK( refused );
    }
}

/* every matching line of `text` once: its number */
std::vector<size_t>
matchingLines( const Regex& regex, const std::string& text, char nl, std::vector<std::pair<size_t, size_t> >* extents )
{
    std::vector<size_t> lines;
    extents->clear();
    size_t at = 0;
    while ( at < text.size() ) {
        size_t end = text.find( nl, at );
        const bool closed = end != std::string::npos;
        if ( !closed ) end = text.size();
        if ( lineMatches( regex, reinterpret_cast<const uint8_t*>( text.data() ) + at, end - at ) ) lines.push_back( extents->size() );
        extents->push_back( { at, closed ? end + 1 : end } );   /* [first byte, behind the delimiter) */
        at = closed ? end + 1 : end;
    }
    return lines;
}

void
checkCuts( const Regex& regex, const std::string& text, char nl, const std::vector<size_t>& cuts, size_t chunk )
{
    std::vector<std::pair<size_t, size_t> > extents;
    const auto expected = matchingLines( regex, text, nl, &extents );
    std::vector<Stretch> stretches;
    size_t from = 0;
    for ( size_t k = 0; k <= cuts.size(); ++k ) {
        const size_t to = k < cuts.size() ? cuts[k] : text.size();
        Stretch stretch;
        stretch.fileOffset = from;
        stretch.size = to - from;
        stretch.summary = summarise( regex, reinterpret_cast<const uint8_t*>( text.data() ) + from, to - from, (uint8_t)nl,
                                     chunk == 0 ? text.size() + 1 : chunk, from );
        stretches.push_back( std::move( stretch ) );
        from = to;
    }
    std::vector<uint64_t> witnesses;
    const auto count = stitchSummaries( regex, stretches, &witnesses );
    CHECK( count == expected.size() && witnesses.size() == expected.size() );
    CHECK( stitchSummaries( regex, stretches, nullptr ) == expected.size() );
    for ( size_t i = 0; i < witnesses.size() && i < expected.size(); ++i ) {
        const auto& line = extents[expected[i]];
        CHECK( witnesses[i] >= line.first && witnesses[i] < line.second );
    }
}

/* ---- the same cases behind a front stretch of 2^32 - k bytes that is never held in memory ----
 *
 * The front is FRONT_BYTE over and over -- closed by one delimiter (the text then starts a line at 2^32 - k) or open (the
 * text's first line then begins at offset 0 and is more than 4 GB long).  Its summary is written down, not computed from
 * bytes: the map of one FRONT_BYTE is applied until one more application changes nothing (checked; no pattern here counts
 * FRONT_BYTEs), which is then the head map of any longer run of it. */
constexpr uint8_t FRONT_BYTE = 'q';
constexpr uint64_t TWO_32 = uint64_t( 1 ) << 32;

StretchSummary
frontSummary( const Regex& regex, bool closed )
{
    StretchSummary s;
    for ( uint32_t q = 0; q < regex.n; ++q ) s.headMap[q] = (uint8_t)q;
    bool stable = false;
    for ( int round = 0; round < 64 && !stable; ++round ) {
        stable = true;
        for ( uint32_t q = 0; q < regex.n; ++q ) {
            const uint8_t next = regex.transitions[(size_t)s.headMap[q] * 256 + FRONT_BYTE];
            stable = stable && next == s.headMap[q];
            s.headMap[q] = next;
        }
    }
    CHECK( stable );
    s.hasDelimiter = closed;      /* closed: the delimiter is the front's last byte, nothing follows it: exit 0, no body */
    return s;
}

/** The lines of front + text and which of them match: the table walked over the text from the state the front leaves. */
std::vector<size_t>
matchingLinesBehind( const Regex& regex, const StretchSummary& front, uint64_t frontSize, bool closed, const std::string& text,
                     char nl, std::vector<std::pair<uint64_t, uint64_t> >* extents )
{
    std::vector<size_t> lines;
    extents->clear();
    uint8_t state = front.headMap[REGEX_START];
    uint64_t lineStart = 0;
    const auto close = [&] ( uint64_t end ) {
        if ( state == REGEX_MATCHED || regex.acceptsAtEnd[state] != 0 ) lines.push_back( extents->size() );
        extents->push_back( { lineStart, end } );
        lineStart = end;
        state = REGEX_START;
    };
    if ( closed ) close( frontSize );
    for ( size_t i = 0; i < text.size(); ++i ) {
        if ( text[i] == nl ) {
            close( frontSize + i + 1 );
        } else if ( state != REGEX_MATCHED ) {
            state = regex.transitions[(size_t)state * 256 + (uint8_t)text[i]];
        }
    }
    if ( lineStart < frontSize + text.size() ) close( frontSize + text.size() );
    return lines;
}

void
checkCutsBehind( const Regex& regex, const std::string& text, char nl, const std::vector<size_t>& cuts, size_t chunk,
                 uint64_t frontSize, bool closed )
{
    std::vector<Stretch> stretches( 1 );
    stretches[0].size = frontSize;
    stretches[0].summary = frontSummary( regex, closed );
    std::vector<std::pair<uint64_t, uint64_t> > extents;
    const auto expected = matchingLinesBehind( regex, stretches[0].summary, frontSize, closed, text, nl, &extents );
    size_t from = 0;
    for ( size_t k = 0; k <= cuts.size(); ++k ) {
        const size_t to = k < cuts.size() ? cuts[k] : text.size();
        Stretch stretch;
        stretch.fileOffset = frontSize + from;
        stretch.size = to - from;
        stretch.summary = summarise( regex, reinterpret_cast<const uint8_t*>( text.data() ) + from, to - from, (uint8_t)nl,
                                     chunk == 0 ? text.size() + 1 : chunk, frontSize + from );
        stretches.push_back( std::move( stretch ) );
        from = to;
    }
    std::vector<uint64_t> witnesses;
    const auto count = stitchSummaries( regex, stretches, &witnesses );
    CHECK( count == expected.size() && witnesses.size() == expected.size() );
    CHECK( stitchSummaries( regex, stretches, nullptr ) == expected.size() );
    for ( size_t i = 0; i < witnesses.size() && i < expected.size(); ++i ) {
        const auto& line = extents[expected[i]];
        CHECK( witnesses[i] >= line.first && witnesses[i] < line.second );
        CHECK( i == 0 || witnesses[i] > witnesses[i - 1] );
        /* a line that starts in the text has its witness in the text: beyond what 32 bits hold where the line is */
        if ( line.first >= frontSize ) CHECK( witnesses[i] >= frontSize && ( line.first < TWO_32 || witnesses[i] >= TWO_32 ) );
    }
}

void
testSummariesBeyondFourGiB( const char* const* patterns, size_t nPatterns, const char* const* texts, size_t nTexts )
{
    for ( size_t p = 0; p < nPatterns; ++p ) {
        for ( const bool fold : { false, true } ) {
            const auto regex = compiled( patterns[p], fold );
            for ( const bool closed : { true, false } ) {
                /* k = 0: the seam between front and text lies at 2^32; k = 1: the text's first line straddles it */
                for ( const uint64_t k : { uint64_t( 0 ), uint64_t( 1 ) } ) {
                    for ( size_t t = 0; t < nTexts; ++t ) {
                        const std::string text( texts[t] );
                        for ( const size_t chunk : { size_t( 0 ), size_t( 1 ), size_t( 3 ) } ) {
                            currentCase = std::string( patterns[p] ) + " behind 2^32 - " + std::to_string( k ) + ( closed ? " closed" : " open" )
                                          + " bytes, a text of " + std::to_string( text.size() ) + " bytes, chunk " + std::to_string( chunk );
                            checkCutsBehind( regex, text, '\n', {}, chunk, TWO_32 - k, closed );
                            for ( size_t a = 0; a <= text.size(); ++a ) {
                                checkCutsBehind( regex, text, '\n', { a }, chunk, TWO_32 - k, closed );
                                for ( size_t b = a; b <= text.size(); ++b ) checkCutsBehind( regex, text, '\n', { a, b }, chunk, TWO_32 - k, closed );
                            }
                        }
                    }
                }
                /* k = 300 under a text of 600 bytes: every single cut, the one at 2^32 exactly among them, lines on both
                 * sides of it and one across it */
                std::string text;
                while ( text.size() < 600 ) text += "aab\n\nb\nxay\nx,y\n,x\nabababab\n";
                text.resize( 600 );
                for ( const size_t chunk : { size_t( 0 ), size_t( 5 ) } ) {
                    currentCase = std::string( patterns[p] ) + " behind 2^32 - 300 bytes, chunk " + std::to_string( chunk );
                    for ( size_t a = 0; a <= text.size(); ++a ) checkCutsBehind( regex, text, '\n', { a }, chunk, TWO_32 - 300, closed );
                    checkCutsBehind( regex, text, '\n', { 299, 300, 301 }, chunk, TWO_32 - 300, closed );
                }
            }
        }
    }
}

void
testSummaries()
{
    const char* patterns[] = { "ab", "a*", "^$", "^a+$", "x.*y", "b$", "^b", "(^|,)x(,|$)", "a^b", "[^a]" };
    const char* texts[] = {
        "", "\n", "\n\n", "ab", "ab\n", "a\nb", "\nab\n\n", "aab\n\nb\nxay\n", "x\ny\nx,y\n,x", "aaaa\naaab\nbaaa", "xaaaaaaaay\nb",
        "b\n\n\nb", "abababab", "a\n\nab\n\n", "x,x\nxx\n,x,\n",
    };
    for ( const auto* pattern : patterns ) {
        for ( const bool fold : { false, true } ) {
            const auto regex = compiled( pattern, fold );
            for ( const auto* raw : texts ) {
                const std::string text( raw );
                for ( const size_t chunk : { size_t( 0 ), size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 5 ) } ) {
                    currentCase = std::string( pattern ) + " on a text of " + std::to_string( text.size() ) + " bytes, chunk "
                                  + std::to_string( chunk );
                    checkCuts( regex, text, '\n', {}, chunk );
                    for ( size_t a = 0; a <= text.size(); ++a ) {
                        checkCuts( regex, text, '\n', { a }, chunk );
                        for ( size_t b = a; b <= text.size(); ++b ) checkCuts( regex, text, '\n', { a, b }, chunk );
                    }
                }
            }
        }
    }
    testSummariesBeyondFourGiB( patterns, sizeof( patterns ) / sizeof( patterns[0] ), texts, sizeof( texts ) / sizeof( texts[0] ) );
    currentCase = "another delimiter";
    {
        const auto regex = compiled( "^a+$" );
        const std::string text( "aa;b;a;;aaa" );
        for ( size_t a = 0; a <= text.size(); ++a ) checkCuts( regex, text, ';', { a }, 2 );
    }
    currentCase = "stretches that do not follow one another";
    {
        const auto regex = compiled( "a" );
        std::vector<Stretch> stretches( 2 );
        stretches[0].size = 3;
        stretches[1].fileOffset = 4;
        bool thrown = false;
        try {
            (void)stitchSummaries( regex, stretches, nullptr );
        } catch ( const std::invalid_argument& ) {
            thrown = true;
        }
        CHECK( thrown );
    }
}
}  // namespace

int
main()
{
    testCompiler();
    testRefusals();
    testSummaries();
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "regex ok\n" );
    return 0;
}
