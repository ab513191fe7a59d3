/**
 * bz2_regex.hpp -- the lines of the decoded file that match a regular expression (mi355x_bz2_reader_grep_regex): the
 * compiler from a pattern to a small DFA, the summary of a stretch of bytes under that DFA, and the rule that stitches
 * the summaries of stretches that lie back to back.  Host code only, no HIP: the reader and the context call it, and
 * tests/native/regex_cases.cpp pins it on the CPU.
 *
 * Semantics (D = the decoded file, nl = the delimiter byte): the content of a line is its bytes without the closing nl;
 * the unterminated tail is a line only if it is non-empty.  A line matches iff Python's re.search( pattern, content,
 * re.DOTALL ) on bytes finds a match (with SEARCH_IGNORE_CASE: re.IGNORECASE, which folds ASCII letters only).  The
 * syntax is a subset of Python's; compileRegex lists it.  What is outside the subset is refused, never reinterpreted.
 *
 * The automaton: a DFA over bytes with n <= REGEX_MAX_STATES states, uint8 transitions[n][256] and acceptsAtEnd[n].
 *   state 0  the start of a line.  No transition leads to it and minimisation merges it with nothing, so "the state is
 *            0" means "no byte since the last nl";
 *   state 1  A, "this line has matched": absorbing, acceptsAtEnd[A] is true.
 * The search is unanchored: every step re-enters the pattern's start through a closure in which `^` is false; `^` holds
 * in the closure of state 0 only.  `$` is decided by acceptsAtEnd.  A pattern that matches the empty string at the start
 * of a line has acceptsAtEnd[0] and every byte leads 0 -> A.  The table does not know nl: transitions on nl are never
 * taken, the summaries treat nl themselves.
 *
 * A DFA is sequential, the bytes lie in launches that run in any order, and inside a launch in chunks of one lane each.
 * Two facts make the run parallel: the automaton restarts at every nl, so a stretch that holds an nl leaves it in a
 * state that does not depend on the state it was entered in; and stretches without nl compose as functions state ->
 * state, which is associative and can be scanned.  One rule serves between the chunks of a span (k_regex_link, and
 * summarise here) and between the launches of a file (stitchSummaries):
 *
 *   The HEAD of a stretch S is the bytes in front of its first nl, all of S if it has none.  The summary of S:
 *     headMap[q]     the state behind the head for every entry state q;
 *     hasDelimiter;
 *     exit           the state behind the bytes that follow the last nl, run from 0 (only with hasDelimiter);
 *     body witnesses for every line that STARTS inside S: the offset of the byte that takes the state from != A to A,
 *                    else the offset of the closing nl if the state there is != A and acceptsAtEnd.  At most one per
 *                    line, inside its line, ascending.
 *   Stitching S_0, S_1, ... that lie back to back, e_0 = 0:
 *     the head line of S_i is reported iff e_i != A and ( headMap_i[e_i] == A, or hasDelimiter_i and
 *     acceptsAtEnd[headMap_i[e_i]] ); its witness is the first byte of S_i; then S_i's body witnesses follow;
 *     e_{i+1} = hasDelimiter_i ? exit_i : headMap_i[e_i];
 *     at the end of D, the final state f != A and != 0 with acceptsAtEnd[f] reports the unterminated tail at size - 1
 *     (f != 0 says that D is non-empty and does not end in nl).
 *   Every matching line gets exactly one witness, and the witnesses ascend: a line is reported where the state first
 *   becomes A (in the stretch that holds that byte: as a body witness if the line started there, else as that stretch's
 *   head hit -- later stretches are entered in A and report nothing) or at its closing nl.
 */
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <map>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "bz2_search.hpp"

namespace bz2gpu
{
constexpr uint32_t REGEX_MAX_STATES = 64;
constexpr uint32_t REGEX_MAX_PATTERN = 4096;
constexpr uint32_t REGEX_CHUNK_BYTES = 256;       /* of the kernels (bz2_regex.hip.h says why), for mi355x_bz2_regex_chunk_bytes */
constexpr uint32_t REGEX_MAX_COUNT = 255;         /* of {m,n} */
constexpr uint32_t REGEX_MAX_NFA_STATES = 8192;   /* the pattern with its repetitions written out */
constexpr uint32_t REGEX_MAX_RAW_STATES = 2048;   /* of the subset construction, before minimisation */
constexpr uint64_t REGEX_MAX_WORK = 1ull << 26;   /* NFA states visited by the subset construction */
constexpr uint8_t REGEX_START = 0, REGEX_MATCHED = 1;

struct Regex
{
    uint32_t n{ 0 };                       /* states */
    std::vector<uint8_t> transitions;      /* [n][256] */
    std::vector<uint8_t> acceptsAtEnd;     /* [n] */
    bool fold{ false };
};

namespace regex_detail
{
struct ByteClass
{
    std::array<uint64_t, 4> bits{};

    void set( uint32_t b ) { bits[b >> 6] |= uint64_t( 1 ) << ( b & 63 ); }
    [[nodiscard]] bool has( uint32_t b ) const { return ( bits[b >> 6] >> ( b & 63 ) & 1 ) != 0; }
    void setRange( uint32_t lo, uint32_t hi ) { for ( uint32_t b = lo; b <= hi; ++b ) set( b ); }
    void add( const ByteClass& other ) { for ( int i = 0; i < 4; ++i ) bits[i] |= other.bits[i]; }
    void invert() { for ( auto& word : bits ) word = ~word; }

    /** A byte is in the class iff it or its other-case ASCII twin is. */
    void
    foldCase()
    {
        for ( uint32_t b = 'a'; b <= 'z'; ++b ) {
            if ( has( b ) || has( b - 32 ) ) {
                set( b );
                set( b - 32 );
            }
        }
    }
};

enum class NodeKind { EMPTY, CLASS, BOL, EOL, CAT, ALT, REPEAT };
constexpr uint32_t UNBOUNDED = ~uint32_t( 0 );

struct Node
{
    NodeKind kind{ NodeKind::EMPTY };
    ByteClass bytes;                         /* CLASS */
    std::vector<std::unique_ptr<Node> > children;
    uint32_t min{ 0 }, max{ 0 };             /* REPEAT */
};

[[noreturn]] inline void
refuse( const std::string& what, size_t at )
{
    throw std::invalid_argument( "regex: " + what + " at offset " + std::to_string( at ) );
}

inline ByteClass
classOfEscape( uint8_t letter )
{
    ByteClass c;
    switch ( letter | 0x20 ) {
    case 'd': c.setRange( '0', '9' ); break;
    case 'w': c.setRange( '0', '9' ); c.setRange( 'a', 'z' ); c.setRange( 'A', 'Z' ); c.set( '_' ); break;
    default: for ( const uint8_t b : { ' ', '\t', '\n', '\r', '\f', '\v' } ) c.set( b ); break;   /* 's' */
    }
    if ( letter < 'a' ) c.invert();
    return c;
}

class Parser
{
public:
    Parser( const uint8_t* pattern, size_t size, bool fold ) : m_p( pattern ), m_size( size ), m_fold( fold ) {}

    std::unique_ptr<Node>
    parse()
    {
        auto node = alternation();
        if ( m_at < m_size ) refuse( "unbalanced ')'", m_at );
        return node;
    }

private:
    [[nodiscard]] bool more() const { return m_at < m_size; }
    [[nodiscard]] uint8_t peek() const { return m_p[m_at]; }

    static bool isPunctuation( uint8_t b ) { return b > 0x20 && b < 0x7F && !isAlnum( b ); }
    static bool isAlnum( uint8_t b ) { return ( b >= '0' && b <= '9' ) || ( ( b | 0x20 ) >= 'a' && ( b | 0x20 ) <= 'z' ); }
    static int hexOf( uint8_t b ) { return b >= '0' && b <= '9' ? b - '0' : ( b | 0x20 ) >= 'a' && ( b | 0x20 ) <= 'f' ? ( b | 0x20 ) - 'a' + 10 : -1; }

    std::unique_ptr<Node>
    classNode( ByteClass bytes, bool negated )
    {
        if ( m_fold ) bytes.foldCase();
        if ( negated ) bytes.invert();
        auto node = std::make_unique<Node>();
        node->kind = NodeKind::CLASS;
        node->bytes = bytes;
        return node;
    }

    std::unique_ptr<Node>
    alternation()
    {
        auto alt = std::make_unique<Node>();
        alt->kind = NodeKind::ALT;
        alt->children.push_back( sequence() );
        while ( more() && peek() == '|' ) {
            ++m_at;
            alt->children.push_back( sequence() );
        }
        if ( alt->children.size() == 1 ) return std::move( alt->children[0] );
        return alt;
    }

    std::unique_ptr<Node>
    sequence()
    {
        auto cat = std::make_unique<Node>();
        cat->kind = NodeKind::CAT;
        while ( more() && peek() != '|' && peek() != ')' ) {
            bool repeatable = true;
            auto item = atom( &repeatable );
            if ( more() && isQuantifier() ) {
                if ( !repeatable ) refuse( "nothing to repeat", m_at );
                item = quantified( std::move( item ) );
                if ( more() && peek() == '?' ) refuse( "lazy quantifier", m_at );
                if ( more() && peek() == '+' ) refuse( "possessive quantifier", m_at );
                if ( more() && isQuantifier() ) refuse( "multiple repeat", m_at );
            }
            cat->children.push_back( std::move( item ) );
        }
        return cat;
    }

    [[nodiscard]] bool
    isQuantifier() const
    {
        const uint8_t b = peek();
        return b == '*' || b == '+' || b == '?' || b == '{';
    }

    /** The digits at m_at, UNBOUNDED if there are none. */
    uint32_t
    count()
    {
        if ( !more() || peek() < '0' || peek() > '9' ) return UNBOUNDED;
        const size_t from = m_at;
        uint32_t value = 0;
        while ( more() && peek() >= '0' && peek() <= '9' ) {
            value = value * 10 + ( peek() - '0' );
            if ( value > REGEX_MAX_COUNT ) refuse( "repetition count above " + std::to_string( REGEX_MAX_COUNT ), from );
            ++m_at;
        }
        return value;
    }

    std::unique_ptr<Node>
    quantified( std::unique_ptr<Node> item )
    {
        auto node = std::make_unique<Node>();
        node->kind = NodeKind::REPEAT;
        const size_t from = m_at;
        const uint8_t q = m_p[m_at++];
        if ( q == '*' ) {
            node->min = 0, node->max = UNBOUNDED;
        } else if ( q == '+' ) {
            node->min = 1, node->max = UNBOUNDED;
        } else if ( q == '?' ) {
            node->min = 0, node->max = 1;
        } else {
            /* {m} {m,} {m,n} {,n}; every other '{' is a literal to Python, and is refused here */
            const uint32_t lo = count();
            uint32_t hi = lo;
            bool comma = false;
            if ( more() && peek() == ',' ) {
                comma = true;
                ++m_at;
                hi = count();
            }
            if ( !more() || peek() != '}' || ( lo == UNBOUNDED && ( !comma || hi == UNBOUNDED ) ) ) {
                refuse( "'{' that does not open {m}, {m,}, {m,n} or {,n} (escape a literal brace)", from );
            }
            ++m_at;
            node->min = lo == UNBOUNDED ? 0 : lo;
            node->max = hi;
            if ( node->max != UNBOUNDED && node->min > node->max ) refuse( "repetition with min above max", from );
        }
        node->children.push_back( std::move( item ) );
        return node;
    }

    /** The byte an escape stands for (m_at behind the backslash), or -1 with *set filled for \d \w \s \D \W \S. */
    int
    escape( ByteClass* set, bool inClass )
    {
        const size_t from = m_at - 1;
        if ( !more() ) refuse( "backslash at the end of the pattern", from );
        const uint8_t b = m_p[m_at++];
        switch ( b ) {
        case 'n': return '\n';
        case 'r': return '\r';
        case 't': return '\t';
        case 'f': return '\f';
        case 'v': return '\v';
        case '0':
            if ( more() && peek() >= '0' && peek() <= '9' ) refuse( "octal escape", from );
            return 0;
        case 'x': {
            if ( m_at + 2 > m_size || hexOf( m_p[m_at] ) < 0 || hexOf( m_p[m_at + 1] ) < 0 ) refuse( "incomplete \\xHH escape", from );
            const int value = hexOf( m_p[m_at] ) * 16 + hexOf( m_p[m_at + 1] );
            m_at += 2;
            return value;
        }
        case 'd': case 'D': case 'w': case 'W': case 's': case 'S':
            *set = classOfEscape( b );
            return -1;
        default: break;
        }
        if ( b >= '1' && b <= '9' ) refuse( "back-reference", from );
        if ( !inClass && ( b == 'b' || b == 'B' || b == 'A' || b == 'Z' ) ) refuse( std::string( "assertion \\" ) + (char)b, from );
        if ( isPunctuation( b ) ) return b;
        if ( isAlnum( b ) ) refuse( std::string( "escape \\" ) + (char)b, from );
        refuse( "backslash in front of a byte that is not ASCII punctuation", from );
    }

    std::unique_ptr<Node>
    bracket()
    {
        const size_t from = m_at - 1;
        bool negated = false;
        if ( more() && peek() == '^' ) {
            negated = true;
            ++m_at;
        }
        if ( more() && peek() == ']' ) refuse( "']' as the first member of a class (escape it)", m_at );
        ByteClass bytes;
        for ( ;; ) {
            if ( !more() ) refuse( "unterminated class", from );
            const size_t itemAt = m_at;
            uint8_t b = m_p[m_at++];
            if ( b == ']' ) break;
            ByteClass set;
            int lo = b;
            if ( b == '\\' ) lo = escape( &set, true );
            if ( more() && peek() == '-' && m_at + 1 < m_size && m_p[m_at + 1] != ']' ) {
                /* a range lo-hi */
                if ( lo < 0 ) refuse( "range that starts with a class escape", itemAt );
                ++m_at;
                int hi = m_p[m_at++];
                if ( hi == '\\' ) {
                    ByteClass ignored;
                    hi = escape( &ignored, true );
                    if ( hi < 0 ) refuse( "range that ends with a class escape", itemAt );
                }
                if ( hi < lo ) refuse( "range with its ends in the wrong order", itemAt );
                bytes.setRange( (uint32_t)lo, (uint32_t)hi );
            } else if ( lo < 0 ) {
                bytes.add( set );
            } else {
                bytes.set( (uint32_t)lo );
            }
        }
        return classNode( bytes, negated );
    }

    std::unique_ptr<Node>
    atom( bool* repeatable )
    {
        const size_t from = m_at;
        const uint8_t b = m_p[m_at++];
        auto node = std::make_unique<Node>();
        switch ( b ) {
        case '^':
            node->kind = NodeKind::BOL;
            *repeatable = false;
            return node;
        case '$':
            node->kind = NodeKind::EOL;
            *repeatable = false;
            return node;
        case '.': {
            ByteClass all;
            all.invert();
            return classNode( all, false );
        }
        case '*': case '+': case '?':
            refuse( "nothing to repeat", from );
        case '{':
            refuse( "'{' with nothing to repeat (escape a literal brace)", from );
        case '[':
            return bracket();
        case '(': {
            if ( more() && peek() == '?' ) {
                const uint8_t kind = m_at + 1 < m_size ? m_p[m_at + 1] : 0;
                if ( kind == ':' ) {
                    m_at += 2;
                } else if ( kind == '=' || kind == '!' || kind == '<' ) {
                    const uint8_t after = m_at + 2 < m_size ? m_p[m_at + 2] : 0;
                    if ( kind == '<' && after != '=' && after != '!' ) refuse( "named group", from );
                    refuse( "look-around", from );
                } else if ( kind == 'P' ) {
                    refuse( "named group", from );
                } else if ( kind == '#' ) {
                    refuse( "comment group", from );
                } else if ( kind == '(' ) {
                    refuse( "conditional group", from );
                } else if ( kind == '>' ) {
                    refuse( "atomic group", from );
                } else {
                    refuse( "inline flags", from );
                }
            }
            if ( ++m_depth > 200 ) refuse( "groups nested deeper than 200", from );
            auto inner = alternation();
            --m_depth;
            if ( !more() || peek() != ')' ) refuse( "unbalanced '('", from );
            ++m_at;
            return inner;
        }
        case '\\': {
            ByteClass set;
            const int value = escape( &set, false );
            if ( value < 0 ) return classNode( set, false );
            ByteClass one;
            one.set( (uint32_t)value );
            return classNode( one, false );
        }
        default: {
            ByteClass one;
            one.set( b );
            return classNode( one, false );
        }
        }
    }

    const uint8_t* m_p;
    size_t m_size, m_at{ 0 };
    bool m_fold;
    uint32_t m_depth{ 0 };
};

/* Thompson's construction.  An NFA state has any number of empty edges -- plain, or passable only at the start of a line
 * (BOL) or at its end (EOL) -- and at most one edge on a class of bytes. */
enum : uint8_t { EDGE_PLAIN = 0, EDGE_BOL = 1, EDGE_EOL = 2 };

struct NfaState
{
    std::vector<std::pair<uint32_t, uint8_t> > empty;   /* target, kind */
    int32_t bytes{ -1 };                                 /* index into Nfa::classes */
    uint32_t next{ 0 };
};

struct Nfa
{
    std::vector<NfaState> states;
    std::vector<ByteClass> classes;
    uint32_t start{ 0 }, accept{ 0 };

    uint32_t
    add()
    {
        if ( states.size() >= REGEX_MAX_NFA_STATES ) {
            throw std::invalid_argument( "regex: the pattern with its repetitions written out needs more than "
                                         + std::to_string( REGEX_MAX_NFA_STATES ) + " NFA states" );
        }
        states.emplace_back();
        return (uint32_t)states.size() - 1;
    }

    void link( uint32_t from, uint32_t to, uint8_t kind = EDGE_PLAIN ) { states[from].empty.push_back( { to, kind } ); }

    /** The fragment of `node`: {entry, exit}. */
    std::pair<uint32_t, uint32_t>
    build( const Node& node )
    {
        const uint32_t in = add(), out = add();
        switch ( node.kind ) {
        case NodeKind::EMPTY: link( in, out ); break;
        case NodeKind::BOL: link( in, out, EDGE_BOL ); break;
        case NodeKind::EOL: link( in, out, EDGE_EOL ); break;
        case NodeKind::CLASS:
            classes.push_back( node.bytes );
            states[in].bytes = (int32_t)classes.size() - 1;
            states[in].next = out;
            break;
        case NodeKind::CAT: {
            uint32_t at = in;
            for ( const auto& child : node.children ) {
                const auto piece = build( *child );
                link( at, piece.first );
                at = piece.second;
            }
            link( at, out );
            break;
        }
        case NodeKind::ALT:
            for ( const auto& child : node.children ) {
                const auto piece = build( *child );
                link( in, piece.first );
                link( piece.second, out );
            }
            break;
        case NodeKind::REPEAT: {
            const Node& child = *node.children[0];
            uint32_t at = in;
            for ( uint32_t i = 0; i < node.min; ++i ) {
                const auto piece = build( child );
                link( at, piece.first );
                at = piece.second;
            }
            if ( node.max == UNBOUNDED ) {
                const auto piece = build( child );
                link( at, piece.first );
                link( piece.second, piece.first );
                link( piece.second, out );
                link( at, out );
            } else {
                for ( uint32_t i = node.min; i < node.max; ++i ) {
                    const auto piece = build( child );
                    link( at, out );
                    link( at, piece.first );
                    at = piece.second;
                }
                link( at, out );
            }
            break;
        }
        }
        return { in, out };
    }
};

class Subsets
{
public:
    explicit Subsets( const Nfa& nfa ) : m_nfa( nfa ), m_stamp( nfa.states.size(), 0 ) {}

    /** The sorted closure of `seeds` over the empty edges whose kind is in `kinds` (a bit per EDGE_*). */
    std::vector<uint32_t>
    closure( const std::vector<uint32_t>& seeds, uint32_t kinds )
    {
        ++m_round;
        std::vector<uint32_t> result, stack;
        for ( const auto s : seeds ) {
            if ( m_stamp[s] != m_round ) {
                m_stamp[s] = m_round;
                stack.push_back( s );
            }
        }
        while ( !stack.empty() ) {
            const uint32_t s = stack.back();
            stack.pop_back();
            result.push_back( s );
            if ( ++m_work > REGEX_MAX_WORK ) throw std::invalid_argument( "regex: the pattern is too complex to compile" );
            for ( const auto& edge : m_nfa.states[s].empty ) {
                if ( ( kinds >> edge.second & 1 ) != 0 && m_stamp[edge.first] != m_round ) {
                    m_stamp[edge.first] = m_round;
                    stack.push_back( edge.first );
                }
            }
        }
        std::sort( result.begin(), result.end() );
        return result;
    }

    [[nodiscard]] bool
    accepts( const std::vector<uint32_t>& set ) const
    {
        return std::binary_search( set.begin(), set.end(), m_nfa.accept );
    }

    /** Work done outside closure(): the budget is one. */
    void
    charge( uint64_t steps )
    {
        m_work += steps;
        if ( m_work > REGEX_MAX_WORK ) throw std::invalid_argument( "regex: the pattern is too complex to compile" );
    }

private:
    const Nfa& m_nfa;
    std::vector<uint32_t> m_stamp;
    uint32_t m_round{ 0 };
    uint64_t m_work{ 0 };
};
}  // namespace regex_detail

/**
 * The DFA of `pattern` as the header describes it.  Throws std::invalid_argument with a sentence that names the
 * construct and its offset for everything outside the subset, and for a pattern that needs more than REGEX_MAX_STATES
 * states (the sentence gives the count) or whose subset construction passes REGEX_MAX_RAW_STATES.
 *
 * Accepted: literal bytes (0x80 .. 0xFF included); a backslash in front of ASCII punctuation; \n \r \t \f \v \0 \xHH;
 * \d \D \w \W \s \S (ASCII); `.` (any byte); [...] and [^...] with ranges, escapes and \d \w \s inside (a `]` must be
 * escaped); ( ) and (?: ), both only grouping; |; * + ? {m} {m,} {m,n} {,n} with counts <= 255; ^ and $ anywhere.
 * Refused: back-references, look-around, inline flags, named groups, lazy and possessive quantifiers, \b \B \A \Z, every
 * other escape, a '{' that opens no repetition, an empty pattern, a pattern over REGEX_MAX_PATTERN bytes.
 * With `fold` a byte is in a class iff it or its other-case ASCII twin is; a negated class is the complement of that.
 */
inline Regex
compileRegex( const uint8_t* pattern, size_t size, bool fold )
{
    using namespace regex_detail;
    if ( size == 0 ) throw std::invalid_argument( "regex: empty pattern" );
    if ( size > REGEX_MAX_PATTERN ) {
        throw std::invalid_argument( "regex: pattern over " + std::to_string( REGEX_MAX_PATTERN ) + " bytes: " + std::to_string( size ) );
    }
    const auto tree = Parser( pattern, size, fold ).parse();
    Nfa nfa;
    const auto whole = nfa.build( *tree );
    nfa.start = whole.first;
    nfa.accept = whole.second;

    /* bytes that no class tells apart behave alike: one representative per group */
    std::vector<uint8_t> groupOf( 256 );
    std::vector<uint8_t> representative;
    {
        std::map<std::vector<bool>, uint8_t> seen;
        for ( uint32_t b = 0; b < 256; ++b ) {
            std::vector<bool> signature( nfa.classes.size() );
            for ( size_t c = 0; c < nfa.classes.size(); ++c ) signature[c] = nfa.classes[c].has( b );
            const auto found = seen.find( signature );
            if ( found == seen.end() ) {
                seen.emplace( std::move( signature ), (uint8_t)representative.size() );
                groupOf[b] = (uint8_t)representative.size();
                representative.push_back( (uint8_t)b );
            } else {
                groupOf[b] = found->second;
            }
        }
    }
    const size_t nGroups = representative.size();

    /* Subset construction.  Raw state 0 is the closure of the start in which ^ holds, raw state 1 is A; every other raw
     * state is a set reached by a byte, closed with ^ false and with the start re-entered. */
    constexpr uint32_t PLAIN = 1u << EDGE_PLAIN, BOL = 1u << EDGE_BOL, EOL = 1u << EDGE_EOL;
    Subsets subsets( nfa );
    std::vector<std::vector<uint32_t> > sets;
    std::vector<std::vector<uint32_t> > rawNext;   /* [state][group] */
    std::vector<uint8_t> rawAccepts;
    std::map<std::vector<uint32_t>, uint32_t> known;
    sets.push_back( subsets.closure( { nfa.start }, PLAIN | BOL ) );
    sets.emplace_back();   /* A */
    const bool emptyMatches = subsets.accepts( sets[0] );
    rawAccepts.push_back( subsets.accepts( subsets.closure( sets[0], PLAIN | BOL | EOL ) ) ? 1 : 0 );
    rawAccepts.push_back( 1 );
    rawNext.assign( 2, std::vector<uint32_t>( nGroups, REGEX_MATCHED ) );
    for ( uint32_t s = 0; s < sets.size(); ++s ) {
        if ( s == REGEX_MATCHED || ( s == REGEX_START && emptyMatches ) ) continue;
        for ( size_t g = 0; g < nGroups; ++g ) {
            std::vector<uint32_t> moved{ nfa.start };
            subsets.charge( sets[s].size() );
            for ( const auto q : sets[s] ) {
                const auto& state = nfa.states[q];
                if ( state.bytes >= 0 && nfa.classes[(size_t)state.bytes].has( representative[g] ) ) moved.push_back( state.next );
            }
            auto target = subsets.closure( moved, PLAIN );
            uint32_t id = REGEX_MATCHED;
            if ( !subsets.accepts( target ) ) {
                const auto found = known.find( target );
                if ( found != known.end() ) {
                    id = found->second;
                } else {
                    if ( sets.size() >= REGEX_MAX_RAW_STATES ) {
                        throw std::invalid_argument( "regex: the pattern needs more than " + std::to_string( REGEX_MAX_RAW_STATES )
                                                     + " states before minimisation; at most " + std::to_string( REGEX_MAX_STATES )
                                                     + " are allowed after it" );
                    }
                    id = (uint32_t)sets.size();
                    known.emplace( target, id );
                    rawAccepts.push_back( subsets.accepts( subsets.closure( target, PLAIN | EOL ) ) ? 1 : 0 );
                    sets.push_back( std::move( target ) );
                    rawNext.emplace_back( nGroups, REGEX_MATCHED );
                }
            }
            rawNext[s][g] = id;
        }
    }

    /* Minimisation by refinement: 0 and A each alone in a block of their own, the others split by acceptsAtEnd first. */
    const size_t raw = sets.size();
    std::vector<uint32_t> block( raw );
    for ( size_t s = 0; s < raw; ++s ) block[s] = s < 2 ? (uint32_t)s : 2 + rawAccepts[s];
    for ( size_t blocks = 0;; ) {
        std::map<std::vector<uint32_t>, uint32_t> byBehaviour;
        std::vector<uint32_t> refined( raw );
        for ( size_t s = 0; s < raw; ++s ) {
            std::vector<uint32_t> behaviour{ block[s] };
            for ( size_t g = 0; g < nGroups; ++g ) behaviour.push_back( block[rawNext[s][g]] );
            refined[s] = byBehaviour.emplace( std::move( behaviour ), (uint32_t)byBehaviour.size() ).first->second;
        }
        block = std::move( refined );
        if ( byBehaviour.size() == blocks ) break;
        blocks = byBehaviour.size();
    }
    /* numbered in the order of the raw states, which is the order of discovery: 0 stays 0 and A stays 1 */
    std::vector<int32_t> number( raw, -1 );
    std::vector<uint32_t> firstOf;
    std::vector<uint32_t> stateOf( raw );
    for ( size_t s = 0; s < raw; ++s ) {
        if ( number[block[s]] < 0 ) {
            number[block[s]] = (int32_t)firstOf.size();
            firstOf.push_back( (uint32_t)s );
        }
        stateOf[s] = (uint32_t)number[block[s]];
    }
    if ( firstOf.size() > REGEX_MAX_STATES ) {
        throw std::invalid_argument( "regex: the pattern needs " + std::to_string( firstOf.size() ) + " states, more than the "
                                     + std::to_string( REGEX_MAX_STATES ) + " allowed" );
    }
    Regex regex;
    regex.n = (uint32_t)firstOf.size();
    regex.fold = fold;
    regex.transitions.resize( (size_t)regex.n * 256 );
    regex.acceptsAtEnd.resize( regex.n );
    for ( uint32_t q = 0; q < regex.n; ++q ) {
        regex.acceptsAtEnd[q] = rawAccepts[firstOf[q]];
        for ( uint32_t b = 0; b < 256; ++b ) regex.transitions[(size_t)q * 256 + b] = (uint8_t)stateOf[rawNext[firstOf[q]][groupOf[b]]];
    }
    return regex;
}

/** The summary of a stretch (the header says what the fields mean).  headMap[q] is 0 for q >= n, exit is 0 without a
 * delimiter, and the witnesses are offsets from the base that summarise was given. */
struct StretchSummary
{
    std::array<uint8_t, REGEX_MAX_STATES> headMap{};
    bool hasDelimiter{ false };
    uint8_t exit{ 0 };
    uint64_t count{ 0 };                 /* body witnesses, whether or not they are listed */
    std::vector<uint64_t> witnesses;
};

/** The summary of one chunk, as k_regex_chunks computes it: the head for every entry state, the body once from 0. */
inline StretchSummary
summariseChunk( const Regex& regex, const uint8_t* bytes, size_t size, uint8_t nl, uint64_t base )
{
    StretchSummary s;
    for ( uint32_t q = 0; q < regex.n; ++q ) s.headMap[q] = (uint8_t)q;
    size_t at = 0;
    for ( ; at < size && bytes[at] != nl; ++at ) {
        for ( uint32_t q = 0; q < regex.n; ++q ) s.headMap[q] = regex.transitions[(size_t)s.headMap[q] * 256 + bytes[at]];
    }
    if ( at == size ) return s;
    s.hasDelimiter = true;
    uint8_t state = REGEX_START;
    for ( ++at; at < size; ++at ) {
        if ( bytes[at] == nl ) {
            if ( state != REGEX_MATCHED && regex.acceptsAtEnd[state] != 0 ) s.witnesses.push_back( base + at );
            state = REGEX_START;
            continue;
        }
        const uint8_t next = regex.transitions[(size_t)state * 256 + bytes[at]];
        if ( next == REGEX_MATCHED && state != REGEX_MATCHED ) s.witnesses.push_back( base + at );
        state = next;
    }
    s.exit = state;
    s.count = s.witnesses.size();
    return s;
}

/** True iff the head line of a stretch with this summary, entered in `entry`, is reported. */
[[nodiscard]] inline bool
headLineMatches( const Regex& regex, const StretchSummary& s, uint8_t entry )
{
    if ( entry == REGEX_MATCHED ) return false;
    const uint8_t behind = s.headMap[entry];
    return behind == REGEX_MATCHED || ( s.hasDelimiter && regex.acceptsAtEnd[behind] != 0 );
}

/**
 * The summary of bytes[0, size), cut into chunks of `chunk` bytes and composed as k_regex_link composes them: a chunk
 * behind the stretch's first delimiter is entered in the state the chunks in front of it leave, its head hit -- witness:
 * the chunk's first byte -- goes in front of its body witnesses; the chunks in front of the first delimiter report no head
 * hit, their line is the stretch's head line.  The result does not depend on `chunk`.  Witnesses are base + offset.
 */
inline StretchSummary
summarise( const Regex& regex, const uint8_t* bytes, size_t size, uint8_t nl, size_t chunk, uint64_t base = 0 )
{
    if ( chunk == 0 ) throw std::invalid_argument( "summarise: the chunk size must not be 0" );
    StretchSummary all;
    for ( uint32_t q = 0; q < regex.n; ++q ) all.headMap[q] = (uint8_t)q;
    for ( size_t at = 0; at < size; at += chunk ) {
        const auto part = summariseChunk( regex, bytes + at, std::min( chunk, size - at ), nl, base + at );
        if ( all.hasDelimiter ) {
            if ( headLineMatches( regex, part, all.exit ) ) all.witnesses.push_back( base + at );
            all.exit = part.hasDelimiter ? part.exit : part.headMap[all.exit];
        } else {
            for ( uint32_t q = 0; q < regex.n; ++q ) all.headMap[q] = part.headMap[all.headMap[q]];
            all.hasDelimiter = part.hasDelimiter;
            all.exit = part.exit;
        }
        all.witnesses.insert( all.witnesses.end(), part.witnesses.begin(), part.witnesses.end() );
    }
    all.count = all.witnesses.size();
    return all;
}

/** A stretch of D for stitchSummaries: where it lies and its summary, the witnesses as offsets in D (they may be
 * missing, or be fewer than `count`, where only the number of matching lines or their first few are wanted). */
struct Stretch
{
    uint64_t fileOffset{ 0 }, size{ 0 };
    StretchSummary summary;
};

/**
 * The rule of the header over stretches that lie back to back from offset 0 (checked: std::invalid_argument) and end at
 * the end of D.  Returns the number of matching lines; `witnesses`, if given, receives one offset inside every matching
 * line, ascending -- as far as the stretches list theirs.
 */
inline uint64_t
stitchSummaries( const Regex& regex, const std::vector<Stretch>& stretches, std::vector<uint64_t>* witnesses )
{
    uint64_t lines = 0, end = 0;
    uint8_t entry = REGEX_START;
    if ( witnesses != nullptr ) witnesses->clear();
    for ( size_t i = 0; i < stretches.size(); ++i ) {
        const auto& stretch = stretches[i];
        if ( stretch.fileOffset != end ) {
            throw std::invalid_argument( "stitchSummaries: stretch " + std::to_string( i ) + " does not follow the one in front of it" );
        }
        end += stretch.size;
        if ( stretch.size == 0 ) continue;
        if ( headLineMatches( regex, stretch.summary, entry ) ) {
            ++lines;
            if ( witnesses != nullptr ) witnesses->push_back( stretch.fileOffset );
        }
        lines += stretch.summary.count;
        if ( witnesses != nullptr ) {
            witnesses->insert( witnesses->end(), stretch.summary.witnesses.begin(), stretch.summary.witnesses.end() );
        }
        entry = stretch.summary.hasDelimiter ? stretch.summary.exit : stretch.summary.headMap[entry];
    }
    /* no transition leads to 0: entry != 0 says that D is non-empty and does not end in nl */
    if ( entry != REGEX_MATCHED && entry != REGEX_START && regex.acceptsAtEnd[entry] != 0 ) {
        ++lines;
        if ( witnesses != nullptr ) witnesses->push_back( end - 1 );
    }
    return lines;
}
}  // namespace bz2gpu
