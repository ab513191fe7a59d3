/* The per-symbol rule of k_mtf's data-parallel pass B (bz2_mtf_expand.hpp) against a byte-by-byte restatement of the serial
 * pass B (bz2_stage1.hip.h: one lane per chunk, runPos / hh in 32 bits with their wraps, the two overflow checks, "an open
 * run where the Huffman stage failed is never flushed").
 *
 * A block is a vector of symbols in the form pass A leaves (digits 0 and 1, literals 2 + position) cut into chunks by the
 * kernel's chunk rule, a list per chunk and the Huffman stage's verdict.  The rule expands every symbol by itself: its digit
 * index from the digit flags of the 24 symbols in front of its group of eight (groups aligned in the block, flags outside
 * the chunk zero: what the lanes of a wave hand each other), its byte from the nearest literal before it in the chunk.
 * For every block: if rule and restatement differ in any way (an error, the total, a byte), mtf_expand_fast_path must send
 * the block to the serial pass; and for the blocks built to be valid it must NOT, or the test would hold for a predicate
 * that is never true.  Prints "mtf expand ok". */
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_mtf_expand.hpp"

using namespace bz2gpu;

namespace
{
int failures = 0;
const char* currentCase = "";

#define CHECK( cond )                                                                          \
    do {                                                                                       \
        if ( !( cond ) ) {                                                                     \
            if ( failures < 20 ) std::printf( "FAILED line %d (%s): %s\n", __LINE__, currentCase, #cond ); \
            ++failures;                                                                        \
        }                                                                                      \
    } while ( 0 )

constexpr uint32_t MAX_N = 900000;
constexpr uint32_t ST_RUN_OVERFLOW = 12, ST_DATA_OVERFLOW = 13;
using Symbols = std::vector<uint16_t>;

/* the kernel's chunk rule: never inside a digit sequence */
std::vector<uint32_t>
chunkStarts( const Symbols& sym, uint32_t lanes )
{
    const uint32_t n = (uint32_t)sym.size();
    const uint32_t S = ( n + lanes - 1 ) / lanes;
    std::vector<uint32_t> starts;
    for ( uint32_t t = 0; t < lanes; ++t ) {
        uint32_t begin = t * S < n ? t * S : n;
        while ( begin < n && begin > 0 && sym[begin] <= 1 && sym[begin - 1] <= 1 ) ++begin;
        starts.push_back( begin );
    }
    starts.push_back( n );
    return starts;
}

/* byte of chunk c's list at position p: any fixed permutation per chunk will do */
uint8_t
listByte( uint32_t c, uint32_t p )
{
    return (uint8_t)( ( p * 167u + c * 29u + 3u ) & 0xFFu );    /* 167 is odd: a permutation of 0..255 */
}

struct Outcome
{
    std::vector<uint8_t> column;      /* bytes written, 0xEE where nothing was */
    std::vector<uint8_t> written;
    uint32_t error{ 0 };              /* the first in chunk order */
    unsigned long long total{ 0 };
    bool tooLong{ false };
    bool beyond{ false };             /* the rule wanted to write at or beyond MAX_N + 64 */

    Outcome() : column( MAX_N + 64, 0xEE ), written( MAX_N + 64, 0 ) {}

    void
    put( unsigned long long at, uint8_t byte )
    {
        if ( at >= column.size() ) { beyond = true; return; }
        column[at] = byte;
        written[at] = 1;
    }
};

/* pass A's count and digit flag, then the serial pass B, chunk by chunk, byte by byte */
void
serialBlock( const Symbols& sym, const std::vector<uint32_t>& starts, bool huffmanOk, Outcome& out )
{
    const uint32_t lanes = (uint32_t)starts.size() - 1, n = (uint32_t)sym.size();
    std::vector<unsigned long long> counts( lanes );
    for ( uint32_t c = 0; c < lanes; ++c ) {
        unsigned long long count = 0;
        uint32_t runPos = 0, hh = 0, weightsSeen = 0;
        for ( uint32_t i = starts[c]; i < starts[c + 1]; ++i ) {
            const uint32_t s = sym[i];
            if ( s <= 1 ) {
                if ( runPos == 0 ) { runPos = 1; hh = 0; }
                hh += runPos << s;
                runPos <<= 1;
                weightsSeen |= runPos;
                continue;
            }
            if ( runPos != 0 ) { count += hh; runPos = 0; }
            ++count;
        }
        if ( runPos != 0 ) count += hh;
        counts[c] = count;
        out.total += count;
        out.tooLong = out.tooLong || mtf_sequence_too_long( weightsSeen );
    }
    unsigned long long prefix = 0;
    for ( uint32_t c = 0; c < lanes; ++c ) {
        uint32_t o = prefix < MAX_N ? (uint32_t)prefix : MAX_N;
        prefix += counts[c];
        uint32_t front = 0, runPos = 0, hh = 0, err = 0;
        const uint32_t end = starts[c + 1];
        for ( uint32_t i = starts[c]; i < end && err == 0; ++i ) {
            const uint32_t s = sym[i];
            if ( s <= 1 ) {
                if ( runPos == 0 ) { runPos = 1; hh = 0; }
                hh += runPos << s;
                runPos <<= 1;
                continue;
            }
            if ( runPos != 0 ) {
                runPos = 0;
                if ( o + hh > MAX_N ) { err = ST_RUN_OVERFLOW; break; }
                for ( uint32_t k = 0; k < hh; ++k ) out.put( o++, listByte( c, front ) );
            }
            if ( o >= MAX_N ) { err = ST_DATA_OVERFLOW; break; }
            front = s - 2u;
            out.put( o++, listByte( c, front ) );
        }
        if ( err == 0 && runPos != 0 && ( end < n || huffmanOk ) ) {
            if ( o + hh > MAX_N ) {
                err = ST_RUN_OVERFLOW;
            } else {
                for ( uint32_t k = 0; k < hh; ++k ) out.put( o++, listByte( c, front ) );
            }
        }
        if ( err != 0 && out.error == 0 ) out.error = err;
    }
}

/* every symbol by itself */
void
ruleBlock( const Symbols& sym, const std::vector<uint32_t>& starts, Outcome& out, uint32_t& longestSequence )
{
    const uint32_t lanes = (uint32_t)starts.size() - 1;
    unsigned long long at = 0;
    longestSequence = 0;
    for ( uint32_t c = 0; c < lanes; ++c ) {
        const uint32_t begin = starts[c], end = starts[c + 1];
        const auto isDigit = [&] ( long long i ) { return i >= (long long)begin && i < (long long)end && sym[(size_t)i] <= 1; };
        uint32_t lastLiteral = 0, sequence = 0;
        for ( uint32_t i = begin; i < end; ++i ) {
            const uint32_t s = sym[i], j = i & 7u;
            const long long group = (long long)( i - j );
            uint32_t flags = 0;
            for ( int bit = 0; bit < 32; ++bit ) flags |= ( isDigit( group - 24 + bit ) ? 1u : 0u ) << bit;
            const uint32_t k = mtf_digit_index( flags, j );
            sequence = s <= 1 ? sequence + 1 : 0;
            longestSequence = sequence > longestSequence ? sequence : longestSequence;
            if ( sequence != 0 && sequence <= 24 ) CHECK( k == sequence - 1 );
            const uint32_t count = mtf_expand_count( s, k );
            const uint32_t source = mtf_expand_source( s, lastLiteral );
            lastLiteral = source;
            if ( at + count > out.column.size() ) {
                out.beyond = true;
                at += count;
                continue;
            }
            for ( uint32_t b = 0; b < count; ++b ) out.put( at++, listByte( c, source ) );
        }
    }
    out.total = at;
}

enum Expect { FAST, SERIAL, EITHER };

void
checkBlock( const char* name, const Symbols& sym, uint32_t lanes, bool huffmanOk, Expect expect )
{
    currentCase = name;
    const auto starts = chunkStarts( sym, lanes );
    Outcome serial, rule;
    uint32_t longest = 0;
    serialBlock( sym, starts, huffmanOk, serial );
    ruleBlock( sym, starts, rule, longest );
    CHECK( serial.tooLong == ( longest > MTF_EXPAND_MAX_DIGITS ) );
    CHECK( !serial.beyond );
    for ( size_t i = MAX_N; i < serial.written.size(); ++i ) CHECK( !serial.written[i] );
    const bool differ = serial.error != 0 || rule.beyond || rule.total != serial.total || rule.column != serial.column
                        || rule.written != serial.written;
    const bool fast = mtf_expand_fast_path( huffmanOk, serial.total, MAX_N, serial.tooLong, false );
    if ( differ ) CHECK( !fast );
    if ( expect == FAST ) { CHECK( fast ); CHECK( !differ ); }
    if ( expect == SERIAL ) { CHECK( !fast ); }
    CHECK( !mtf_expand_fast_path( huffmanOk, serial.total, MAX_N, serial.tooLong, true ) );
}

void
appendRun( Symbols& sym, unsigned long long count )     /* the digits of a run of `count` bytes */
{
    for ( unsigned long long v = count; v > 0; v = ( v - 1 ) / 2 ) sym.push_back( ( v & 1 ) ? 0 : 1 );
}

Symbols
seeded( uint32_t seed, uint32_t n, uint32_t maxDigits, uint32_t positions )
{
    std::mt19937 r( seed );
    Symbols sym;
    while ( sym.size() < n ) {
        const uint32_t kind = r() % 8;
        if ( kind < 3 ) {
            const uint32_t digits = 1 + r() % maxDigits;
            for ( uint32_t d = 0; d < digits; ++d ) sym.push_back( (uint16_t)( r() & 1u ) );
        }
        const uint32_t literals = 1 + r() % ( kind == 7 ? 40 : 4 );
        for ( uint32_t l = 0; l < literals; ++l ) sym.push_back( (uint16_t)( 2 + r() % positions ) );
    }
    if ( seed & 1 ) sym.push_back( 0 );      /* ends with an open run */
    return sym;
}
}  // namespace

int
main()
{
    /* seeded blocks: short runs, every alignment of a sequence to the groups of eight comes up; 1 to 300 chunks */
    for ( uint32_t seed = 1; seed <= 60; ++seed ) {
        const uint32_t lanes = seed % 5 == 0 ? 1 : ( seed % 3 == 0 ? 300 : 7 + seed );
        char name[64];
        std::snprintf( name, sizeof( name ), "seeded %u", seed );
        checkBlock( name, seeded( seed, 400 + 37 * seed, 1 + seed % 9, seed % 2 ? 256 : 128 ), lanes, true, FAST );
    }
    /* the same with a failed Huffman stage: the blocks that end with an open run differ there */
    for ( uint32_t seed = 1; seed <= 8; ++seed ) {
        checkBlock( "huffman failed", seeded( seed, 500, 5, 256 ), 16, false, SERIAL );
    }
    /* chunks that start with a run: at the block's start, and behind a literal on a chunk boundary */
    {
        Symbols sym;
        appendRun( sym, 37 );
        for ( uint32_t k = 0; k < 7; ++k ) { sym.push_back( (uint16_t)( 2 + k ) ); appendRun( sym, 5 + k ); }
        checkBlock( "run first", sym, 1, true, FAST );
        checkBlock( "run first, chunks", sym, 8, true, FAST );
        checkBlock( "run first, a chunk per symbol", sym, 256, true, FAST );
    }
    /* a chunk of digits only between chunks of literals: its byte is the front of ITS list */
    {
        Symbols sym( 30, 5 );
        for ( uint32_t k = 10; k < 20; ++k ) sym[k] = 0;
        checkBlock( "digits-only chunk", sym, 3, true, FAST );
    }
    /* sequences of d digits (all RUNA: 2^d - 1 bytes) at every offset in a group of eight, behind and in front of literals */
    for ( const uint32_t d : { 1u, 19u, 20u, 21u, 31u, 32u, 33u } ) {
        for ( uint32_t offset = 0; offset < 9; ++offset ) {
            Symbols sym( offset, 9 );
            for ( uint32_t k = 0; k < d; ++k ) sym.push_back( 0 );
            sym.push_back( 4 );
            sym.push_back( 1 );
            char name[64];
            std::snprintf( name, sizeof( name ), "%u digits at %u", d, offset );
            /* 20 RUNA digits are 1 048 575 bytes: serial by the total; from 21 on by the flag (33: the total wraps to a small one) */
            checkBlock( name, sym, 1, true, d <= 19 ? FAST : SERIAL );
            checkBlock( name, sym, 4, true, d <= 19 ? FAST : SERIAL );
        }
    }
    {
        /* 20 digits within MAX_N do not exist (the smallest are 2^20 - 1 bytes); 19 RUNB digits are 2^20 - 2: by the total */
        Symbols sym( 19, 1 );
        checkBlock( "19 RUNB", sym, 1, true, SERIAL );
        Symbols wrapped( 33, 0 );
        wrapped.push_back( 7 );
        Outcome o;
        serialBlock( wrapped, chunkStarts( wrapped, 1 ), true, o );
        currentCase = "33 digits";
        CHECK( o.total <= MAX_N && o.tooLong );      /* nothing but the flag keeps this block off the fast path */
    }
    /* totals of exactly MAX_N and MAX_N + 1 */
    {
        Symbols sym;
        appendRun( sym, MAX_N );
        checkBlock( "run of MAX_N", sym, 1, true, FAST );
        sym.clear();
        appendRun( sym, MAX_N - 1 );
        sym.push_back( 200 );
        checkBlock( "run of MAX_N - 1, literal", sym, 2, true, FAST );
        sym.clear();
        appendRun( sym, MAX_N + 1 );
        checkBlock( "run of MAX_N + 1", sym, 1, true, SERIAL );
        sym.clear();
        appendRun( sym, MAX_N );
        sym.push_back( 3 );
        checkBlock( "run of MAX_N, literal", sym, 2, true, SERIAL );
        sym.clear();
        for ( uint32_t k = 0; k < 3000; ++k ) { sym.push_back( (uint16_t)( 2 + k % 100 ) ); appendRun( sym, 299 ); }
        checkBlock( "3000 x (literal, run of 299) = MAX_N", sym, 256, true, FAST );
        sym.push_back( 2 );
        checkBlock( "... and a literal", sym, 256, true, SERIAL );
        sym.pop_back();
        sym.push_back( 0 );
        checkBlock( "... and a digit", sym, 256, true, SERIAL );
    }
    if ( failures != 0 ) {
        std::printf( "%d checks failed\n", failures );
        return 1;
    }
    std::printf( "mtf expand ok\n" );
    return 0;
}
