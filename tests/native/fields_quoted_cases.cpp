/**
 * fields_quoted_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldquote.hpp on the CPU, as a program of its own that the test
 * suite builds with -fsanitize=address,undefined: known answers, summariseQuotedFields against a naive walk of the
 * definition and independent of the chunk size, stitchQuotedFields over every 2- and 3-way cut of small texts, the
 * scanned element's composition against a walk over random three-way splits, field 1023 behind 1 024 counted delimiters
 * with more inside quotes, the content rule and the refusals.
 */
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fieldquote.hpp"

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
using Bytes = std::vector<uint8_t>;
constexpr uint8_t NL = '\n', DL = ',', Q = '"';

Bytes
bytesOf( const std::string& s )
{
    return Bytes( s.begin(), s.end() );
}

/** Raw field j of the content data[s, end), by the definition's loop. */
FieldSpan
naiveField( const Bytes& data, size_t s, size_t end, uint8_t dl, uint8_t q, uint32_t j )
{
    std::vector<std::pair<size_t, size_t> > parts;   /* begin, size */
    size_t from = s;
    bool inq = false;
    for ( size_t at = s; at < end; ++at ) {
        if ( data[at] == q ) {
            inq = !inq;
        } else if ( data[at] == dl && !inq ) {
            parts.emplace_back( from, at - from );
            from = at + 1;
        }
    }
    parts.emplace_back( from, end - from );
    if ( j >= parts.size() ) return { end, -1 };
    return { parts[j].first, (int64_t)parts[j].second };
}

/** Raw field j of every line of `data`; a non-empty unterminated tail is one more line. */
std::vector<FieldSpan>
direct( const Bytes& data, uint8_t nl, uint8_t dl, uint8_t q, uint32_t j )
{
    std::vector<FieldSpan> fields;
    size_t from = 0;
    for ( size_t at = 0; at < data.size(); ++at ) {
        if ( data[at] != nl ) continue;
        fields.push_back( naiveField( data, from, at, dl, q, j ) );
        from = at + 1;
    }
    if ( from < data.size() ) fields.push_back( naiveField( data, from, data.size(), dl, q, j ) );
    return fields;
}

FieldSpan
contentOf( const Bytes& data, const FieldSpan& raw, uint8_t q )
{
    if ( raw.size < 2 ) return raw;
    return quotedFieldContent( raw, data[raw.start], data[raw.start + raw.size - 1], q );
}

bool
same( const QuotedFieldSummary& a, const QuotedFieldSummary& b )
{
    return a.size == b.size && a.hasDelimiter == b.hasDelimiter && a.tailNonEmpty == b.tailNonEmpty && a.count == b.count
           && a.firstNl == b.firstNl && a.headPositions[0] == b.headPositions[0] && a.headPositions[1] == b.headPositions[1]
           && a.headQuoteParity == b.headQuoteParity && a.tailStart == b.tailStart && a.tailDelims == b.tailDelims
           && a.tailFieldStart == b.tailFieldStart && a.tailFieldEnd == b.tailFieldEnd && a.tailInQuote == b.tailInQuote
           && a.starts == b.starts && a.sizes == b.sizes;
}

/** The texts the cases walk: empty fields, "", """", a lone quote, an unbalanced quote followed by further lines, quotes
 * next to delimiters, delimiters only inside quotes, a missing field, and an unterminated tail open inside a quote. */
std::vector<Bytes>
texts()
{
    return { bytesOf( "" ),
             bytesOf( "\n" ),
             bytesOf( "a,b,c\n" ),
             bytesOf( ",,\n,\n\n" ),
             bytesOf( "\"\",\"\"\"\",x\n" ),
             bytesOf( "\",a,b\nc,d\n" ),
             bytesOf( "a,\"b,c\",d\n\"x\ny,z\"\nlast,\"open, tail" ),
             bytesOf( "\"a\",\"b\"\n\",\",\",,\"\nq\"r,s\"t\n" ),
             bytesOf( "\",,,,\"\n\"a,b\"\n" ),
             bytesOf( "one\n\"two\"\n,\"\"\n" ),
             bytesOf( "x,\"y\"\"z\",\"\"\"\"\nw\"" ) };
}

std::vector<FieldSpan>
listed( const QuotedFieldSummary& s, uint32_t j )
{
    std::vector<QuotedFieldStretch> one( 1 );
    one[0].summary = s;
    return stitchedQuotedFields( one, j );
}

void
knownAnswers()
{
    const Bytes text = bytesOf( "a,\"b,c\",d\n\"x\ny,z\"\nlast,\"open, tail" );
    /* lines: a,"b,c",d at 0; "x at 10; y,z" at 13; last,"open, tail at 18 */
    const auto raw = [&] ( uint32_t j ) { return direct( text, NL, DL, Q, j ); };
    CHECK( ( raw( 0 ) == std::vector<FieldSpan>{ { 0, 1 }, { 10, 2 }, { 13, 1 }, { 18, 4 } } ) );
    CHECK( ( raw( 1 ) == std::vector<FieldSpan>{ { 2, 5 }, { 12, -1 }, { 15, 2 }, { 23, 11 } } ) );
    CHECK( ( raw( 2 ) == std::vector<FieldSpan>{ { 8, 1 }, { 12, -1 }, { 17, -1 }, { 34, -1 } } ) );
    CHECK( ( contentOf( text, { 2, 5 }, Q ) == FieldSpan{ 3, 3 } ) );         /* "b,c" */
    CHECK( ( contentOf( text, { 10, 2 }, Q ) == FieldSpan{ 10, 2 } ) );       /* "x: one quote */
    CHECK( ( contentOf( text, { 23, 11 }, Q ) == FieldSpan{ 23, 11 } ) );
    /* the content rule on its own */
    CHECK( ( quotedFieldContent( { 5, 2 }, Q, Q, Q ) == FieldSpan{ 6, 0 } ) );        /* "" */
    CHECK( ( quotedFieldContent( { 5, 1 }, Q, Q, Q ) == FieldSpan{ 5, 1 } ) );        /* a lone quote */
    CHECK( ( quotedFieldContent( { 5, 4 }, Q, Q, Q ) == FieldSpan{ 6, 2 } ) );        /* """" keeps its doubled quote */
    CHECK( ( quotedFieldContent( { 5, 3 }, Q, 'a', Q ) == FieldSpan{ 5, 3 } ) );
    CHECK( ( quotedFieldContent( { 5, 3 }, 'a', Q, Q ) == FieldSpan{ 5, 3 } ) );
    CHECK( ( quotedFieldContent( { 5, -1 }, Q, Q, Q ) == FieldSpan{ 5, -1 } ) );
    CHECK( ( quotedFieldContent( { 5, 0 }, Q, Q, Q ) == FieldSpan{ 5, 0 } ) );
    for ( uint32_t j = 0; j < 4; ++j ) {
        std::vector<QuotedFieldStretch> one( 1 );
        one[0].summary = summariseQuotedFields( text.data(), text.size(), NL, DL, Q, j, 3 );
        CHECK( stitchedQuotedFields( one, j ) == raw( j ) );
    }
    const auto s = summariseQuotedFields( text.data(), text.size(), NL, DL, Q, 1, 4 );
    CHECK( s.tailInQuote && s.tailNonEmpty && s.tailDelims == 1 && s.tailFieldStart == 23 && s.tailFieldEnd == FIELD_UNKNOWN );
    CHECK( !s.headQuoteParity && ( s.headPositions[0] == std::vector<uint64_t>{ 1, 7 } ) && ( s.headPositions[1] == std::vector<uint64_t>{ 4 } ) );
    CHECK( quotedFieldArgumentsError( NL, DL, Q, 1023 ).empty() && !quotedFieldArgumentsError( NL, DL, Q, 1024 ).empty() );
    CHECK( !quotedFieldArgumentsError( NL, DL, NL, 0 ).empty() && !quotedFieldArgumentsError( NL, DL, DL, 0 ).empty() );
    CHECK( !quotedFieldArgumentsError( NL, NL, Q, 0 ).empty() );
}

void
chunkSizes( std::mt19937_64& rng )
{
    auto all = texts();
    const uint8_t alphabet[] = { 'a', DL, NL, Q, Q, DL, 'b', DL };
    for ( int round = 0; round < 300; ++round ) {
        Bytes data( rng() % 160 );
        for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
        all.push_back( std::move( data ) );
    }
    for ( const auto& data : all ) {
        for ( const uint32_t j : { 0u, 1u, 2u, 5u, 1023u } ) {
            const auto whole = summariseQuotedFieldChunk( data.data(), data.size(), NL, DL, Q, j );
            for ( const size_t chunk : { size_t( 1 ), size_t( 2 ), size_t( 3 ), size_t( 7 ), size_t( 256 ), data.size() + 1 } ) {
                CHECK( same( summariseQuotedFields( data.data(), data.size(), NL, DL, Q, j, chunk ), whole ) );
            }
            CHECK( whole.headDelims( 0 ) <= j + 1 && whole.headDelims( 1 ) <= j + 1 && whole.tailDelims <= j + 1 );
            /* one stretch from offset 0 is the file */
            const auto want = direct( data, NL, DL, Q, j );
            CHECK( listed( whole, j ) == want );
            CHECK( whole.count + ( whole.tailNonEmpty ? 1 : 0 ) == want.size() );
        }
    }
    try {
        (void)summariseQuotedFields( nullptr, 0, NL, DL, Q, 0, 0 );
        CHECK( false );
    } catch ( const std::invalid_argument& ) {}
}

std::vector<FieldSpan>
stitchedCuts( const Bytes& data, const std::vector<size_t>& cuts, uint32_t j, size_t chunk )
{
    std::vector<QuotedFieldStretch> stretches;
    for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
        QuotedFieldStretch stretch;
        stretch.fileOffset = cuts[k];
        stretch.summary = summariseQuotedFields( data.data() + cuts[k], cuts[k + 1] - cuts[k], NL, DL, Q, j, chunk );
        stretches.push_back( std::move( stretch ) );
    }
    return stitchedQuotedFields( stretches, j );
}

/** Every 2- and 3-way cut of the small texts: the stitched stretches are the whole. */
void
everyCut()
{
    for ( const auto& data : texts() ) {
        for ( const uint32_t j : { 0u, 1u, 2u, 3u } ) {
            const auto want = direct( data, NL, DL, Q, j );
            for ( size_t a = 0; a <= data.size(); ++a ) {
                CHECK( stitchedCuts( data, { 0, a, data.size() }, j, 2 ) == want );
                for ( size_t b = a; b <= data.size(); ++b ) CHECK( stitchedCuts( data, { 0, a, b, data.size() }, j, 3 ) == want );
            }
        }
    }
}

/** The scanned element: both bracketings of a three-way split equal the walk of the whole. */
void
elements( std::mt19937_64& rng )
{
    const uint8_t alphabet[] = { 'a', DL, NL, Q, Q, DL, DL, 'b', DL, DL };
    for ( int round = 0; round < 20000; ++round ) {
        const uint32_t cap = std::vector<uint32_t>{ 1, 2, 3, 5 }[round % 4];
        Bytes data( rng() % 24 );
        for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
        const size_t x = rng() % ( data.size() + 1 ), y = rng() % ( data.size() + 1 );
        const size_t a = std::min( x, y ), b = std::max( x, y );
        const auto of = [&] ( size_t from, size_t to ) { return quotedElementOf( data.data() + from, to - from, NL, DL, Q, cap ); };
        const auto whole = of( 0, data.size() );
        CHECK( composeQuotedElement( composeQuotedElement( of( 0, a ), of( a, b ), cap ), of( b, data.size() ), cap ) == whole );
        CHECK( composeQuotedElement( of( 0, a ), composeQuotedElement( of( a, b ), of( b, data.size() ), cap ), cap ) == whole );
        CHECK( !whole.reset || whole.a1 == whole.a0 );
        /* and the element is what the summary's tail says of a stretch entered outside */
        const auto s = summariseQuotedFieldChunk( data.data(), data.size(), NL, DL, Q, cap - 1 );
        CHECK( whole.reset == s.hasDelimiter && whole.p == s.tailInQuote && whole.a0 == s.tailDelims );
        if ( !whole.reset ) CHECK( whole.a1 == s.headDelims( 1 ) && whole.a0 == s.headDelims( 0 ) );
    }
}

/** j = 1023: 1 024 counted delimiters, and in between quoted stretches full of delimiters that do not count. */
void
saturation()
{
    Bytes line;
    std::vector<uint64_t> countedAt;
    for ( int i = 0; i < 1024; ++i ) {
        if ( i % 100 == 7 ) {
            const auto quoted = bytesOf( "\",,,,,,,x,,\"" );
            line.insert( line.end(), quoted.begin(), quoted.end() );
        } else {
            line.push_back( 'a' + i % 3 );
        }
        countedAt.push_back( line.size() );
        line.push_back( DL );
    }
    const auto rest = bytesOf( "\"the,last\"" );
    line.insert( line.end(), rest.begin(), rest.end() );
    line.push_back( NL );
    CHECK( countedAt.size() == 1024 );
    for ( const size_t chunk : { size_t( 1 ), size_t( 5 ), size_t( 256 ), size_t( 100000 ) } ) {
        const auto s = summariseQuotedFields( line.data(), line.size(), NL, DL, Q, 1023, chunk );
        CHECK( s.headPositions[0] == countedAt && s.count == 1 && s.tailDelims == 0 && !s.headQuoteParity );
        CHECK( s.starts[0] == countedAt[1022] + 1 && s.sizes[0] == 1 );
        const auto first = summariseQuotedFields( line.data(), line.size(), NL, DL, Q, 7, chunk );
        CHECK( first.starts[0] == countedAt[6] + 1 && first.sizes[0] == 12 );        /* the quoted field with its quotes */
        CHECK( ( contentOf( line, { first.starts[0], first.sizes[0] }, Q ) == FieldSpan{ countedAt[6] + 2, 10 } ) );
    }
    /* 1 024 delimiters in front of it: field 1024 would be the last one, and 1023 is the cap */
    const auto want = direct( line, NL, DL, Q, 1023 );
    CHECK( want.size() == 1 && want[0].size == 1 );
    for ( size_t a = 0; a <= line.size(); a += 97 ) CHECK( stitchedCuts( line, { 0, a, line.size() }, 1023, 64 ) == want );
    /* the same line without its nl, cut inside a quoted stretch: the tail saturates and both head lists are full */
    line.pop_back();
    const auto open = summariseQuotedFields( line.data(), line.size(), NL, DL, Q, 1023, 33 );
    CHECK( !open.hasDelimiter && open.tailDelims == 1024 && open.tailNonEmpty && !open.tailInQuote );
    CHECK( open.headDelims( 0 ) == 1024 && open.headDelims( 1 ) > 0 );
}

template<typename Call>
bool
refused( const Call& call )
{
    try {
        call();
    } catch ( const std::invalid_argument& ) {
        return true;
    }
    return false;
}

void
refusals()
{
    const auto nothing = [] ( uint64_t, const FieldSpan& ) {};
    const Bytes text = bytesOf( "a,\",\ncd" );
    std::vector<QuotedFieldStretch> stretches( 2 );
    stretches[0].summary = summariseQuotedFields( text.data(), 5, NL, DL, Q, 1, 2 );
    stretches[1].fileOffset = 5;
    stretches[1].summary = summariseQuotedFields( text.data() + 5, 2, NL, DL, Q, 1, 2 );
    CHECK( !refused( [&] { (void)stitchQuotedFields( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 6;    /* a gap */
    CHECK( refused( [&] { (void)stitchQuotedFields( stretches, 1, nothing ); } ) );
    stretches[1].fileOffset = 5;
    stretches[0].summary.headPositions[1] = { 1, 2, 3 };    /* too many positions under the second hypothesis */
    CHECK( refused( [&] { (void)stitchQuotedFields( stretches, 1, nothing ); } ) );
    stretches[0].summary.headPositions[1].clear();
    stretches[0].summary.starts.clear();        /* a count without its lines cannot be listed */
    CHECK( refused( [&] { (void)stitchedQuotedFields( stretches, 1 ); } ) );
    stretches[0].summary.count = 0;             /* a delimiter that closes no line */
    CHECK( refused( [&] { (void)stitchQuotedFields( stretches, 1, nothing ); } ) );
}
}  // namespace

int
main()
{
    std::mt19937_64 rng( 0xC5F );
    knownAnswers();
    chunkSizes( rng );
    everyCut();
    elements( rng );
    saturation();
    refusals();
    std::puts( "quoted fields cases ok" );
    return 0;
}
