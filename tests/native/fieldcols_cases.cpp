/**
 * fieldcols_cases.cpp -- indexed_bzip2_amd/csrc/bz2_fieldcols.hpp on the CPU, as a program of its own that the test suite
 * builds with -fsanitize=address,undefined: the model of a column against known answers, planColumnAssembly executed over
 * per-stretch packs (summariseFields), the stitcher's patches (stitchFields) and fix-ups fetched from the text against the
 * model -- random texts, cuts, fields and windows of lines; a line through three stretches; patched lines with missing and
 * with empty fields; a tail; no lines at all --, its refusals, and sizes whose sum passes 2^32 (arithmetic only, no bytes)
 * with every destination offset checked against a 128-bit sum.
 */
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../../indexed_bzip2_amd/csrc/bz2_fields.hpp"
#include "../../indexed_bzip2_amd/csrc/bz2_fieldcols.hpp"

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

Bytes
bytesOf( const std::string& s )
{
    return Bytes( s.begin(), s.end() );
}

struct Assembled
{
    Bytes data;
    ColumnAssembly plan;
    uint64_t lines{ 0 };
    size_t patched{ 0 };
};

/** The column of the lines [first, first + count) of `data`, cut at `cuts` into stretches that are summarised with chunks
 * of `chunk` bytes: packs, patches, plan, and the plan carried out. */
Assembled
assemble( const Bytes& data, std::vector<size_t> cuts, uint8_t nl, uint8_t dl, uint32_t j, uint64_t first, uint64_t count, size_t chunk )
{
    cuts.insert( cuts.begin(), 0 );
    cuts.push_back( data.size() );
    std::sort( cuts.begin(), cuts.end() );
    std::vector<FieldStretch> stretches;
    for ( size_t k = 0; k + 1 < cuts.size(); ++k ) {
        stretches.push_back( { cuts[k], summariseFields( data.data() + cuts[k], cuts[k + 1] - cuts[k], nl, dl, j, chunk ) } );
    }
    uint64_t closed = 0;
    for ( const auto& stretch : stretches ) closed += stretch.summary.count;
    const uint64_t end = count > ~uint64_t( 0 ) - first ? ~uint64_t( 0 ) : first + count;
    const uint64_t wantedClosed = std::min( end, closed ) - std::min( first, closed );

    /* every stretch packs the wanted lines it closes, as it alone sees them */
    std::vector<ColumnStretch> places( stretches.size() );
    std::vector<Bytes> packs( stretches.size() );
    uint64_t before = 0;
    for ( size_t k = 0; k < stretches.size(); ++k ) {
        const auto& s = stretches[k].summary;
        const uint64_t lo = std::max( before, first ), hi = std::min( { before + s.count, end, closed } );
        if ( hi > lo ) {
            places[k].at = lo - first;
            places[k].take = hi - lo;
            for ( uint64_t i = lo - before; i < hi - before; ++i ) {
                const uint64_t size = s.sizes[i] > 0 ? (uint64_t)s.sizes[i] : 0;
                const uint8_t* const from = data.data() + stretches[k].fileOffset + ( size > 0 ? s.starts[i] : 0 );
                packs[k].insert( packs[k].end(), from, from + size );
                if ( i == lo - before ) places[k].firstSize = size;
            }
            places[k].total = packs[k].size();
        }
        before += s.count;
    }
    std::vector<ColumnPatch> patches;
    const auto stitched = stitchFields( stretches, j, [&] ( uint64_t k, const FieldSpan& field ) {
        if ( k >= first && k - first < wantedClosed ) patches.push_back( { k - first, field.start, field.size } );
    } );
    CHECK( stitched.closed == closed );
    Assembled result;
    result.lines = wantedClosed;
    if ( stitched.hasTail && first <= closed && closed < end ) patches.push_back( { result.lines++, stitched.tail.start, stitched.tail.size } );
    result.patched = patches.size();
    result.plan = planColumnAssembly( places, patches );

    /* the copies and the fix-ups tile [0, size) */
    result.data.assign( result.plan.size, 0 );
    std::vector<uint8_t> written( result.plan.size, 0 );
    const auto put = [&] ( const uint8_t* from, uint64_t dst, uint64_t size ) {
        CHECK( size <= result.plan.size && dst <= result.plan.size - size );
        for ( uint64_t i = 0; i < size; ++i ) {
            CHECK( written[dst + i] == 0 );
            written[dst + i] = 1;
            result.data[dst + i] = from[i];
        }
    };
    for ( const auto& copy : result.plan.copies ) {
        CHECK( copy.size > 0 && copy.stretch < packs.size() && copy.src + copy.size <= packs[copy.stretch].size() );
        put( packs[copy.stretch].data() + copy.src, copy.dst, copy.size );
    }
    for ( const auto& fixup : result.plan.fixups ) {
        CHECK( fixup.fileOffset + fixup.size <= data.size() );
        put( data.data() + fixup.fileOffset, fixup.dst, fixup.size );
    }
    CHECK( std::count( written.begin(), written.end(), 1 ) == (long)written.size() );
    return result;
}

/** assemble against the model's slice for the same lines. */
Assembled
checkAssembly( const Bytes& data, const std::vector<size_t>& cuts, uint8_t nl, uint8_t dl, uint32_t j, uint64_t first, uint64_t count,
               size_t chunk )
{
    const auto model = fieldColumn( data.data(), data.size(), nl, dl, j );
    const uint64_t n = model.sizes.size();
    const uint64_t lo = std::min( first, n ), hi = count > n - lo ? n : lo + count;
    const auto got = assemble( data, cuts, nl, dl, j, first, count, chunk );
    CHECK( got.lines == hi - lo );
    CHECK( got.plan.size == model.offsets[hi] - model.offsets[lo] );
    CHECK( std::equal( got.data.begin(), got.data.end(), model.data.begin() + (long)model.offsets[lo] ) );
    return got;
}

void
testModel()
{
    const auto text = bytesOf( "a\t12\t\n\n-7\n\t\t+3" );
    const auto c0 = fieldColumn( text.data(), text.size(), '\n', '\t', 0 );
    CHECK( c0.data == bytesOf( "a-7" ) );
    CHECK( ( c0.sizes == std::vector<int64_t>{ 1, 0, 2, 0 } ) );
    CHECK( ( c0.offsets == std::vector<uint64_t>{ 0, 1, 1, 3, 3 } ) );
    const auto c1 = fieldColumn( text.data(), text.size(), '\n', '\t', 1 );
    CHECK( c1.data == bytesOf( "12" ) );
    CHECK( ( c1.sizes == std::vector<int64_t>{ 2, -1, -1, 0 } ) );
    const auto c2 = fieldColumn( text.data(), text.size(), '\n', '\t', 2 );
    CHECK( c2.data == bytesOf( "+3" ) );
    CHECK( ( c2.sizes == std::vector<int64_t>{ 0, -1, -1, 2 } ) );
    CHECK( ( c2.offsets == std::vector<uint64_t>{ 0, 0, 0, 0, 2 } ) );
    const auto c3 = fieldColumn( text.data(), text.size(), '\n', '\t', 1023 );
    CHECK( c3.data.empty() && ( c3.sizes == std::vector<int64_t>{ -1, -1, -1, -1 } ) );
    const auto none = fieldColumn( nullptr, 0, '\n', '\t', 0 );
    CHECK( none.data.empty() && none.sizes.empty() && ( none.offsets == std::vector<uint64_t>{ 0 } ) );
    /* the model against the field spans of bz2_fields.hpp */
    std::mt19937_64 rng( 0xC01 );
    for ( int round = 0; round < 500; ++round ) {
        const uint8_t alphabet[] = { 'a', ',', '\n', 0, 0xFF, ',', 'b' };
        Bytes data( rng() % 100 );
        for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
        const uint32_t j = (uint32_t)( rng() % 4 );
        const auto model = fieldColumn( data.data(), data.size(), '\n', ',', j );
        const auto spans = stitchedFields( { { 0, summariseFields( data.data(), data.size(), '\n', ',', j, 7 ) } }, j );
        CHECK( spans.size() == model.sizes.size() && model.offsets.size() == spans.size() + 1 );
        for ( size_t i = 0; i < spans.size(); ++i ) {
            CHECK( spans[i].size == model.sizes[i] );
            const uint64_t size = spans[i].size > 0 ? (uint64_t)spans[i].size : 0;
            CHECK( model.offsets[i + 1] - model.offsets[i] == size );
            CHECK( std::equal( model.data.begin() + (long)model.offsets[i], model.data.begin() + (long)model.offsets[i + 1],
                               data.begin() + (long)( size > 0 ? spans[i].start : 0 ) ) );
        }
    }
}

void
testRandomAssemblies()
{
    std::mt19937_64 rng( 0xF1E1DC01 );
    size_t patched = 0, fixups = 0, windows = 0;
    for ( int round = 0; round < 4000; ++round ) {
        const uint8_t nl = round % 5 == 0 ? 0 : '\n';
        const uint8_t dl = (uint8_t)( round % 4 == 0 ? 0xFF : round % 4 == 1 ? ',' : '\t' );
        const uint8_t alphabet[] = { 'a', dl, nl, 'q', 0xFE, dl, 'b', 'c' };
        Bytes data( rng() % 160 );
        for ( auto& b : data ) b = alphabet[rng() % sizeof( alphabet )];
        const uint32_t j = (uint32_t)( round % 7 == 0 ? 1023 : rng() % 4 );
        std::vector<size_t> cuts( rng() % 7 );
        for ( auto& cut : cuts ) cut = rng() % ( data.size() + 1 );
        const size_t chunk = 1 + rng() % 64;
        const auto whole = checkAssembly( data, cuts, nl, dl, j, 0, ~uint64_t( 0 ), chunk );
        patched += whole.patched;
        fixups += whole.plan.fixups.size();
        const uint64_t first = rng() % ( whole.lines + 2 ), count = rng() % ( whole.lines + 2 );
        windows += checkAssembly( data, cuts, nl, dl, j, first, count, chunk ).lines;
    }
    /* the cases do patch, and some patched lines have no field to fetch */
    CHECK( patched > 4000 && fixups > 1000 && fixups < patched && windows > 4000 );
}

void
testNamedAssemblies()
{
    /* a line through three stretches, its field's start in the first and its end in the third */
    const auto text = bytesOf( "k,abcdefghij,x\nl,m\n" );
    for ( uint32_t j = 0; j < 4; ++j ) {
        const auto got = checkAssembly( text, { 4, 9 }, '\n', ',', j, 0, ~uint64_t( 0 ), 3 );
        CHECK( got.patched == 1 && got.lines == 2 );
        CHECK( got.plan.fixups.size() == ( j < 3 ? 1u : 0u ) );
    }
    const auto long1 = checkAssembly( text, { 4, 9 }, '\n', ',', 1, 0, ~uint64_t( 0 ), 3 );
    CHECK( ( long1.plan.fixups == std::vector<ColumnFixup>{ { 2, 10, 0 } } ) );
    CHECK( ( long1.plan.copies == std::vector<ColumnCopy>{ { 2, 1, 10, 1 } } ) );   /* the third stretch packed "x" for it */
    /* every byte a stretch of its own */
    std::vector<size_t> everywhere;
    for ( size_t at = 1; at < text.size(); ++at ) everywhere.push_back( at );
    for ( uint32_t j = 0; j < 4; ++j ) checkAssembly( text, everywhere, '\n', ',', j, 0, ~uint64_t( 0 ), 1 );
    /* patched lines whose field is missing (no fix-up) and empty (a fix-up of no bytes) */
    const auto gaps = bytesOf( "a,,c\nd\n,e\n" );
    const auto missing = checkAssembly( gaps, { 6 }, '\n', ',', 1, 0, ~uint64_t( 0 ), 64 );
    CHECK( missing.patched == 1 && missing.plan.fixups.empty() );
    const auto empty = checkAssembly( gaps, { 2 }, '\n', ',', 1, 0, ~uint64_t( 0 ), 64 );
    CHECK( empty.patched == 1 && ( empty.plan.fixups == std::vector<ColumnFixup>{ { 2, 0, 0 } } ) );
    /* a tail: always a patch, inside one stretch or across two */
    const auto tailed = bytesOf( "a,b\nc,tail" );
    const auto t0 = checkAssembly( tailed, {}, '\n', ',', 1, 0, ~uint64_t( 0 ), 64 );
    CHECK( t0.patched == 1 && ( t0.plan.fixups == std::vector<ColumnFixup>{ { 6, 4, 1 } } ) );
    const auto t1 = checkAssembly( tailed, { 8 }, '\n', ',', 1, 1, 5, 64 );
    CHECK( t1.lines == 1 && t1.plan.copies.empty() && ( t1.plan.fixups == std::vector<ColumnFixup>{ { 6, 4, 0 } } ) );
    const auto t2 = checkAssembly( tailed, { 8 }, '\n', ',', 1, 0, 1, 64 );
    CHECK( t2.lines == 1 && t2.patched == 0 && t2.plan.size == 1 );
    /* no lines at all */
    const auto nothing = checkAssembly( {}, {}, '\n', ',', 0, 0, ~uint64_t( 0 ), 64 );
    CHECK( nothing.lines == 0 && nothing.plan.size == 0 && nothing.plan.copies.empty() && nothing.plan.fixups.empty() );
    CHECK( checkAssembly( text, { 4, 9 }, '\n', ',', 1, 2, 7, 3 ).lines == 0 );
    CHECK( checkAssembly( text, { 4, 9 }, '\n', ',', 1, 0, 0, 3 ).lines == 0 );
    const auto planned = planColumnAssembly( {}, {} );
    CHECK( planned.size == 0 && planned.copies.empty() && planned.fixups.empty() );
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
testRefusals()
{
    CHECK( refused( [] { (void)planColumnAssembly( { { 1, 2, 5, 1 } }, {} ); } ) );                       /* does not begin at 0 */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 1 }, { 3, 1, 1, 1 } }, {} ); } ) );       /* a gap */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 0, 5, 0 } }, {} ); } ) );                       /* bytes for no line */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 6 } }, {} ); } ) );                       /* first line > pack */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 1 } }, { { 1, 0, 3 } } ); } ) );          /* no first line */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 1 } }, { { 3, 0, 3 } } ); } ) );          /* behind the tail */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 1 } }, { { 2, 0, 3 }, { 2, 0, 3 } } ); } ) );   /* two tails */
    CHECK( refused( [] { (void)planColumnAssembly( { { 0, 2, 5, 1 } }, { { 2, 0, 3 }, { 0, 0, 3 } } ); } ) );   /* descending */
    const uint64_t huge = ~uint64_t( 0 ) - 10;
    CHECK( refused( [=] { (void)planColumnAssembly( { { 0, 1, huge, 0 }, { 1, 1, 11, 0 } }, {} ); } ) );  /* beyond 64 bits */
    CHECK( refused( [=] { (void)planColumnAssembly( { { 0, 1, huge, 0 } }, { { 1, 0, 11 } } ); } ) );
    CHECK( planColumnAssembly( { { 0, 1, huge, 0 } }, { { 1, 0, 10 } } ).size == ~uint64_t( 0 ) );
}

/** Sizes whose sum passes 2^32 and 2^33: every destination offset against a 128-bit running sum. */
void
testBeyond32Bits()
{
    std::mt19937_64 rng( 0xB16 );
    for ( int round = 0; round < 200; ++round ) {
        std::vector<ColumnStretch> stretches;
        std::vector<ColumnPatch> patches;
        std::vector<std::pair<bool, unsigned __int128> > expected;   /* fix-up or copy, its dst, in order */
        unsigned __int128 sum = 0;
        uint64_t line = 0;
        const size_t n = 2 + rng() % 12;
        for ( size_t k = 0; k < n; ++k ) {
            if ( rng() % 5 == 0 ) {
                stretches.push_back( {} );   /* closes none of the wanted lines */
                continue;
            }
            const uint64_t take = 1 + rng() % 1000, total = ( rng() % 3 ) * ( 1ull << 31 ) + rng() % 5000;
            const uint64_t firstSize = take == 1 ? total : std::min<uint64_t>( total, rng() % ( ( 1ull << 32 ) + 77 ) );
            stretches.push_back( { line, take, total, firstSize } );
            uint64_t src = 0;
            if ( rng() % 2 == 0 ) {
                const int64_t size = rng() % 4 == 0 ? -1 : (int64_t)( rng() % ( ( 1ull << 33 ) + 5 ) );
                patches.push_back( { line, rng() >> 8, size } );
                if ( size >= 0 ) {
                    expected.emplace_back( true, sum );
                    sum += (uint64_t)size;
                }
                src = firstSize;
            }
            if ( total > src ) {
                expected.emplace_back( false, sum );
                sum += total - src;
            }
            line += take;
        }
        if ( rng() % 2 == 0 ) {
            patches.push_back( { line, rng() >> 8, (int64_t)( ( 1ull << 32 ) + rng() % 99 ) } );
            expected.emplace_back( true, sum );
            sum += (uint64_t)patches.back().size;
        }
        const auto plan = planColumnAssembly( stretches, patches );
        CHECK( (unsigned __int128)plan.size == sum && plan.copies.size() + plan.fixups.size() == expected.size() );
        size_t copy = 0, fixup = 0;
        for ( const auto& [isFixup, dst] : expected ) {
            if ( isFixup ) {
                CHECK( fixup < plan.fixups.size() && (unsigned __int128)plan.fixups[fixup].dst == dst );
                ++fixup;
            } else {
                CHECK( copy < plan.copies.size() && (unsigned __int128)plan.copies[copy].dst == dst );
                CHECK( stretches[plan.copies[copy].stretch].total == plan.copies[copy].src + plan.copies[copy].size );
                ++copy;
            }
        }
        if ( round == 0 ) CHECK( sum > 0 );
    }
    /* a fixed one, past 2^33 */
    const uint64_t g = 1ull << 32;
    const auto plan = planColumnAssembly( { { 0, 3, g + 7, 5 }, { 0, 0, 0, 0 }, { 3, 2, g, g - 1 } }, { { 3, 99, (int64_t)( g + 1 ) }, { 5, 7, 3 } } );
    CHECK( ( plan.copies == std::vector<ColumnCopy>{ { 0, 0, 0, g + 7 }, { 2, g - 1, 2 * g + 8, 1 } } ) );
    CHECK( ( plan.fixups == std::vector<ColumnFixup>{ { 99, g + 1, g + 7 }, { 7, 3, 2 * g + 9 } } ) );
    CHECK( plan.size == 2 * g + 12 );
}
}  // namespace

int
main()
{
    testModel();
    testNamedAssemblies();
    testRandomAssemblies();
    testRefusals();
    testBeyond32Bits();
    std::printf( "fieldcols cases ok\n" );
    return 0;
}
